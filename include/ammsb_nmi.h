/* libammsb_nmi.so: the overlapping NMI of the detected cover against a known one -- the pair pass over the dense
 * overlap[G, K] that ammsb_cover_match writes (include/ammsb_cover.h), slab by slab, to one running minimum per
 * ground-truth community and one per detected community.
 *
 * Definitions (the contract):
 *   N = the number of nodes.  X_g is ground-truth community g with t = t_g valid members (truth_size[G] u32, what
 *   ammsb_cover_match writes); Y_k = D_k = {a : pi[a, k] >= thr} with d = d_k (detected_size[K] u64, the read-out's
 *   community sizes at the same thr); o = overlap[g, k] as ammsb_cover.h defines it.
 *   Every probability is ONE integer subtraction, then ONE float64 division by N; never 1 - x / N.
 *     h(x)      = -(x / N) * log2(x / N) for an integer x > 0, h(0) = 0
 *     n11 = o,  n10 = t - o,  n01 = d - o,  n00 = N - t - d + o
 *     H(X_g)    = h(t) + h(N - t)
 *     H(Y_k)    = h(d) + h(N - d)
 *     J(g, k)   = (h(n11) + h(n00)) + (h(n01) + h(n10)), in that association
 *     a pair qualifies (Lancichinetti, Fortunato, Kertesz) iff n00 >= 0 and h(n11) + h(n00) >= h(n01) + h(n10)
 *     c_truth[g]    = the minimum over the qualifying k of max(0, J - H(Y_k)); +inf if none qualifies
 *     c_detected[k] = the minimum over the qualifying g of max(0, J - H(X_g)); +inf if none qualifies
 *   With this association an identical pair (t = d = o) gives exactly 0.  float64 throughout, no FMA contraction.
 *   Zero-overlap pairs are part of the definition: N = 1000, t = 1, d = 599, o = 0 qualifies.
 *
 * The shortcut.  -x log x is strictly subadditive, so for o = 0, t + d > 0 and 2 (t + d) < N
 *     h(d) + h(t) > -(s log2 s) > -((1 - s) log2 (1 - s)) = h(n00)   with s = (t + d) / N < 1 / 2,
 * by a margin of at least 1 / N >= 2^-32 (far above the rounding of the four terms): such a pair can never qualify, and
 * the kernel skips its logarithms.  (t = d = 0 is not skipped: both sides are 0 and the pair qualifies.)  Most entries of
 * a real overlap matrix are 0, so the pass is a stream of 4 G K bytes plus the logarithms of the pairs that remain.
 *
 * Inputs that break the contract are safe: n00 < 0, o > t or o > d mean "does not qualify"; t >= N or d >= N gives
 * H = 0; nothing is read or written out of range.  NMI is defined on sets: a ground truth that lists a node twice
 * inside one community is rejected by the Python and C++ layers, on the host.
 *
 * Host side (float64, sums in index order; _nmi.py and mcmc::Learner::CoverNMI use these formulas):
 *     H(X_g | Y) = min(c_truth[g], H(X_g)),   H(Y_k | X) = min(c_detected[k], H(Y_k))
 *     nmi_lfk = 1 - (mean over the g with H(X_g) > 0 of H(X_g | Y) / H(X_g) + the same over k) / 2;
 *               -1 if either side has nothing to average
 *     nmi_max = (sum H(X_g) - sum H(X_g | Y) + sum H(Y_k) - sum H(Y_k | X)) / 2 / max(sum H(X_g), sum H(Y_k))
 *               (McDaid, Greene, Hurley); -1 when the denominator is 0
 *
 * The running minima are non-negative doubles or +inf, whose bit patterns order as unsigned 64-bit integers: they are
 * combined with 64-bit unsigned atomic minima (vector atomics).  A minimum does not depend on the order of arrival, so
 * every output is the same from run to run and does not depend on how the matrix is cut into slabs.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged, no
 * ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h.  AMMSB_EINVAL, before anything is launched
 * and before any device pointer is used: a NULL detected_size, H_detected or c_detected; with G > 0 a NULL truth_size,
 * H_truth or c_truth; with Gs > 0 a NULL overlap; K == 0 or > 8192; N == 0 or >= 2^32; G >= 2^31; g0 + Gs > G. */
#ifndef AMMSB_NMI_H_
#define AMMSB_NMI_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_NMI_MAX_COLS 8192u

/* Writes H_truth[G] = H(X_g) and H_detected[K] = H(Y_k) and presets c_truth[G] and c_detected[K] to +inf. */
int ammsb_nmi_begin(uint64_t num_nodes, const uint32_t* truth_size, uint64_t num_truth, const uint64_t* detected_size,
                    uint32_t num_cols, double* H_truth, double* H_detected, double* c_truth, double* c_detected,
                    void* stream);

/* Folds one slab into the minima: overlap[Gs, K] holds rows g0 .. g0 + Gs - 1 of the overlap matrix, exactly what
 * ammsb_cover_match writes for that slice of the CSR (its dense output, rebased).  The other arrays are the ones
 * ammsb_nmi_begin was given, after it on the same stream.  Gs == 0 is a valid call that launches nothing. */
int ammsb_nmi_accumulate(const uint32_t* overlap, uint64_t g0, uint64_t num_slab_rows, uint64_t num_nodes,
                         const uint32_t* truth_size, uint64_t num_truth, const uint64_t* detected_size,
                         uint32_t num_cols, const double* H_truth, const double* H_detected, double* c_truth,
                         double* c_detected, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   nmi_begin     the entropies and the presets, a thread per community.
 *   nmi_fast      K a multiple of 4 and a 16-byte aligned overlap: a persistent grid over tiles of 4 rows x 1024
 *                 columns, a wave per row, 16-byte loads; lane l owns columns 256 i + 4 l + c of the chunk, keeps their
 *                 d and H(Y_k) in registers while its block stays in the chunk, and a private minimum per column that
 *                 it offers with one atomic per column when the block leaves the chunk; the row minimum is a wave
 *                 butterfly and one atomic; the next tile's row is requested before this one is worked on.
 *   nmi_generic   every other 1 <= K <= 8192, and a misaligned overlap: scalar loads, lane l owns columns 64 j + l; the
 *                 same pipeline. */
const char* ammsb_nmi_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_nmi_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_NMI_H_ */
