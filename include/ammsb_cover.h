/* libammsb_cover.so: how well does the detected cover match a known one?  Per ground-truth community its best-matching
 * detected community and per detected community its best-matching ground-truth one -- what the best-match F1 of Yang &
 * Leskovec, averaged over both directions, is made of.
 *
 * Definitions (the contract):
 *   detected cover   D_k = {a : pi[a, k] >= thr}: a binary32 compare of the stored value, so a NaN is never a member
 *                    (ammsb_readout.h's definition).  d_k = |D_k| is an input: detected_size[K], 64-bit, on the device,
 *                    what the read-out's community sizes are at the same thr.  It counts all num_rows nodes, also the
 *                    nodes that no ground-truth community holds; restricting the comparison to covered nodes is not
 *                    done here.
 *   ground truth     G communities as a CSR: offsets[G + 1] u64 (non-decreasing, offsets[0] == 0, offsets[G] == M),
 *                    members[M] u32 node ids.  A member >= num_rows is invalid: it reads nothing and is counted only in
 *                    `skipped`.  Duplicates inside a community are counted as written.  t_g = the valid entries of g.
 *                    offsets lives on the device, so the call cannot check that it ascends from 0 to M: for offsets
 *                    that do not, every walk is still bounded by M and G (nothing is read or written out of range),
 *                    but the results are unspecified.  The Python and C++ layers check it on the host.
 *   overlap[g, k]    the sum over the valid members a of g of [pi[a, k] >= thr].
 *   best match of g  among the k with overlap > 0 the k that maximises F1(g, k) = 2 overlap / (t_g + d_k), compared as
 *                    a rational: o1 (t + d2) against o2 (t + d1) in 128-bit integers.  Equal rationals go to the lower
 *                    k; none with overlap > 0 gives -1.
 *   best match of k  among the g with overlap > 0 the g that maximises overlap / (t_g + d_k), compared the same way.
 *                    Equal rationals go to the lower g; none gives -1.
 * In numpy: M = pi >= np.float32(thr); overlap[g] = M[members_g].sum(0); the argmax by integer cross-multiplication.
 * Integer counts and integer compares only, and a maximum under a total order does not depend on the order of arrival:
 * every output is exact and the same from run to run.
 *
 * Outputs: truth_best[G] i32, truth_overlap[G] u32 (the overlap with the best match, 0 for none), truth_size[G] u32
 * (= t_g); detected_best[K] i32, detected_overlap[K] u32; skipped u64 (set, not added to); and, when the caller passes
 * a buffer, the dense overlap[G, K] u32 (for small G, for tests, and for measures that need every pair).
 *
 * Derived measures (float64 on the host; mcmc::Learner::WriteCoverMatch and _cover.py use these formulas):
 *   F1 = 2 o / (t + d),   Jaccard = o / (t + d - o)   (the same argmax)
 *   f1_truth    = the mean of F1(g, best) over the g with t_g > 0, an unmatched g scoring 0
 *   f1_detected = the same over the k with d_k > 0
 *   avg_f1      = (f1_truth + f1_detected) / 2;  each is -1 where its mean is over nothing.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  The call only enqueues work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): memsets and kernels, no allocation, no synchronisation.  Return values
 * are the codes of ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used: a NULL
 * pi, detected_size, skipped, detected_best or detected_overlap; with G > 0 a NULL offsets, truth_best, truth_overlap
 * or truth_size; with M > 0 a NULL members or workspace; thr negative, NaN or infinite; num_cols == 0 or > 8192;
 * num_rows >= 2^32; a descriptor whose blocks do not cover num_rows; G >= 2^31 or M >= 2^32 (the outputs are 32-bit);
 * a workspace that is smaller than ammsb_cover_workspace_bytes or not 8-byte aligned.
 * G == 0 or M == 0 is a valid call without a device: it launches nothing and writes nothing, so every community is
 * unmatched -- the caller presets -1 / 0.
 *
 * The work is a segmented reduction over `members`.  A unit is AMMSB_COVER_UNIT consecutive entries; a wave of a
 * persistent grid takes a unit, so every unit reads the same number of rows of pi whatever the sizes of the
 * communities.  It finds the communities its unit spans from `offsets`.  A community that lies inside the unit is
 * finished in place; one that crosses a unit boundary adds its partial counts into the workspace row of the unit it
 * starts in (at most one such community per unit), and a second launch finishes those rows. */
#ifndef AMMSB_COVER_H_
#define AMMSB_COVER_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_COVER_MAX_COLS 8192u
#define AMMSB_COVER_UNIT 128u

/* Bytes of the workspace of a cover of num_members entries against num_cols communities, with U = ceil(num_members /
 * AMMSB_COVER_UNIT) and W = ceil(num_cols / 64):  8 num_cols (the running best of every detected community)
 * + 8 ceil(U / 2) (the valid entries of the crossing communities) + 256 U W (their partial counts).
 * 0 for a shape the library refuses, and for num_members == 0. */
uint64_t ammsb_cover_workspace_bytes(uint64_t num_members, uint32_t num_cols);

/* overlap: [G, K] or NULL.  Every word of every output is written (G > 0 and M > 0). */
int ammsb_cover_match(const ammsb_rpm* pi, float thr, const uint64_t* offsets, uint64_t num_truth,
                      const uint32_t* members, uint64_t num_members, const uint64_t* detected_size,
                      int32_t* truth_best, uint32_t* truth_overlap, uint32_t* truth_size, int32_t* detected_best,
                      uint32_t* detected_overlap, uint64_t* skipped, uint32_t* overlap, void* workspace,
                      uint64_t workspace_bytes, void* stream);

/* Name of the counting form the calling thread's last successful call took ("" before the first):
 *   cover_fast      K a multiple of 256 and 16-byte aligned blocks: a wave per row, 16-byte loads in chunks of 1024
 *                   columns; lane l owns columns 256 i + 4 l + c, counted in wave-private LDS words that only that
 *                   lane touches; the next chunk (or the next valid row's first) is requested before this one's hits
 *                   are added.
 *   cover_generic   every other 1 <= K <= 8192, and misaligned blocks: scalar loads, lane l owns columns 64 j + l; the
 *                   same pipeline.
 * Both are followed by
 *   cover_finish    a wave per workspace row that a crossing community used: the same epilogue (lane-local best, wave
 *                   reduction of the rational compare, one 64-bit compare-and-swap loop per non-zero overlap).
 *   cover_unpack    the running best of every detected community into detected_best / detected_overlap. */
const char* ammsb_cover_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_cover_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_COVER_H_ */
