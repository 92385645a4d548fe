/* libammsb_reduce.so: merge and drop communities of a fitted model -- pi, phi_sum and theta at K' < K columns.
 *
 * A PLAN over K communities is map[K] of int32: map[k] = j sends community k to the new community j in [0, K'), map[k] = -1
 * drops k.  Every new community has at least one source, so 1 <= K' <= K <= 8192.  The device takes the plan as its inverse
 * in CSR form: src_off[K' + 1] and src[src_off[K']], the sources of each j ascending; the hosts build and validate it, the
 * kernels trust it.  The plan DROPS iff some map[k] = -1.
 *
 * For row a, every operation an IEEE operation rounded by itself (no contraction):
 *
 *   1. t[j] = pi[a, src0] + pi[a, src1] + ...  in binary32, left to right over the ascending sources of j; one source is a
 *      copy of its bits.
 *   2. The plan does not drop:  pi'[a, j] = t[j], phi_sum'[a] = phi_sum[a].  The mass of a row is unchanged in exact
 *      arithmetic; the identity and a permutation come out bit for bit.
 *   3. The plan drops:  s is the binary64 sum of the t[j] in ONE order, whatever the kernel form, the width of the group of
 *      lanes, the alignment and the grid: there are 64 virtual lanes; virtual lane v adds the columns j = v, v + 64, ...
 *      (ascending) into a binary64 0; then six butterfly levels at the distances 32, 16, 8, 4, 2, 1, each x = x + x_partner
 *      (the sum of all 64 by halving: y[v] = x[v] + x[v + 32] for v < 32, and so on).  A group narrower than 64 lanes
 *      emulates the virtual lanes.  With sf = (float) s:
 *          pi'[a, j] = t[j] / sf         one binary32 division
 *          phi_sum'[a] = phi_sum[a] * sf one binary32 multiplication
 *   4. The plan drops and !(sf > 0) -- zero, a NaN, a row whose whole mass was dropped: the row is EMPTIED,
 *          pi'[a, j] = 1.0f / (float) K' for every j, phi_sum'[a] = phi_sum[a],
 *      and *emptied (uint64, device, zeroed by the caller) is incremented once for the row, by an atomic add.
 *
 * Against the exact quotient: n_j - 1 additions, one rounding of s, one division, so
 *      |pi'[a, j] - exact| <= (n_j + 3) * 2^-24 * exact,      n_j the number of sources of j.
 *
 * theta is [K, 2]: theta'[j, i] is the binary32 left-to-right sum of theta[k, i] over the ascending sources of j --
 * pseudo-counts add, those of a dropped community are discarded.  beta' follows from theta' by ammsb_beta_from_theta.
 *
 * The conventions of the other post-fit libraries: a library, a header and a signature table of its own; the ammsb_rpm of
 * ammsb.h is taken by pointer (copied before return) and no ammsb_ctx is needed.  Calls only enqueue work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation; the caller owns every buffer.
 * Return values are the codes of ammsb.h (0 = AMMSB_OK, AMMSB_EINVAL, AMMSB_EHIP); a bad argument is refused before
 * anything is launched. */
#ifndef AMMSB_REDUCE_H_
#define AMMSB_REDUCE_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_REDUCE_MAX_COLS 8192u

/* Rows first .. first + count of pi [N, K] into out_pi [N, K'] and of phi_sum [N] into out_phi_sum [N] (which may be
 * phi_sum itself).  pi and out_pi: descriptors with the same rows, over different memory; their blocks need not be cut
 * alike.  new_cols = K' = out_pi->num_cols (the length of the CSR; stated twice on purpose).  src_off [K' + 1] and src: u32,
 * device.  src_off == NULL states that every new community has exactly one source, src[j] (a permutation or a pruning):
 * the call is then a pure gather, the SELECT form; otherwise the MERGE form walks the CSR.  Both give the same bits for the
 * same plan.  drops != 0: steps 3 and 4 above, and emptied must not be NULL.
 * Callable slab by slab: nothing depends on the cut.
 * A group of lanes owns a row (the smallest power of two >= ceil(K / 4), at most a wave) and stages it in LDS once, with
 * 16-byte loads where K is a multiple of 4 and every block of pi is 16-byte aligned, 4-byte loads otherwise; lane l of the
 * group owns the output columns l, l + G, ... and walks their sources in the staged row.
 * AMMSB_EINVAL: a NULL pointer (src_off excepted), K or K' 0 or > 8192, K' > K, new_cols != K', descriptors whose rows
 * differ or whose blocks do not cover them, first + count > num_rows, out_pi sharing a block with pi, drops with emptied
 * NULL, a misaligned pointer. */
int ammsb_reduce_rows(const ammsb_rpm* pi, const float* phi_sum, const uint32_t* src_off, const uint32_t* src,
                      uint32_t new_cols, uint32_t drops, const ammsb_rpm* out_pi, float* out_phi_sum, uint64_t* emptied,
                      uint64_t first, uint64_t count, void* stream);

/* theta [old_cols, 2] -> out_theta [new_cols, 2] (different memory), one block.  src_off == NULL as above.
 * AMMSB_EINVAL: a NULL or misaligned pointer, old_cols or new_cols 0 or > 8192, new_cols > old_cols, out_theta == theta. */
int ammsb_reduce_theta(const float* theta, const uint32_t* src_off, const uint32_t* src, uint32_t old_cols,
                       uint32_t new_cols, float* out_theta, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first): "reduce_select_v4",
 * "reduce_select_s1", "reduce_merge_v4", "reduce_merge_s1", "reduce_theta". */
const char* ammsb_reduce_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_reduce_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_REDUCE_H_ */
