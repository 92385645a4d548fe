/* libammsb_spread.so: the running mean AND variance of pi and beta over the iterations of the chain, at mini-batch cost.
 *
 * The lazy scheme of ammsb_average.h carries a second moment as well.  Sample t (t = 1, 2, ...) is the state after the
 * t-th iteration since the spread was started; per row a,
 *
 *     mean[a, :] and var[a, :]  are the mean and the POPULATION variance (divisor last[a], not last[a] - 1) of the samples
 *                               1 .. last[a]                          (last[a] == 0: nothing stored yet), and
 *     the samples last[a] + 1 .. n of that row all equal the current pi[a, :].
 *
 * The caller keeps the invariant of ammsb_average.h: flush the rows an iteration is about to change with the n BEFORE that
 * iteration, and flush every row (a row range) with the current n before reading mean or var.
 *
 * Merging "w copies of x" into old samples of mean m and variance V, with n = old + w, r = w / n and d = x - m, is exact:
 *     m' = m + r d,        V' = (1 - r) V + r (1 - r) d^2 = V + r ((1 - r) d^2 - V).
 * Flushing row a to n, with old = last[a] and w = n - old:
 *     w == 0    nothing is read or written;
 *     old == 0  mean[a, :] = pi[a, :] and var[a, :] = 0; neither mean nor var is read: the buffers need no initialisation
 *               and may hold NaNs;
 *     else      nine separately rounded binary32 operations per entry (no fused multiply-add), in this order:
 *                   r     = float(w) / float(n)
 *                   d     = pi - mean
 *                   mean' = mean + r * d           (a multiply, an add: the three operations of ammsb_average.h, so mean
 *                                                   comes out bit for bit as ammsb_average_rows leaves it)
 *                   s     = 1.0f - r
 *                   e     = d * d
 *                   e     = e * s
 *                   e     = e - var
 *                   e     = r * e
 *                   var'  = var + e
 * and last[a] becomes n.  A numpy float32 statement of the same operations gives the same bits.
 *
 * What is stored is the variance itself (at most 1/4 for values in [0, 1]), not a sum of squares, so an earlier error
 * contracts by 1 - r as it does for the mean.  Two invariants, for pi and mean in [0, 1] and var >= 0 on entry:
 *
 *   var >= 0 ALWAYS.  r = fl(w / n) <= 1 and e2 = fl(fl(d d) s) >= 0.  Rounding is monotone, so where e3 = fl(e2 - var) is
 *   negative, |e3| <= var, and |fl(r e3)| <= |e3| <= var: var + fl(r e3) >= 0 before its rounding and therefore after it.
 *   Where e3 >= 0 two non-negative numbers are added.  (A NaN in pi stays a NaN.)
 *
 *   THE ERROR against the exact variance of the samples, for n <= 2^24 (w and n are then exact as floats).  Write h = 2^-25:
 *   every intermediate above has magnitude <= 1, so each rounding moves it by at most h.  Let mu = |mean - exact mean| and
 *   eps = var - exact variance before the flush.  Then d is off by at most mu + h; fl(d d) by 2 (mu + h) + (mu + h)^2 + h;
 *   s by 2 h (r's rounding and its own); e2 = fl(fl(d d) s) from (1 - r) d^2 by 2 mu + (mu + h)^2 + 6 h; and
 *       var' = exact' + (1 - r) eps + r (e2's error + h) + (r's error) e3 + two roundings,
 *       |eps'| <= (1 - r) |eps| + r D + 3 h,          D = 2 mu + (mu + h)^2 + 7 h.
 *   This is a CONVEX combination of the old error and D, plus 3 h: the mean's error enters as a maximum, not as a sum over
 *   the flushes.  With mu <= (F - 1) 2^-22 before the F-th flush (ammsb_average.h) and D growing with F, induction gives
 *       |eps| after F flushes <= 3 h F + D(F) <= (9.5 F + 3.5) 2^-24 + (8 F + 1)^2 2^-50,
 *       |var - exact| <= 13 F 2^-24 + F^2 2^-43           (a = 13; the second-order term is the square of the mean's error),
 *   F the flushes that wrote the row.  (The first one is exact.)  At F = 200 this is 1.6e-4.
 *
 * beta is small and changes whole every iteration: its mean and its sum of squared deviations m2 are kept in binary64,
 * eagerly, by Welford's update; the population variance is m2 / n.
 *
 * The conventions of the other post-fit libraries: a library, a header and a signature table of its own; the ammsb_rpm of
 * ammsb.h is taken by pointer (copied before return) and no ammsb_ctx is needed.  Calls only enqueue work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation; the caller owns every buffer.
 * Return values are the codes of ammsb.h (0 = AMMSB_OK, AMMSB_EINVAL, AMMSB_EHIP); a bad argument is refused before
 * anything is launched. */
#ifndef AMMSB_SPREAD_H_
#define AMMSB_SPREAD_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_SPREAD_MAX_COLS 8192u

/* Flush rows of pi into mean and var, to the sample count n, in one pass.  pi, mean and var: descriptors of equal geometry
 * (rows, columns, rows per block, blocks) over different memory; last: [pi->num_rows] u32, device, zero when the spread
 * starts.  nodes, first, count, n, the claiming of a listed row by an atomic exchange of last[a] (a node listed many times
 * is flushed once), the plain loads and stores of a row range and the group of lanes that owns a row (the smallest power of
 * two >= ceil(K / 4), at most a wave) are those of ammsb_average_rows.  16-byte loads and stores where K is a multiple of 4
 * and every block of all three matrices is 16-byte aligned, 4-byte ones otherwise: same results.
 * AMMSB_EINVAL: a NULL pointer, descriptors that differ or whose blocks do not cover num_rows, num_cols == 0 or > 8192, two
 * of the three matrices sharing a block, a node list with first != 0 or with n == 0, first + count > num_rows for a range,
 * count >= 2^32, a misaligned last or nodes. */
int ammsb_spread_rows(const ammsb_rpm* pi, const ammsb_rpm* mean, const ammsb_rpm* var, uint32_t* last,
                      const uint32_t* nodes, uint64_t first, uint64_t count, uint32_t n, void* stream);

/* Welford's update of x [len] float as sample n, in separately rounded binary64 operations:
 *     delta = double(x[i]) - mean64[i];  mean64'[i] = mean64[i] + delta / double(n)     (as ammsb_average_vector: same bits)
 *     m2'[i] = m2[i] + delta * (double(x[i]) - mean64'[i])
 * n == 1 writes double(x[i]) and 0.0 and reads neither buffer.  mean64, m2: [len] double (8-byte aligned), device.
 * AMMSB_EINVAL: a NULL pointer with len > 0, a misaligned pointer, mean64 == m2, n == 0, len >= 2^32. */
int ammsb_spread_vector(const float* x, double* mean64, double* m2, uint64_t len, uint32_t n, void* stream);

/* The credible bound of the rows first .. first + count:
 *     out[a, k] = min(1, max(0, mean[a, k] + z * sqrt(var[a, k])))
 * in separately rounded binary32 operations (a square root, a multiply, an add), for any finite z; z < 0 gives the lower
 * bound.  The square root is the correctly rounded binary32 one, whatever the build's flags say about f32 sqrt: it is taken
 * in binary64 and rounded once more, which cannot differ from the direct rounding because 53 >= 2 * 24 + 2.  numpy.sqrt on
 * float32 gives the same bits.  A NaN in mean or var (a negative var included) gives 0: a NaN is never a member.
 * mean, var, out: equal geometry; out shares no block with mean or var.  16-byte accesses under the rule above.
 * AMMSB_EINVAL: a NULL pointer, bad or differing descriptors, out sharing a block with an input, a z that is not finite,
 * first + count > num_rows, count >= 2^32. */
int ammsb_spread_bound(const ammsb_rpm* mean, const ammsb_rpm* var, const ammsb_rpm* out, float z, uint64_t first,
                       uint64_t count, void* stream);

/* out[a - first] (double, 8-byte aligned, device; [count]) = the sum of row a of var, a in first .. first + count, in ONE
 * order whatever the width of the group of lanes, the alignment and the grid, so the same from run to run: the order
 * include/ammsb_reduce.h states for a row's sum.  There are 64 virtual lanes; virtual lane v adds the columns v, v + 64, ...
 * (ascending, each converted to binary64) into a binary64 0; then six butterfly levels at the distances 32, 16, 8, 4, 2, 1,
 * y[v] = x[v] + x[v + d] for v < d.  A group narrower than 64 lanes emulates the virtual lanes.
 * AMMSB_EINVAL: a NULL or misaligned pointer, a bad descriptor, first + count > num_rows, count >= 2^32. */
int ammsb_spread_rowsum(const ammsb_rpm* var, double* out, uint64_t first, uint64_t count, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first): "spread_rows_v4<list>",
 * "spread_rows_v4<range>", "spread_rows_s1<list>", "spread_rows_s1<range>", "spread_vector", "spread_bound_v4",
 * "spread_bound_s1", "spread_rowsum". */
const char* ammsb_spread_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_spread_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_SPREAD_H_ */
