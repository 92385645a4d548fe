/* libammsb_average.so: the running mean of pi and beta over the iterations of the chain, at mini-batch cost.
 *
 * The learner is a stochastic-gradient MCMC sampler: after an iteration (pi, beta) hold one draw.  Sample t (t = 1, 2, ...)
 * is the state after the t-th iteration since the average was started, and the quantity kept here is the mean of the
 * samples 1..n.  An iteration changes only the pi rows of its mini-batch nodes, so the mean of pi is LAZY: per row a,
 *
 *     mean[a, :]  is the mean of the samples 1 .. last[a]           (last[a] == 0: nothing stored yet), and
 *     the samples last[a] + 1 .. n of that row all equal the current pi[a, :].
 *
 * A row is brought up to date ("flushed") just before it is overwritten and once more when the mean is read:
 * O(mini-batch x K) bytes per iteration instead of O(N x K), over every iteration and not a thinned subset.  The caller
 * keeps the invariant: flush the rows an iteration is about to change with the n BEFORE that iteration, and flush every
 * row (a row range) with the current n before reading mean.  n must not be smaller than any last[a] it meets.
 *
 * Flushing row a to n, with old = last[a] and w = n - old (the samples that equal the current row):
 *     w == 0    nothing is read or written;
 *     old == 0  mean[a, :] = pi[a, :], and mean is NOT read: the mean buffer needs no initialisation and may hold NaNs;
 *     else      r = float(w) / float(n);  mean[a, k] = mean[a, k] + r * (pi[a, k] - mean[a, k])
 * in separately rounded binary32 operations (a divide, a subtract, a multiply, an add: no fused multiply-add), so that
 * a numpy float32 statement of the same four operations gives the same bits.  last[a] becomes n.
 * Each flush moves the stored mean by at most 4 * 2^-24 (values in [0, 1]) beside the exact recurrence, which contracts
 * an earlier error by 1 - r: after F flushes a row is within F * 2^-22 of the mean of its samples.
 *
 * beta is small (2K floats) and changes whole every iteration: its mean is kept in binary64, eagerly, and rounded to
 * binary32 once for the consumers that take a float vector.
 *
 * The conventions of the other post-fit libraries: a library, a header and a signature table of its own; the ammsb_rpm of
 * ammsb.h is taken by pointer (copied before return) and no ammsb_ctx is needed.  Calls only enqueue work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation; the caller owns every buffer.
 * Return values are the codes of ammsb.h (0 = AMMSB_OK, AMMSB_EINVAL, AMMSB_EHIP); a bad argument is refused before
 * anything is launched. */
#ifndef AMMSB_AVERAGE_H_
#define AMMSB_AVERAGE_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_AVERAGE_MAX_COLS 8192u

/* Flush rows of pi into mean, to the sample count n.  pi and mean: descriptors of equal geometry (rows, columns, rows per
 * block, blocks) over different memory; last: [pi->num_rows] u32, device, zero when the average starts.
 * nodes != NULL: the rows nodes[0 .. count) (device pointer; `first` must be 0).  An id >= num_rows is skipped.  One lane
 * per listed row claims it with old = atomic exchange(last[a], n): a node listed twice (or many times) is flushed once,
 * the later claimants see w == 0.  n must be >= 1.
 * nodes == NULL: the rows first .. first + count, which hold no repeats: plain loads and stores of last.  n == 0 is a
 * valid no-op.
 * One group of lanes owns a row (the smallest power of two >= ceil(K / 4), at most a wave); 16-byte loads and stores where
 * K is a multiple of 4 and every block of both matrices is 16-byte aligned, 4-byte ones otherwise: same results.
 * AMMSB_EINVAL: a NULL pointer, descriptors that differ or whose blocks do not cover num_rows, num_cols == 0 or > 8192,
 * pi and mean sharing a block, a node list with first != 0 or with n == 0, first + count > num_rows for a range, count
 * >= 2^32. */
int ammsb_average_rows(const ammsb_rpm* pi, const ammsb_rpm* mean, uint32_t* last, const uint32_t* nodes, uint64_t first,
                       uint64_t count, uint32_t n, void* stream);

/* mean64[i] = mean64[i] + (double(x[i]) - mean64[i]) / double(n) for i < len, in separately rounded binary64 operations;
 * n == 1 writes double(x[i]) and does not read mean64.  x: [len] float, mean64: [len] double (8-byte aligned), device.
 * AMMSB_EINVAL: a NULL pointer with len > 0, a misaligned mean64, n == 0, len >= 2^32. */
int ammsb_average_vector(const float* x, double* mean64, uint64_t len, uint32_t n, void* stream);

/* out32[i] = mean64[i] rounded to binary32 (to nearest, ties to even), i < len.  AMMSB_EINVAL as above. */
int ammsb_average_round(const double* mean64, float* out32, uint64_t len, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first): "average_rows_v4<list>",
 * "average_rows_v4<range>", "average_rows_s1<list>", "average_rows_s1<range>", "average_vector", "average_round". */
const char* ammsb_average_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_average_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_AVERAGE_H_ */
