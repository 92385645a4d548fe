/* libammsb_readout.so: node memberships and community sizes read out of a fitted pi on the device.
 *
 * For a row p = pi[a, 0..K), an integer 1 <= T <= 16 and a threshold thr >= 0 (binary32):
 *   ids[a, 0..T), weights[a, 0..T)   the columns of p ordered by value descending, EQUAL VALUES BY COLUMN ASCENDING,
 *                                    cut to the first T.  A slot whose value is < thr, or whose rank is >= K, holds
 *                                    id = 0xFFFFFFFF (AMMSB_READOUT_NONE), weight = 0.  Weights are the stored binary32
 *                                    values, untouched: no arithmetic is done on them, every result here is exact.
 *   count[a]                         number of columns with p[k] >= thr, NOT capped at T (count > T = truncated).
 *   sizes[k] (u64, K entries)        number of read-out rows with pi[a, k] >= thr, also uncapped; a row that is read
 *                                    twice (a node list with repeats, two calls) counts twice.
 * pi holds finite values >= 0 by construction (MAX(., 1e-24), then a division by the row sum).  NaN and negative
 * entries (-0.0 included) are outside the contract: they are never selected ahead of a value >= 0, but which slot
 * they take, and whether they are counted, is unspecified.
 *
 * One streaming pass over the rows.  Two kernel forms, same results: a register form for K a multiple of 256 (16-byte
 * loads; needs 16-byte aligned blocks, which hipMalloc and torch give) and a generic form for every other
 * 1 <= K <= 8192.  A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are
 * unchanged; the ammsb_rpm of ammsb.h is taken by pointer (copied before return) and no ammsb_ctx is needed.
 * Calls only enqueue work on `stream` (a hipStream_t as void*, NULL = the null stream): no allocation, no
 * synchronisation.  Return values are the codes of ammsb.h (0 = AMMSB_OK, AMMSB_EINVAL, AMMSB_EHIP). */
#ifndef AMMSB_READOUT_H_
#define AMMSB_READOUT_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_READOUT_MAX_TOP 16u
#define AMMSB_READOUT_MAX_COLS 8192u
#define AMMSB_READOUT_NONE 0xFFFFFFFFu

/* Rows row_lo .. row_lo + n_rows of pi when nodes == NULL, otherwise rows nodes[0 .. n_rows) (device pointer; row_lo
 * must be 0; an entry >= pi->num_rows reads nothing and yields sentinels and count 0).  Output row i belongs to input
 * row i: ids, weights: [n_rows, T]; count: [n_rows]; all device pointers.  sizes: [K] u64 or NULL; it is ACCUMULATED
 * into (integer adds: the result does not depend on order), so row slabs can be read out in pieces of bounded output;
 * the caller zeroes it.  ids, weights and count may all three be NULL when sizes is given (sizes only: T is ignored).
 * AMMSB_EINVAL before anything is launched: T == 0 or > 16, thr negative or NaN, row_lo + n_rows > num_rows, a node
 * list with row_lo != 0, some but not all of ids / weights / count NULL, nothing to write at all, num_cols == 0 or
 * > 8192, num_rows or n_rows >= 2^32, a descriptor whose blocks do not cover num_rows. */
int ammsb_readout_top(const ammsb_rpm* pi, const uint32_t* nodes, uint64_t row_lo, uint64_t n_rows, uint32_t T,
                      float thr, uint32_t* ids, float* weights, uint32_t* count, uint64_t* sizes, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first):
 * "readout_fast<V>" (V = 16-byte loads per lane the instance holds: 1, 2, 4, 8, 16, 32) or "readout_generic". */
const char* ammsb_readout_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_readout_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_READOUT_H_ */
