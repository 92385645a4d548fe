/* libammsb_linkcomm.so: which community explains a link, read out of a fitted (pi, beta) on the device.
 *
 * The model's probability of the link (a, b), with beta_k = beta[2k+1] and eps = Config::epsilon, is
 *     p(a, b) = eps (1 - sum_k pi[a,k] pi[b,k]) + sum_k pi[a,k] pi[b,k] beta_k
 * and term k of the second sum is the share of it owed to both ends acting in community k: t_k / p is the posterior
 * that (a, b) is a community-k link.  For every edge of a list this library writes the T largest terms with their
 * communities, p, and per community the number of edges whose largest term it holds.
 *
 * Terms are exact.  t_k = (pi[a,k] * pi[b,k]) * beta_k: two binary32 multiplications in this order, no contraction,
 * subnormal results kept, so a term is a function of the two rows and beta alone and swapping the ends gives the same
 * bits.  Slot j of an edge holds the j-th largest term that is > 0 and >= min_term; order is term descending, equal
 * terms (bit patterns) by community ascending; a term that is zero, negative or NaN never takes a slot; empty slots hold
 * AMMSB_LINKCOMM_NONE and term 0.  ids and terms equal the stable argsort of the numpy float32 statement bit for bit.
 *
 * prob[i] = eps + sum_k pi[a,k] pi[b,k] (beta_k - eps), as include/ammsb_linkpred.h defines it, evaluated in binary32 as
 * w_k = beta_k - eps, q_k = pi[a,k] * pi[b,k], s = sum_k q_k * w_k, p = s + eps.  The sum runs per lane over its columns
 * in ascending order and then over the 64 lanes as a butterfly.  Three roundings make a summand (w_k, q_k, q_k * w_k);
 * an addition rounds only when both operands are non-zero, i.e. when it merges two non-empty disjoint sets of summands,
 * and a summand passes through at most K - 1 such merges; + eps is one more.  At most K + 3 roundings touch a summand,
 * gamma_{K+3} < (K + 8) 2^-24 for K <= 8192, and results that underflow binary32 lose at most 2^-149 each:
 *     |prob - p64| <= (K + 8) 2^-24 M + 2^-100,   M = eps + sum_k pi[a,k] pi[b,k] |beta_k - eps|
 * against a float64 evaluation over the stored binary32 values -- the bound of ammsb_linkpred.h, NOT the bits of
 * ammsb_linkpred_pairs.
 *
 * sizes[k] += 1 for every edge whose slot 0 holds community k; sizes[K] += 1 for every edge with valid ends and an
 * empty slot 0 (the links no community explains at min_term).  Integer adds only (block-private u32 counters, flushed
 * with 64-bit atomics): exact and independent of scheduling.
 *
 * An edge is (a << 32) | b with the ends in either order; a == b is computed as written.  An edge with an end >=
 * num_rows reads nothing: it writes empty slots and prob = -1 and is counted nowhere.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  The call only enqueues work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation.  Return values are the codes of
 * ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used: NULL pi, beta or edges
 * with n > 0; every output NULL; exactly one of ids / terms NULL; T == 0 or T > 16 when ids is given; min_term negative,
 * NaN or infinite; epsilon negative, NaN or >= 1; num_cols == 0 or > 8192; num_rows >= 2^32; a descriptor whose blocks
 * do not cover num_rows.  n == 0 is a valid no-op without a device. */
#ifndef AMMSB_LINKCOMM_H_
#define AMMSB_LINKCOMM_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_LINKCOMM_MAX_TOP 16u
#define AMMSB_LINKCOMM_MAX_COLS 8192u
#define AMMSB_LINKCOMM_NONE 0xFFFFFFFFu

/* ids, terms: [n, T] or NULL (both or neither); prob: [n] or NULL; sizes: [K + 1], zeroed by the caller, or NULL.
 * ids == terms == NULL with sizes != NULL is the sizes-only pass: T is ignored and the call writes the K + 1 counters
 * (and prob, if given) and nothing else. */
int ammsb_linkcomm_edges(const ammsb_rpm* pi, const float* beta, float epsilon, const uint64_t* edges, uint64_t n,
                         uint32_t T, float min_term, uint32_t* ids, float* terms, float* prob, uint64_t* sizes,
                         void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first):
 *   linkcomm_fast_v{1,2,4}, linkcomm_fast_v4_chunked   K a multiple of 256 and 16-byte aligned blocks: 16-byte loads,
 *       both rows' loads issued together, the next edge's loads issued before this edge's selection rounds.  V = float4
 *       registers per lane and row: K <= 256 V, both rows in registers (v1, v2, v4); K > 1024 (v4_chunked) walks the
 *       rows in chunks of 1024 columns and keeps the wave's running list of T keys across chunks.
 *   linkcomm_generic         every other 1 <= K <= 8192: lane l owns columns l, l + 64, ..., scalar loads. */
const char* ammsb_linkcomm_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_linkcomm_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_LINKCOMM_H_ */
