/* libammsb_linkpred.so: link probabilities predicted from a fitted (pi, beta) on the device.
 *
 * For nodes a, b, with beta_k = beta[2k+1] and eps = Config::epsilon:
 *     p(a, b) = eps + sum_k pi[a,k] pi[b,k] (beta_k - eps)
 * which is 1 - (the non-link likelihood of the perplexity pass, perplexity.cc:93-128).  The reference's LINK branch
 * leaves the (1 - sum_k pi pi) eps term out, so p here exceeds that branch's value by at most eps (1e-7 by default).
 * Evaluated in binary32 as  w_k = beta_k - eps,  s_ak = pi[a,k] * w_k,  acc = sum_k s_ak * pi[b,k],  p = acc + eps.
 *
 *   block, top   acc runs on the f32-input matrix core (v_mfma_f32_32x32x2_f32): per output one accumulator chain from
 *                +0 over ALL k in one fixed order, so a score is a function of (query row, candidate row, beta, eps)
 *                alone -- not of Q, T, the tile a pair falls in, the grid, or how the candidates are cut.  `top`
 *                selects from exactly the values `block` writes.
 *   pairs        a gather of two rows per pair, reduced over the lanes of a wave: the same bound, NOT the same bits as
 *                `block` (the summation order differs).
 * Accuracy of all three against a float64 evaluation over the stored binary32 pi, beta, eps:
 *     |got - p64| <= (K + 8) 2^-24 M + 2^-100,   M = eps + sum_k pi[a,k] pi[b,k] |beta_k - eps|.
 * Results are deterministic from call to call.
 *
 * An edge key is (min(a,b) << 32) | max(a,b), as everywhere else.  A library, a header and a signature table of their
 * own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm and ammsb_set are taken by pointer (copied before
 * return) and no ammsb_ctx is needed.  Calls only enqueue work on `stream` (a hipStream_t as void*, NULL = the null
 * stream): no allocation, no synchronisation.  Return values are the codes of ammsb.h.  AMMSB_EINVAL, before anything
 * is launched and before any device pointer is used: a NULL pi / beta / queries / output, eps negative, NaN or >= 1,
 * num_cols == 0 or > 8192, num_rows >= 2^32, a descriptor whose blocks do not cover num_rows, cand_lo + cand_n >
 * num_rows (the wrapped sum included), T == 0 or > 64, a workspace that is NULL, not 16-byte aligned or too small.
 * AMMSB_ERANGE: cand_n > 2^32 - 257 (cut the range in two). */
#ifndef AMMSB_LINKPRED_H_
#define AMMSB_LINKPRED_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_LINKPRED_MAX_TOP 64u
#define AMMSB_LINKPRED_MAX_COLS 8192u
#define AMMSB_LINKPRED_NONE 0xFFFFFFFFu

/* out[i, j] = p(queries[i], cand_lo + j), out: [Q, cand_n] row-major.  The diagonal is computed like any other entry.
 * A query >= num_rows reads nothing; its row of out is -1. */
int ammsb_linkpred_block(const ammsb_rpm* pi, const float* beta, float epsilon, const uint32_t* queries, uint32_t Q,
                         uint64_t cand_lo, uint64_t cand_n, float* out, void* stream);

/* Per query the T best candidates b in [cand_lo, cand_lo + cand_n): b != the query, and the key of (query, b) in
 * neither exclude0 nor exclude1 (each may be NULL).  Order: score descending, equal scores (bit patterns) by id
 * ascending.  ids, scores: [Q, T]; row i belongs to queries[i] (repeats allowed); slots past the eligible candidates
 * hold AMMSB_LINKPRED_NONE and score 0; a query >= num_rows reads nothing and yields empty slots.  Scores are the
 * values ammsb_linkpred_block writes, bit for bit, so lists over disjoint candidate ranges merge on the host by
 * (score bits descending, id ascending) into the list of one call.  No Q x cand_n matrix exists anywhere: workspace
 * holds the partial lists of the blocks (ammsb_linkpred_top_workspace_bytes; 16-byte aligned; contents are scratch). */
int ammsb_linkpred_top(const ammsb_rpm* pi, const float* beta, float epsilon, const uint32_t* queries, uint32_t Q,
                       uint32_t T, const ammsb_set* exclude0, const ammsb_set* exclude1, uint64_t cand_lo,
                       uint64_t cand_n, uint32_t* ids, float* scores, void* workspace, uint64_t workspace_bytes,
                       void* stream);
uint64_t ammsb_linkpred_top_workspace_bytes(uint32_t Q, uint32_t T, uint64_t cand_n, uint64_t K);

/* out[i] = p(a, b) for edges[i] = (a << 32) | b, either order of the ends; a == b is computed as written.  A pair with
 * an end >= num_rows reads nothing and writes -1. */
int ammsb_linkpred_pairs(const ammsb_rpm* pi, const float* beta, float epsilon, const uint64_t* edges, uint64_t n,
                         float* out, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first):
 *   linkpred_block_mfma_{q128,q32}_{v4,v1}, linkpred_top_mfma_{q128,q32}_{v4,v1}   q128: Q > 32, a block owns 128
 *       queries x 64 candidates per tile; q32: Q <= 32 (padded to 32), 32 queries x 256 candidates; v4: 16-byte loads
 *       (K a multiple of 4, 16-byte aligned blocks), v1: any other shape.
 *   linkpred_pairs_{v4,v1} */
const char* ammsb_linkpred_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_linkpred_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_LINKPRED_H_ */
