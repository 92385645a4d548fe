/* libammsb_connect.so: how are the K detected communities linked to each other?  The K x K matrix of the links of an
 * edge list that run between every two communities -- the community (quotient) graph -- and per community the partners
 * it is linked to most, by count or by density.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  It is ammsb_quality.h's definition.  M[a, k] is 1 for a member and 0 otherwise.
 *   edge list       keys (a << 32) | b with the ends in either order; duplicates and a == b are computed as written.  A
 *                   key with an end >= num_rows reads nothing and is counted in `skipped` only; the others are valid.
 *   directed[k, l]  = the sum over the valid edges of M[a, k] M[b, l], with a the high half of the key as written.  uint64.
 *   links[k, l]     = directed[k, l] + directed[l, k], uint64.  The matrix is symmetric, and links[k, k] = 2 internal[k]
 *                   of ammsb_quality_edges over the same inputs.
 *                   In numpy: C = M[a].T.astype(np.float64) @ M[b].astype(np.float64); links = C + C.T, which is exact
 *                   below 2^53.
 *   pairs[k, l]     = d_k d_l - overlap[k, l]: the ordered node pairs (a in k, b in l, a != b).  overlap is
 *                   the relate library's matrix (the nodes in both k and l) and d its diagonal (the community sizes).
 *   density[k, l]   = links[k, l] / pairs[k, l].  On the diagonal, for a simple edge list (every link once, no loop), it
 *                   is 2 internal[k] / (d_k (d_k - 1)): the density of ammsb_quality.h.
 *   partners of k   the `top` <= 64 communities l != k with links[k, l] >= max(1, min_links), ranked by one measure of
 *                   w = links[k, l]:
 *                     AMMSB_CONNECT_LINKS     w
 *                     AMMSB_CONNECT_DENSITY   w / pairs[k, l]; a pair with pairs[k, l] == 0 is no partner
 *                   Two rationals are compared by cross-multiplication in unsigned 128 bits (w and pairs are each below
 *                   2^64), so no value is rounded; equal values go to the lower l.  A slot past the last partner holds
 *                   partner -1, links 0 and shared 0.
 * Only integer adds over binary32 compares and integer compares: every output is exact and the same from run to run, and
 * none depends on the kernel form, the grid or how the edge list was cut into calls.
 *
 * The mask (public: a caller may make or read it).  ammsb_connect_mask turns pi into node-major bits: for each of the
 * num_rows nodes W = ceil(K / 64) 64-bit words, node a at words a W .. a W + W - 1.  Bit k & 63 of word k >> 6 stands for
 * community k.  Every word is written and every bit that stands for no community is zero.  (ammsb_quality.h's mask has a
 * layout private to its library, so this library writes its own.)
 *
 * The cost of the edge pass is the sum over the valid edges of |S_a| |S_b| cell updates, S_a being the communities of a:
 * an edge whose ends hold few communities each is cheap whatever K is, and thr = 0 at a large K makes every edge K^2
 * updates.  That is the caller's to avoid; the library does not refuse it.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation.  Return values are the codes of
 * ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used, is listed per call. */
#ifndef AMMSB_CONNECT_H_
#define AMMSB_CONNECT_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_CONNECT_MAX_COLS 8192u
#define AMMSB_CONNECT_MAX_TOP 64u
/* the largest num_cols the runs form of ammsb_connect_edges takes */
#define AMMSB_CONNECT_RUNS_MAX_COLS 4096u
/* the measures of ammsb_connect_top */
#define AMMSB_CONNECT_LINKS 0u
#define AMMSB_CONNECT_DENSITY 1u

/* Bytes of the mask of a num_rows x num_cols pi: 8 ceil(num_cols / 64) per row.  0 for a shape the library refuses
 * (num_cols == 0 or > 8192, num_rows >= 2^32) and for num_rows == 0. */
uint64_t ammsb_connect_mask_bytes(uint64_t num_rows, uint32_t num_cols);

/* mask: ammsb_connect_mask_bytes(pi->num_rows, pi->num_cols) bytes, 8-byte aligned.  num_rows == 0 launches nothing.
 * EINVAL: a NULL pi or mask; thr negative, NaN or infinite; num_cols == 0 or > 8192; num_rows >= 2^32; a descriptor whose
 * blocks do not cover num_rows (a NULL block among them); a mask that is not 8-byte aligned. */
int ammsb_connect_mask(const ammsb_rpm* pi, float thr, uint64_t* mask, void* stream);

/* Adds the n edges to directed[num_cols, num_cols] and to counts[2] = (valid, skipped); the caller zeroes both before
 * the first call.  mask as ammsb_connect_mask writes it for a num_rows x num_cols pi.  n == 0 is a valid no-op that needs
 * no device.
 * EINVAL: a NULL mask or edges with n > 0; a NULL directed or counts; num_cols == 0 or > 8192; num_rows >= 2^32; a value
 * of AMMSB_CONNECT_FORM that is neither d nor r (see ammsb_connect_last_kernel_name). */
int ammsb_connect_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges, uint64_t n,
                        uint64_t* directed, uint64_t* counts, void* stream);

/* links = directed + directed^T, both [num_cols, num_cols]; they must not be the same buffer.
 * EINVAL: a NULL directed or links; links == directed; num_cols == 0 or > 8192. */
int ammsb_connect_finish(const uint64_t* directed, uint32_t num_cols, uint64_t* links, void* stream);

/* partner[num_cols, top], plinks[num_cols, top] (links[k, partner]) and pshared[num_cols, top] (overlap[k, partner]) from
 * the finished links[num_cols, num_cols] and the relate library's overlap[num_cols, num_cols].
 * EINVAL: a NULL links, overlap, partner, plinks or pshared; num_cols == 0 or > 8192; a measure that is neither of the
 * two; top == 0 or > 64. */
int ammsb_connect_top(const uint64_t* links, const uint32_t* overlap, uint32_t num_cols, uint32_t measure, uint32_t top,
                      uint64_t min_links, int32_t* partner, uint64_t* plinks, uint32_t* pshared, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   connect_mask_fast      K a multiple of 256 and 16-byte aligned blocks: a wave per row, 16-byte loads in chunks of
 *                          1024 columns and four ballots per load; a lane then puts the 16-bit slices of four ballots
 *                          together into the word of 64 consecutive communities it stores.
 *   connect_mask_generic   every other 1 <= K <= 8192, and misaligned blocks: scalar loads, one ballot per 64 columns;
 *                          the same words.
 *   connect_edges_direct   a wave per edge over a persistent grid.  The wave loads both bit rows (one or two words per
 *                          lane), compacts b's set bits into a wave-private list in LDS by prefix population counts,
 *                          walks a's set bits wave-uniformly and, for each, has its lanes stride over the list with one
 *                          64-bit vector atomic per cell of directed.  Every shape; the default above K = 4096.
 *   connect_edges_runs     K <= 4096.  A wave owns a chunk of consecutive edges; over a run of equal high ends a it
 *                          counts b's bits into wave-private u32 counters h[K] in LDS, and at the run's end adds h[l] to
 *                          directed[k, l] for every k of a and every l with h[l] > 0.  A sorted list of links of an
 *                          assortative graph flushes a handful of cells per run.  Any segmentation is correct: an
 *                          unsorted list has runs of length 1.  The default for K <= 4096: the faster of the two on a
 *                          sorted list of links.
 *                          AMMSB_CONNECT_FORM=d or =r in the environment (read at every call) takes that form wherever
 *                          the shape has it: above K = 4096 there is only connect_edges_direct.
 *   connect_finish         one lane per cell: directed[k, l] + directed[l, k].
 *   connect_top            a wave per community: `top` rounds over its row of links, d from the diagonal of overlap
 *                          (staged in LDS), each round the best candidate that comes after the previous winner. */
const char* ammsb_connect_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_connect_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_CONNECT_H_ */
