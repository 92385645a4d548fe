/* libammsb_quality.so: how good is a community?  Per community of a fitted pi the links of an edge list that lie inside
 * it and the links that leave it -- what internal density, conductance and the edge coverage of the cover are made of.
 *
 * Definitions (the contract):
 *   membership   node a is a member of community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a
 *                NaN is never a member.  It is ammsb_readout.h's definition of a community's size, not capped by a top.
 *   edge list    keys (a << 32) | b with the ends in either order; duplicates and a == b are computed as written.  A
 *                key with an end >= num_rows is invalid: it reads nothing and is counted only in `skipped`.
 *   internal[k]  the valid edges with both ends in k.
 *   boundary[k]  the valid edges with exactly one end in k.
 *   uncovered    the valid edges whose ends share no community.
 *   skipped      the invalid edges.
 *   shared[i]    the number of communities that hold both ends of edge i, or -1 for an invalid edge.
 * In numpy: M = pi >= np.float32(thr); both = M[a] & M[b]; one = M[a] ^ M[b]; internal and boundary are the column
 * sums of both and one over the valid edges, shared = both.sum(1).  Only integer adds (block-private u32 counters,
 * flushed with 64-bit atomics): exact and independent of scheduling.
 *
 * Two passes.  ammsb_quality_mask streams pi once and writes one bit per (node, community), ceil(K / 64) 64-bit words
 * per node; ammsb_quality_edges reads two such rows per edge, K / 4 bytes instead of the 8 K bytes of the two rows of
 * pi.  The layout of the mask is private to the library: a function of (num_rows, num_cols) alone, whichever kernel
 * form wrote it, with every bit that stands for no community zero.  A mask is valid for the (pi, thr) it was made from.
 *
 * Derived measures (float64 on the host; mcmc::Learner::WriteCommunityQuality and _quality.py use these formulas), with
 * links = the valid edges and size[k] = the members of k (ammsb_readout.h's sizes):
 *   vol[k]         = 2 internal[k] + boundary[k]                      (the members' degrees in the list, summed)
 *   conductance[k] = boundary[k] / min(vol[k], 2 links - vol[k]),     or -1 where that minimum is 0
 *   density[k]     = internal[k] / (size[k] (size[k] - 1) / 2),       or -1 where size[k] < 2
 *   coverage       = 1 - uncovered / links,                           or -1 with no links
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  The calls only enqueue work on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation.  Return values are the codes of
 * ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used:
 *   ammsb_quality_mask   NULL pi or mask; thr negative, NaN or infinite; num_cols == 0 or > 8192; num_rows >= 2^32; a
 *                        descriptor whose blocks do not cover num_rows (a NULL block among them).
 *   ammsb_quality_edges  NULL mask or edges with n > 0; counts and shared both NULL; num_cols == 0 or > 8192;
 *                        num_rows >= 2^32.  n == 0 is a valid no-op without a device. */
#ifndef AMMSB_QUALITY_H_
#define AMMSB_QUALITY_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_QUALITY_MAX_COLS 8192u

/* Bytes of the mask of a num_rows x num_cols pi: 8 ceil(num_cols / 64) per row.  0 for a shape the library refuses. */
uint64_t ammsb_quality_mask_bytes(uint64_t num_rows, uint32_t num_cols);

/* mask: ammsb_quality_mask_bytes(pi->num_rows, pi->num_cols) bytes, 8-byte aligned; every word of it is written. */
int ammsb_quality_mask(const ammsb_rpm* pi, float thr, uint64_t* mask, void* stream);

/* counts: [2K + 2] zeroed by the caller, or NULL: internal[0..K), boundary[K..2K), uncovered at 2K, skipped at 2K + 1;
 * the call adds to them.  shared: [n] or NULL. */
int ammsb_quality_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges, uint64_t n,
                        uint64_t* counts, int32_t* shared, void* stream);

/* Name of the kernel form the calling thread's last successful launch took ("" before the first):
 *   quality_mask_fast      K a multiple of 256 and 16-byte aligned blocks: a wave per row, 16-byte loads in chunks of
 *                          1024 columns, one ballot per register slot; the next chunk (or the next row's first) is
 *                          requested before this one's words are placed and stored.
 *   quality_mask_generic   every other 1 <= K <= 8192, and misaligned blocks: scalar loads, the same words.
 *   quality_edges_w1       K <= 4096: W = ceil(K / 64) <= 64 words per row; a group of lanes (the smallest power of two
 *                          >= W) owns an edge, 64 / group edges per wave, one word per lane.
 *   quality_edges_w2       K > 4096: a wave owns an edge, two words per lane. */
const char* ammsb_quality_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_quality_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_QUALITY_H_ */
