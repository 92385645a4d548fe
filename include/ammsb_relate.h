/* libammsb_relate.so: how do the K detected communities relate to each other?  The K x K matrix of the nodes every two
 * communities share, and per community the partners it overlaps most -- which communities are the same set of nodes,
 * which lie inside which, which overlap substantially.
 *
 * Definitions (the contract):
 *   membership     node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is never
 *                  a member.  It is ammsb_readout.h's and ammsb_quality.h's definition.
 *   overlap[k, l]  = |{a < N : a in k and a in l}|, a uint32.  The matrix is symmetric and overlap[k, k] = d_k, the size
 *                  of k (ammsb_readout.h's sizes).
 *                  In numpy: M = pi >= np.float32(thr); overlap = M.T.astype(np.float64) @ M.astype(np.float64), which
 *                  is exact: every count is below 2^32.
 *   partners of k  the `top` communities l != k with overlap[k, l] >= max(1, min_overlap), ranked by one measure of
 *                  o = overlap[k, l]:
 *                    AMMSB_RELATE_OVERLAP     o
 *                    AMMSB_RELATE_JACCARD     o / (d_k + d_l - o)
 *                    AMMSB_RELATE_CONTAINED   o / d_l: the share of l that lies inside k, which finds k's sub-communities
 *                  largest first.  Two rationals are compared by cross-multiplication in 128 bits (the Jaccard products
 *                  reach 2^65), so no value is rounded; equal values go to the lower l.  A slot past the last partner
 *                  holds partner -1 and shared 0.
 * Only integer adds over binary32 compares and integer compares: every output is exact, the same from run to run, and
 * does not depend on scheduling or on how the nodes were cut into slabs.
 *
 * Bit rows (public: a caller may make or read them).  ammsb_relate_bits turns rows [row0, row0 + rows) of pi into
 * community-major bits: for each of the K communities W = ceil(rows / 64) 64-bit words, community k at words k W ..
 * k W + W - 1.  Bit (a - row0) & 63 of word (a - row0) >> 6 of community k is set iff node a is a member of k.  Every
 * word is written and every bit that stands for no node is zero.
 *
 * Three passes.  ammsb_relate_bits streams a slab of pi once; ammsb_relate_pairs adds the slab's AND + population counts
 * into overlap[K, K]; ammsb_relate_top selects from the finished matrix.  A slab holds K rows / 8 bytes, so the nodes of a
 * large pi are cut into slabs that fit a byte budget: overlap is the sum over the slabs.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation.  Return values are the codes of
 * ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used, is listed per call. */
#ifndef AMMSB_RELATE_H_
#define AMMSB_RELATE_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_RELATE_MAX_COLS 8192u
#define AMMSB_RELATE_MAX_TOP 64u
#define AMMSB_RELATE_TILE 128u
/* the measures of ammsb_relate_top */
#define AMMSB_RELATE_OVERLAP 0u
#define AMMSB_RELATE_JACCARD 1u
#define AMMSB_RELATE_CONTAINED 2u

/* Bytes of the bit rows of `rows` nodes and num_cols communities: 8 num_cols ceil(rows / 64).  0 for a shape the library
 * refuses (num_cols == 0 or > 8192, rows >= 2^32) and for rows == 0. */
uint64_t ammsb_relate_bits_bytes(uint64_t rows, uint32_t num_cols);

/* bits: ammsb_relate_bits_bytes(rows, pi->num_cols) bytes, 8-byte aligned, from rows [row0, row0 + rows) of pi.
 * rows == 0 launches nothing.
 * EINVAL: a NULL pi or bits; thr negative, NaN or infinite; num_cols == 0 or > 8192; num_rows >= 2^32; row0 + rows past
 * num_rows; row0 not a multiple of 64; a descriptor whose blocks do not cover num_rows (a NULL block among them). */
int ammsb_relate_bits(const ammsb_rpm* pi, float thr, uint64_t row0, uint64_t rows, uint64_t* bits, void* stream);

/* Adds the counts of one slab to overlap[num_cols, num_cols] (zeroed by the caller before the first slab): both halves
 * of the symmetric matrix and the diagonal.  bits as ammsb_relate_bits writes them for `rows` nodes.  rows == 0 launches
 * nothing.
 * EINVAL: a NULL bits or overlap; num_cols == 0 or > 8192; rows >= 2^32. */
int ammsb_relate_pairs(const uint64_t* bits, uint32_t num_cols, uint64_t rows, uint32_t* overlap, void* stream);

/* partner[num_cols, top] and shared[num_cols, top] from the finished overlap[num_cols, num_cols].
 * EINVAL: a NULL overlap, partner or shared; num_cols == 0 or > 8192; a measure that is none of the three; top == 0 or
 * > 64. */
int ammsb_relate_top(const uint32_t* overlap, uint32_t num_cols, uint32_t measure, uint32_t top, uint32_t min_overlap,
                     int32_t* partner, uint32_t* shared, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   relate_bits_fast      K a multiple of 256 and 16-byte aligned blocks.  A block of 256 lanes owns 256 consecutive
 *                         rows x 256 columns, a wave 64 of the rows: per row one 16-byte load per lane and four ballots,
 *                         which lane (row & 63) keeps; then the four 64 x 64 bit blocks are transposed by 64 ballots of
 *                         one bit of the kept words each, and every lane stores four whole words, one per community.
 *   relate_bits_generic   every other 1 <= K <= 8192, and misaligned blocks: 64 columns per wave, scalar loads, one
 *                         ballot per row; the same words.
 *   relate_pairs          a persistent grid over (tile, depth slice): the upper triangle of AMMSB_RELATE_TILE x
 *                         AMMSB_RELATE_TILE tiles of community pairs times slices of the node words, so that K = 1024
 *                         (36 tiles) still fills the chip.  A block of 256 lanes streams 16-word chunks (32-bit words)
 *                         of both community sets through LDS, every lane keeps an 8 x 8 micro-tile of counters in
 *                         registers (AND + population count), and the partial tile is added with 32-bit vector atomics:
 *                         to (k, l) and (l, k) off the diagonal, to each cell once on it.
 *   relate_top            a wave per community: `top` rounds over its row of overlap, d_l from the diagonal (staged in
 *                         LDS), each round the best candidate that comes after the previous winner. */
const char* ammsb_relate_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_relate_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_RELATE_H_ */
