/* libammsb_modularity.so: is the detected cover better than chance?  The overlapping modularity EQ of Shen et al. (2009)
 * of the cover against an edge list, per community and in all, from sums that are integers and therefore exact.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  The bits are the public node-major mask of the community-links library: W =
 *                   ceil(K / 64) 64-bit words per node, node a at words a W .. a W + W - 1, bit k & 63 of word k >> 6
 *                   standing for community k.  Every bit that stands for no community is zero; this library clears the
 *                   bits past K of every word it reads anyway, so a foreign mask cannot address outside the outputs.
 *   O_a             the population count of node a's row of bits: the communities a belongs to.
 *   edge list       keys (a << 32) | b with the ends in either order; duplicates and a == b are computed as written.  A
 *                   key with an end >= num_rows reads nothing and is counted in `skipped` only; the others are valid.
 *                   m is the number of valid keys.
 *   deg[a]          uint32: the number of times a occurs as an end of a valid key.  A key a == a adds 2.
 *   With F = 2^62:
 *   IN[k]           = the sum over the valid keys with both ends in k of floor(F / (O_a O_b))          (unsigned 128-bit)
 *   SV[k]           = the sum over the nodes a in k of deg[a] floor(F / O_a)     (unsigned 128-bit; a 94-bit product, exact)
 *   in_k, s_k       = float64(IN[k]) 2^-62 and float64(SV[k]) 2^-62: one round-to-nearest-even conversion of the integer,
 *                   then an exact scaling.
 *   q_k             = (2 in_k - s_k s_k / (2m)) / (2m) in float64, in this association, no contraction;
 *   q               = the sum of q_k in index order.  q_k and q are -1 when m = 0.
 *                   For a partition (O_a = 1 everywhere) IN[k] = internal[k] 2^62 and SV[k] = (2 internal + boundary)[k]
 *                   2^62 of ammsb_quality.h, and q is Newman's modularity.
 *
 * A 128-bit accumulator is two uint64, the low word at [2k] and the high word at [2k + 1].  It is combined only with
 * 64-bit unsigned vector atomics: the term's low part is added to the low word, the wrap is read off the returned old
 * value, and the carry plus the term's high part is added to the high word.  Addition modulo 2^128 does not depend on the
 * order of arrival, so every integer output is exact, the same from run to run, and independent of the kernel form, the
 * grid and how the edge list was cut into calls.  No float touches an accumulator.
 *
 * Rounding.  Relative to the unquantised EQ (terms 1 / (O_a O_b) and deg[a] / O_a as rationals) a term's truncation is
 * below P 2^-62 of the term, P = O_a O_b <= 2^26 at the library's limit of 8192 communities: at most 2^-36 of a term, and
 * far below a float64 ulp of it while P <= 512.  The host's float64 arithmetic on in_k and s_k (four operations per q_k)
 * is the only other rounding.
 *
 * The cost of the edge pass is one 128-bit add (one or two 64-bit atomics) per community that holds both ends of an
 * edge, and two 32-bit atomics per edge; that of the node pass one 128-bit add per membership of a node with a link.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged and no
 * ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h.  AMMSB_EINVAL, before anything is launched and
 * before any device pointer is used, is listed per call. */
#ifndef AMMSB_MODULARITY_H_
#define AMMSB_MODULARITY_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_MODULARITY_MAX_COLS 8192u
/* the largest num_cols the one-word-per-lane forms take */
#define AMMSB_MODULARITY_W1_MAX_COLS 4096u
/* F = 2^AMMSB_MODULARITY_FRAC_BITS */
#define AMMSB_MODULARITY_FRAC_BITS 62u
/* an edge call takes fewer keys than this */
#define AMMSB_MODULARITY_MAX_EDGES 2147483648ull

/* Adds the n edges to degree[num_rows] (uint32), to internal[2 num_cols] (IN, 128-bit as two uint64 each) and to
 * counts[2] = (valid, skipped); the caller zeroes all three before the first call, and keeps the total of the calls
 * below 2^31 keys so that no degree wraps.  mask: the community-links library's mask of a num_rows x num_cols pi.  n == 0
 * is a valid no-op that needs no device.
 * EINVAL: a NULL mask or edges with n > 0; a NULL degree, internal or counts; num_cols == 0 or > 8192; num_rows >= 2^32;
 * n >= 2^31; a degree that is not 4-byte aligned, an internal or counts that is not 8-byte aligned. */
int ammsb_modularity_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges, uint64_t n,
                           uint32_t* degree, uint64_t* internal, uint64_t* counts, void* stream);

/* After the last edge call: adds deg[a] floor(F / O_a) to volume[2 num_cols] (SV, 128-bit as two uint64 each) for every
 * community of every node with deg[a] > 0; the caller zeroes volume.  num_rows == 0 launches nothing.
 * EINVAL: a NULL mask or degree with num_rows > 0; a NULL volume; num_cols == 0 or > 8192; num_rows >= 2^32; a degree
 * that is not 4-byte aligned, a volume that is not 8-byte aligned. */
int ammsb_modularity_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint32_t* degree,
                           uint64_t* volume, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   modularity_edges_w1    K <= 4096.  A group of lanes, the smallest power of two >= W, owns an edge with one word of
 *                          each row per lane, over a persistent grid; the next edge's words are requested before this
 *                          one's atomics.  The group sums the population counts of both rows by shuffles, a lane with a
 *                          shared community divides F by O_a O_b once and adds the quotient to IN[k] for every set bit
 *                          of the AND of its two words; the group's first lane adds 1 to both ends' degrees.
 *   modularity_edges_w2    K > 4096: a wave owns an edge with two words of each row per lane; otherwise the same.
 *   modularity_nodes_w1    K <= 4096.  A group of lanes owns a node with deg > 0: the population count of its row, one
 *                          division, the 32 x 64 -> 96-bit product, one 128-bit add per set bit.
 *   modularity_nodes_w2    K > 4096: a wave per node, two words per lane. */
const char* ammsb_modularity_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_modularity_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_MODULARITY_H_ */
