/* libammsb_triangles.so: do the detected communities hold triangles?  Per node of a simple adjacency its triangles, those
 * that lie inside a community all three corners share, and per community the triangles inside it and the members that
 * take part in one: the integers behind the triangle participation ratio of Yang and Leskovec, the internal clustering
 * coefficient of a community and the strong-ties embeddedness of a node, all of them exact.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  The bits are the public node-major mask of the community-links library: W =
 *                   ceil(K / 64) 64-bit words per node, node a at words a W .. a W + W - 1, bit k & 63 of word k >> 6
 *                   standing for community k.  This library clears the bits past K of every word it reads, so a foreign
 *                   mask cannot address outside the outputs.  S_a is a's set of communities.
 *   adjacency       a simple CSR over the num_rows nodes: offsets[num_rows + 1] (uint64, non-decreasing, offsets[0] need
 *                   not be 0) and targets[] (uint32).  Row a is targets[offsets[a] .. offsets[a + 1]) and
 *                     is strictly ascending,
 *                     holds no b == a,
 *                     is symmetric: b is in row a iff a is in row b,
 *                     holds targets < num_rows only.
 *                   The hosts build it and verify it; this entry point cannot.  For any other input the counts are
 *                   unspecified, but no access outside mask, targets and the outputs results: every search stays inside
 *                   its row's bounds, and a target >= num_rows reads nothing and is counted in counts[1].
 *   triangles       a triangle at a is an unordered pair {b, c} of neighbours of a with b < c and c a neighbour of b.  Its
 *                   communities are m = S_a & S_b & S_c.
 *   per node        (arrays of num_rows, uint32, indexed by the absolute node id)
 *     tri[a]        = triangles at a
 *     tri_in[a]     = triangles at a with m not empty
 *     tri_comms[a]  = #{k : tk[a, k] > 0}, where tk[a, k] = triangles at a with k in m.  tk is never stored for all (a, k).
 *   per community   (arrays of K, uint64, zeroed by the caller, added to with 64-bit vector atomics)
 *     ktri3[k]      = the sum over a of tk[a, k]: three times the number of triangles inside k (the hosts assert that 3
 *                     divides it)
 *     kpart[k]      = #{a : tk[a, k] > 0}
 *   counts[2]       counts[0] = the sum of tri[a] over the rows handled; counts[1] = targets >= num_rows met.
 *   limits          K <= 8192; num_rows < 2^32; rows of at most AMMSB_TRIANGLES_MAX_ROW = 65535 targets, so that tri <=
 *                   C(65535, 2) < 2^31 and no uint32 counter wraps.  The hosts refuse a longer row.
 *
 * Every output is made of integer adds and compares: exact, the same from run to run, and independent of the kernel
 * form, the grid and how the node range is cut into calls.
 *
 * What the hosts derive in float64 (the same statement in _triangles.py and in mcmc::Learner::TrianglesResult::Derive; no
 * contraction, each integer converted once, round to nearest even; a value is -1 where its denominator is 0).  kmembers
 * and wedges come from one run of the node-roles library without a selection over the same simple CSR: with its ksum and
 * ksq, wedges[k] = (ksq - ksum) / 2 = the sum over the members a of k of C(c[a, k], 2), an exact integer.
 *   tpr[k]              = float64(kpart) / float64(kmembers)
 *   triangles[k]        = ktri3 / 3 (an integer)
 *   clustering[k]       = float64(ktri3) / float64(wedges)
 *   local_clustering[a] = float64(tri) / (float64(deg) (float64(deg) - 1) / 2); -1 where deg < 2
 *   inside[a]           = float64(tri_in) / float64(tri)
 *   total               = (the sum of tri) / 3;  transitivity = float64(the sum of tri) / float64(the sum of C(deg, 2));
 *   avg_clustering      = the sum of local_clustering over the nodes with deg >= 2, added in node order, over their number
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged and no
 * ammsb_ctx is needed.  A call only enqueues a kernel on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h. */
#ifndef AMMSB_TRIANGLES_H_
#define AMMSB_TRIANGLES_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_TRIANGLES_MAX_COLS 8192u
/* the largest num_cols the one-word-per-lane form takes */
#define AMMSB_TRIANGLES_W1_MAX_COLS 4096u
/* the longest row for which the uint32 counters cannot wrap; the hosts refuse a longer one */
#define AMMSB_TRIANGLES_MAX_ROW 65535u
/* ROW_LDS: a row of at most this many targets is copied into its wave's LDS and searched there; a longer one is searched
 * in global memory by the same code.  The budget, per wave: the counters h[64 W] take 16 KiB at K = 4096 and 32 KiB at
 * K = 8192, the row 4 KiB.  A block of the one-word form has two waves (40 KiB at most), one of the two-word form has one
 * (36 KiB): both stay below the 64 KiB a block may ask for without an attribute, and four blocks of either fit the 160 KiB
 * of a CU.  At K <= 1024 a wave needs at most 8 KiB and the 32 waves a CU can hold fit.  1024 targets cover every row of
 * the graphs the project fits but their few hubs. */
#define AMMSB_TRIANGLES_ROW_LDS 1024u

/* Handles the nodes first_row .. first_row + n_rows - 1: writes their entries of tri, tri_in and tri_comms, and adds to
 * ktri3, kpart [num_cols] and to counts[2], which the caller zeroes before the first call.  Calls over disjoint ranges
 * fill one result.  n_rows == 0 is a valid no-op that needs no device.
 * AMMSB_EINVAL, before anything is launched and before any device pointer is used:
 *   mask, offsets, targets            NULL, or mask / offsets not 8-byte aligned, targets not 4-byte aligned
 *   num_cols                          0 or > 8192
 *   num_rows                          >= 2^32
 *   first_row, n_rows                 first_row + n_rows > num_rows
 *   tri, tri_in, tri_comms            NULL or not 4-byte aligned
 *   ktri3, kpart, counts              NULL or not 8-byte aligned */
int ammsb_triangles_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* offsets,
                          const uint32_t* targets, uint64_t first_row, uint64_t n_rows, uint32_t* tri, uint32_t* tri_in,
                          uint32_t* tri_comms, uint64_t* ktri3, uint64_t* kpart, uint64_t* counts, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   triangles_nodes_w1  K <= 4096.  A wave owns a node a; lane l holds word l of a row of bits.  The row of a is copied
 *                       into the wave's LDS where it has at most ROW_LDS targets.  For each neighbour b the triangles
 *                       with c > b: the shorter of (the row of a after b, the row of b above b) gives the candidates, 64
 *                       at a time, one per lane, each binary-searched in the other list inside that list's bounds; a
 *                       ballot collects the hits.  Where S_a & S_b is empty (one ballot) only the population count of
 *                       the hits is added to tri.  Otherwise the rows of bits of four hits are requested together, m =
 *                       S_a & S_b & S_c, a ballot gives tri_in, and each lane walks the set bits of its word of m and
 *                       increments counters it alone owns in the wave's private uint32 h[64 W] in LDS (counter (w, t) at
 *                       t W + w, so the lanes of a request fall on different banks): no LDS atomics.  Each lane ORs the
 *                       words it has touched and at the row's end walks only those bits: ktri3 and kpart by atomics,
 *                       the population count into tri_comms, and the counters set back to zero.  Rows go to the waves of
 *                       a persistent grid in turn; a hub row is walked by its one wave.  Two waves per block.
 *   triangles_nodes_w2  K > 4096: lane l holds words l and l + 64; otherwise the same, one wave per block. */
const char* ammsb_triangles_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_triangles_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_TRIANGLES_H_ */
