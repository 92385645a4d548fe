/* libammsb_roles.so: how does a single node sit in the detected cover?  Per node of an adjacency the counts behind the
 * node roles of Guimera and Amaral for an overlapping cover (within-community degree z-score, participation coefficient)
 * and the node's embeddedness, all of them integers and therefore exact.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  The bits are the public node-major mask of the community-links library: W =
 *                   ceil(K / 64) 64-bit words per node, node a at words a W .. a W + W - 1, bit k & 63 of word k >> 6
 *                   standing for community k.  This library clears the bits past K of every word it reads, so a foreign
 *                   mask cannot address outside the outputs.  S_a is a's set of communities and O_a = |S_a|.
 *   adjacency       a CSR over the num_rows nodes: offsets[num_rows + 1] (uint64, non-decreasing, offsets[0] need not be
 *                   0) and targets[] (uint32).  Row a is targets[offsets[a] .. offsets[a + 1]), counted as written:
 *                   duplicates count twice, and b == a is a neighbour like any other.  A target >= num_rows reads nothing
 *                   and is counted in counts[1] (skipped); the others are valid and counted in counts[0].  R_a is the
 *                   multiset of the valid targets of row a.
 *   c[a, k]         = #{b in R_a : k in S_b}: how many of a's neighbours are in k.  Never stored for all (a, k).
 *   per node        (arrays of num_rows, indexed by the absolute node id)
 *     degree   u32  = |R_a|
 *     own      u32  = O_a
 *     embedded u32  = #{b in R_a : S_a and S_b share a community}
 *     reached  u32  = #{k : c[a, k] > 0}
 *     votes    u64  = the sum over k of c[a, k]   (= the sum over b in R_a of O_b)
 *     squares  u64  = the sum over k of c[a, k]^2, modulo 2^64: exact whenever |R_a| <= 2^25 (8192 (2^25)^2 = 2^63); the
 *                     hosts refuse a longer row.
 *   slots           home[num_rows, top] int32, hcount[num_rows, top] uint32, hflags[num_rows] uint32, 1 <= top <= 16.
 *                   Candidates with among = AMMSB_ROLES_ALL: every k with c[a, k] >= max(1, min_count).  With among =
 *                   AMMSB_ROLES_OWN: every k in S_a with c[a, k] >= min_count, where c = 0 is allowed.  Candidates are
 *                   ranked by c descending, equal counts going to the lower k; slot j holds the j-th of them, an empty
 *                   slot holds -1 and 0.  Bit j of hflags[a] is set iff slot j is filled and home[a, j] is in S_a.
 *                   top = 0 with NULL slot arrays skips the selection.
 *   per community   (arrays of K, uint64, zeroed by the caller, added to with 64-bit vector atomics)
 *     ksum[k]       = the sum over the nodes a in k of c[a, k]
 *     ksq[k]        = the sum over the nodes a in k of c[a, k]^2
 *     kmembers[k]   = #{a in k}
 *                   With fewer than 2^32 targets in all none of them wraps, because ksq <= ksum^2.
 *
 * Every output is made of integer adds and compares: exact, the same from run to run, and independent of the kernel
 * form, the grid and how the node range is cut into calls.
 *
 * What the hosts derive in float64 (the same statement in _roles.py and in mcmc::Learner::NodeRolesResult::Derive; no
 * contraction, each uint64 converted once, round to nearest even):
 *   embeddedness[a]  = float64(embedded) / float64(degree); -1 where degree = 0.
 *   participation[a] = 1 - float64(squares) / (float64(votes) float64(votes)): one multiplication, one division, one
 *                      subtraction, in this association; -1 where votes = 0.
 *   z[a, j]          for a filled slot j with k = home[a, j], n = float64(kmembers[k]) where kmembers[k] >= 2:
 *                      mean = float64(ksum[k]) / n;  var = float64(ksq[k]) / n - mean mean;
 *                      z = (float64(hcount[a, j]) - mean) / sqrt(var) where var > 0; 0 elsewhere.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged and no
 * ammsb_ctx is needed.  A call only enqueues a kernel on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h. */
#ifndef AMMSB_ROLES_H_
#define AMMSB_ROLES_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_ROLES_MAX_COLS 8192u
/* the largest num_cols the one-word-per-lane form takes */
#define AMMSB_ROLES_W1_MAX_COLS 4096u
#define AMMSB_ROLES_MAX_TOP 16u
/* the longest row for which squares is exact; the hosts refuse a longer one */
#define AMMSB_ROLES_MAX_ROW 33554432u
/* among */
#define AMMSB_ROLES_ALL 0u
#define AMMSB_ROLES_OWN 1u

/* Handles the nodes first_row .. first_row + n_rows - 1: writes their entries of the per-node arrays (and of the slot
 * arrays where top > 0), and adds to ksum, ksq, kmembers [num_cols] and to counts[2] = (valid, skipped), which the caller
 * zeroes before the first call.  Calls over disjoint ranges fill one result.  n_rows == 0 is a valid no-op that needs no
 * device.
 * AMMSB_EINVAL, before anything is launched and before any device pointer is used:
 *   mask, offsets, targets            NULL, or mask / offsets not 8-byte aligned, targets not 4-byte aligned
 *   num_cols                          0 or > 8192
 *   num_rows                          >= 2^32
 *   first_row, n_rows                 first_row + n_rows > num_rows
 *   among                             neither AMMSB_ROLES_ALL nor AMMSB_ROLES_OWN
 *   top                               > 16; > 0 with a NULL home, hcount or hflags
 *   degree, own, embedded, reached    NULL or not 4-byte aligned
 *   votes, squares                    NULL or not 8-byte aligned
 *   home, hcount, hflags              (where not NULL) not 4-byte aligned
 *   ksum, ksq, kmembers, counts       NULL or not 8-byte aligned */
int ammsb_roles_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* offsets,
                      const uint32_t* targets, uint64_t first_row, uint64_t n_rows, uint32_t among, uint32_t top,
                      uint32_t min_count, uint32_t* degree, uint32_t* own, uint32_t* embedded, uint32_t* reached,
                      uint64_t* votes, uint64_t* squares, int32_t* home, uint32_t* hcount, uint32_t* hflags, uint64_t* ksum,
                      uint64_t* ksq, uint64_t* kmembers, uint64_t* counts, void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   roles_nodes_w1    K <= 4096.  A wave owns a node; lane l holds word l of a row of bits and alone owns the 64 counters
 *                     of that word in the wave's private uint32 h[64 W] in LDS (counter (w, t) at t W + w, so the lanes of
 *                     a request fall on different banks): no LDS atomics, no conflicts between lanes.  Per neighbour the
 *                     W words of its row in one coalesced request, four neighbours in flight; each lane walks the set bits
 *                     of its word and increments; one ballot of word_a & word_b gives embedded, population counts give
 *                     votes.  Each lane ORs the words it has seen and at the row's end walks only those bits: squares,
 *                     reached, ksum / ksq for k in S_a, `top` rounds of a wave-wide arg-max of (c, -k) taken after the
 *                     previous winner, and the counters it touched set back to zero.  Rows go to the waves of a persistent
 *                     grid in turn.
 *   roles_nodes_w2    K > 4096: lane l holds words l and l + 64; otherwise the same, two waves per block. */
const char* ammsb_roles_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_roles_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_ROLES_H_ */
