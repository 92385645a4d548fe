/* libammsb_components.so: is each detected community one piece?  The connected components of every community of the cover
 * inside the graph of an edge list, by a lock-free union-find on the device: per membership the component it lies in and
 * that component's size, per community the number of components, the largest one and the singletons, per node the
 * memberships outside their community's largest component.  All of them exact integers.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  The bits are the public node-major mask of the community-links library: W =
 *                   ceil(K / 64) 64-bit words per node, node a at words a W .. a W + W - 1, bit k & 63 of word k >> 6
 *                   standing for community k.  This library clears the bits past K of every word it reads.  S_a is a's
 *                   set of communities and own[a] = |S_a|.
 *   slots           the memberships are numbered node by node, the communities of a node ascending: base[a] is the
 *                   exclusive prefix sum of own (uint64, base[N] = M, the hosts make it), and the slot of (a, k in S_a) is
 *                   base[a] + #{l in S_a : l < k}.  M < 2^32; the hosts refuse a larger one and name the threshold.
 *   edge list       keys (a << 32) | b, the ends in either order.  A key with an end >= N is counted in skipped only.
 *                   Duplicates and a == a are valid and change nothing but the counts.  links = the valid keys; shared =
 *                   the sum over the valid keys of |S_a & S_b|, the unions attempted.
 *   components      two members a, b of k are connected in k iff a path of valid keys joins them whose nodes are all
 *                   members of k.  A component is an equivalence class; its root is its smallest node id, its size the
 *                   number of its members.
 *   per slot        (arrays of M, in slot order, uint32)
 *     root[s]       = the root of the component the slot's node is in, in the slot's community
 *     size[s]       = the size of that component
 *   per community   (arrays of K; zeroed by the caller where they are added to)
 *     members       uint64  number of members
 *     components    uint64  number of components
 *     singletons    uint64  components of size 1
 *     largest       uint32  size of the largest component
 *     largest_root  int32   its root; among equal sizes the smallest root; -1 for an empty community
 *   per node        stray[a] (uint32) = #{k in S_a : root of (a, k) != largest_root[k]}: what a trim would drop
 *   counts[4]       valid, skipped, shared, give-ups (below); uint64, zeroed by the caller, added to
 *   limits          K <= 8192; N < 2^32; M < 2^32; fewer than 2^31 keys per call
 *
 * Every output is an integer that the partition alone determines: exact, the same from run to run, and independent of
 * the kernel form, the grid, the order of the keys and how the list is cut into calls.
 *
 * The union-find.  parent[M] (uint32) with parent[x] <= x always: the smaller index wins, so no cycle can form, the root
 * of a set is its smallest slot, and since slots are numbered node by node that is the slot of its smallest node.  find
 * halves paths; unite hooks the larger root under the smaller by a 32-bit compare-and-swap.  No lane waits for another.
 *   stale reads     the L2s of the eight XCDs are not coherent with each other, so a load of parent[] may return an older
 *                   value.  An older value is still a smaller member of the same set, so find stays correct; and a retry
 *                   after a failed hook continues from the value the atomic returned, never from a fresh load, which
 *                   could repeat the stale value for ever.  Loads and halving stores of parent are relaxed agent-scope
 *                   atomics, not plain accesses.
 *   bounded loops   a find or a hook that takes more than AMMSB_COMPONENTS_MAX_STEPS = 2^20 steps stops, adds 1 to
 *                   counts[3] and leaves that union undone (in finish: takes the slot as its own root).  The hosts raise
 *                   on counts[3] != 0.  Every failed hook moves to a strictly smaller index, so this is a fuse, not a
 *                   path that correct inputs take.
 *
 * What the hosts derive in float64 (the same statement in _components.py and in
 * mcmc::Learner::ComponentsResult::Derive; each integer converted once; -1 where members is 0):
 *   giant[k]         = float64(largest) / float64(members)
 *   fragmentation[k] = 1 - giant[k]
 *   connected        = #{k : components == 1} / #{k : members > 0}; -1 over nothing
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged and no
 * ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h.  Every call refuses, with AMMSB_EINVAL and
 * before anything is launched or any device pointer is used: num_cols 0 or > 8192, num_rows >= 2^32, num_slots >= 2^32, a
 * NULL pointer it would use, and a pointer that is not aligned to its element (mask, base, edges, counts and the uint64
 * arrays 8 bytes, the uint32 / int32 arrays 4, slot_comm 2). */
#ifndef AMMSB_COMPONENTS_H_
#define AMMSB_COMPONENTS_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_COMPONENTS_MAX_COLS 8192u
/* the largest num_cols the one-word-per-lane forms take */
#define AMMSB_COMPONENTS_W1_MAX_COLS 4096u
#define AMMSB_COMPONENTS_MAX_EDGES (1ull << 31)
#define AMMSB_COMPONENTS_MAX_SLOTS (1ull << 32)
/* the fuse of every find and hook */
#define AMMSB_COMPONENTS_MAX_STEPS (1u << 20)

/* own[a] = the population count of row a, for every a < num_rows.  num_rows == 0 is a valid no-op. */
int ammsb_components_own(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, uint32_t* own, void* stream);

/* For the nodes first_row .. first_row + n_rows - 1 and each of their slots s: slot_node[s] = the node, slot_comm[s] = the
 * community, parent[s] = s.  base[num_rows + 1] is the exclusive prefix sum of own; a slot >= num_slots is not written.
 * Also EINVAL: first_row + n_rows > num_rows.  n_rows == 0 is a valid no-op. */
int ammsb_components_slots(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                           uint64_t num_slots, uint64_t first_row, uint64_t n_rows, uint32_t* slot_node,
                           uint16_t* slot_comm, uint32_t* parent, void* stream);

/* Unites, for every valid key and every community both ends share, the two slots in parent[num_slots]; adds to counts[4].
 * May be called any number of times on pieces of the list, after slots has covered every node.  Also EINVAL: n >= 2^31.
 * n == 0 is a valid no-op. */
int ammsb_components_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                           uint64_t num_slots, const uint64_t* edges, uint64_t n, uint32_t* parent, uint64_t* counts,
                           void* stream);

/* After the last edges call, in launches of their own (the kernel boundary makes the unions visible):
 *   components_finish_roots   root[s] = find(s) as a slot, size[s] = 0
 *   components_finish_sizes   a 32-bit atomic add of 1 at size[root slot]
 *   components_finish_slots   at a root slot: members += size, components += 1, singletons += (size == 1) and one 64-bit
 *                             atomic max of (size << 32) | (0xFFFFFFFF - root node) into best[k]; at every slot root[s] =
 *                             slot_node[root slot] and size[s] = the root slot's
 *   components_finish_best    largest[k], largest_root[k] out of best[k]
 *   components_finish_stray   a group of lanes per node compares the roots of its slots with largest_root
 * members, components, singletons, best [num_cols] and counts[4] are zeroed by the caller; root, size [num_slots], largest,
 * largest_root [num_cols] and stray [num_rows] are written whole.  num_slots == 0 and num_rows == 0 are valid. */
int ammsb_components_finish(uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                            const uint32_t* slot_node, const uint16_t* slot_comm, uint32_t* parent, uint32_t* root,
                            uint32_t* size, uint64_t* members, uint64_t* components, uint64_t* singletons, uint64_t* best,
                            uint32_t* largest, int32_t* largest_root, uint32_t* stray, uint64_t* counts, void* stream);

/* Name of the kernel form the calling thread's last successful call launched last ("" before the first):
 *   components_own_w1 / _w2    a group of lanes (the smallest power of two >= W; above K = 4096 a wave with two words per
 *                              lane) owns a node and sums the population counts of its words by shuffles
 *   components_slots_w1 / _w2  the same groups; an exclusive prefix sum by shuffles gives every lane the slot of its word's
 *                              first bit, and the lane walks its bits
 *   components_edges_w1 / _w2  a group owns an edge over a persistent grid and requests the next edge's words before this
 *                              edge's unions; the exclusive prefix sums of the population counts of both rows by shuffles;
 *                              a lane walks the set bits of Sa_word & Sb_word and unites the two slots of each
 *   components_finish_stray    the last launch of finish */
const char* ammsb_components_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_components_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_COMPONENTS_H_ */
