/* libammsb_cores.so: where does a node sit inside a detected community?  The k-core decomposition of the subgraph every
 * community induces in a simple adjacency, by a level-synchronous parallel peel on the device: per membership its inner
 * degree and its core number, per community the degeneracy, the size of the innermost core (the "nucleus") and the
 * isolated members, per node its deepest membership.  All of them exact integers.
 *
 * Definitions (the contract):
 *   membership      node a is in community k iff pi[a, k] >= thr: a binary32 compare of the stored value, so a NaN is
 *                   never a member.  The bits are the public node-major mask of the community-links library (W = ceil(K /
 *                   64) 64-bit words per node); this library clears the bits past K of every word it reads.  S_a is a's
 *                   set of communities.
 *   slots           exactly the numbering of ammsb_components.h: base[a] is the exclusive prefix sum of own (uint64,
 *                   base[N] = M) and the slot of (a, k in S_a) is base[a] + #{l in S_a : l < k}.  own, slot_node and
 *                   slot_comm come from ammsb_components_own / ammsb_components_slots; there is no second numbering.
 *                   M < 2^32.
 *   adjacency       the simple symmetric CSR of the triangles library: offsets[N + 1] uint64, targets uint32; both
 *                   directions of every valid key, rows strictly ascending, no loops, no repeats.  A row may have any
 *                   length below 2^32 (the 65535-target limit of the triangles library is not inherited).  A target >= N
 *                   is read as a node without a membership.
 *   induced slot graph
 *     indeg[s]      for s = (a, k): #{b in row(a) : k in S_b}
 *     nbr_off       uint64 [M + 1], the exclusive prefix sum of indeg (one 64-bit cumsum on the host side between the two
 *                   build calls); L = nbr_off[M]
 *     nbr           uint32 [L]: nbr[nbr_off[s] + j] = the slot of (b_j, k) for the j-th such b in ascending order, so
 *                   the array is fully determined.  It is symmetric: t is in row s iff s is in row t.
 *                   The kernels read a row as (nbr_off[s], indeg[s]) and never as nbr_off[s + 1] - nbr_off[s]: rows need
 *                   not be packed, and `num_nbr`, the number of entries nbr holds, bounds every index.
 *                   L < 2^32; the hosts also refuse 4 L > max_bytes (4 GiB by default) before any launch, and name the
 *                   threshold.
 *   core number     core[s] = the largest c such that s lies in a subgraph of the slot graph in which every degree is >= c.
 *                   The slot graph is the disjoint union of the K induced subgraphs, so this is the core number of a inside
 *                   community k.  core <= indeg, and core == 0 iff indeg == 0.
 *   per community   (arrays of K; zeroed by the caller, added to)
 *     members       uint64
 *     inlinks2      uint64  the sum of indeg: twice the simple links inside
 *     degeneracy    uint32  the largest core number, 0 for an empty community
 *     nucleus       uint64  #{s in k : core[s] == degeneracy[k]}, 0 for an empty community
 *     isolated      uint64  #{s in k : core[s] == 0}
 *   per node        (arrays of N, written whole)
 *     best_core     uint32  the largest core number over S_a (0 for a node in no community)
 *     best_comm     int32   the lowest k that attains it; -1 for a node in no community
 *     in_nucleus    uint32  #{k in S_a : degeneracy[k] > 0 and core == degeneracy[k]}
 *   counts[4]       M, L, scans, rounds; uint64, zeroed by the caller, added to: degrees adds the slots and the inner
 *                   degrees of its node range, every scan launch adds 1 to scans and every peel launch 1 to rounds.  The
 *                   last two are launch counts, diagnostic only.
 *   limits          K <= 8192; N < 2^32; M < 2^32; L < 2^32
 *
 * Every output is an integer that the cover and the simple adjacency alone determine: exact, the same from run to run,
 * and independent of the kernel form, the grid, the order in which the queue fills and how the node range of the two
 * build passes is cut into calls.
 *
 * The peel.  deg[M] (uint32) starts as a copy of indeg; queue[M] (uint32) holds every slot once, in the order in which
 * the slots leave; *tail (uint64) counts them and *next_level (uint32) is set to 0xFFFFFFFF before a scan.  For level =
 * 0, 1, ... the host
 *   scans           ammsb_cores_scan(level): every slot with deg == level is appended, pos = atomicAdd(tail, 1), queue[pos]
 *                   = s, and a 32-bit atomic min of the deg > level goes into *next_level;
 *   peels           ammsb_cores_peel(level, head, tail) while head < tail: a group of 16 lanes per slot of queue[head ..
 *                   tail) reads the slot's row of nbr and lowers every neighbour t with deg[t] > level by exactly one;
 *                   the lane whose decrement takes deg[t] from level + 1 to level appends t behind *tail.  What a launch
 *                   appends is work of the next launch, never of the same one;
 *   reads back      *tail and *next_level (12 bytes) between launches, and ends when tail == M.  (The slots of level 0
 *                   have no row, so the hosts launch no peel for them.)
 * A slot's degree never goes below the level at which it leaves, so at the end deg is core.
 *   no waiting      no lane ever waits for another lane, wave or block: there is no in-kernel work queue that is polled,
 *                   no grid-wide barrier and no flag that is spun on.  Each peel launch retires at least one slot and a
 *                   slot is queued exactly once (by the scan of its level, or by the one decrement that reaches the
 *                   level), so the host loop is bounded by M launches without a fuse.
 *   stale reads     the L2s of the eight XCDs are not coherent with each other.  The decrement is a compare-and-swap
 *                   loop that starts from a relaxed agent-scope atomic load and, after a failed swap, continues from the
 *                   value the atomic returned, never from a fresh load (the rule ammsb_components.h states for unite).
 *                   deg only decreases, so a stale value is never below the true one: a loaded value <= level proves the
 *                   slot has left, and a larger stale value only makes the first swap fail.  The loop stops as soon as
 *                   the value is <= level; every failed swap means another lane's decrement of the same word succeeded,
 *                   so it runs at most indeg[t] times.
 *   empty levels    after level c is exhausted the host scans c + 1; if that scan queues nothing it jumps to the
 *                   *next_level it found (no peel ran in between, so it is the smallest degree left).  scans is
 *                   therefore at most twice the number of distinct core values plus one, whatever the largest degree.
 *
 * What the hosts derive in float64 (the same statement in _cores.py and in mcmc::Learner::CoresResult::Derive; each
 * integer converted once):
 *   coreness[s]      = float64(core) / float64(degeneracy[k]); -1 where the degeneracy is 0
 *   nucleus_share[k] = float64(nucleus) / float64(members); -1 where members is 0
 *   mean_core[k]     = float64(the sum of core over k, added in integers) / float64(members); -1 where members is 0
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged and no
 * ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a hipStream_t as void*, NULL = the null stream): no
 * allocation, no synchronisation.  Return values are the codes of ammsb.h.  Every call refuses, with AMMSB_EINVAL and
 * before anything is launched or any device pointer is used: num_cols 0 or > 8192, num_rows >= 2^32, num_slots >= 2^32,
 * num_nbr >= 2^32, a node range outside num_rows, head > tail or tail > num_slots, a NULL pointer it would use, and a
 * pointer that is not aligned to its element (8 bytes for the uint64 arrays, 4 for the uint32 / int32 arrays, 2 for
 * slot_comm). */
#ifndef AMMSB_CORES_H_
#define AMMSB_CORES_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_CORES_MAX_COLS 8192u
/* the largest num_cols the one-word-per-lane forms take */
#define AMMSB_CORES_W1_MAX_COLS 4096u
#define AMMSB_CORES_MAX_SLOTS (1ull << 32)
#define AMMSB_CORES_MAX_NBR (1ull << 32)
/* lanes that own a queued slot in the peel */
#define AMMSB_CORES_PEEL_LANES 16u

/* indeg[s] for every slot of the nodes first_row .. first_row + n_rows - 1; adds their slots to counts[0] and their inner
 * degrees to counts[1].  base[num_rows + 1] is the exclusive prefix sum of own; a slot >= num_slots is not written.
 * n_rows == 0 is a valid no-op. */
int ammsb_cores_degrees(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                        const uint64_t* offsets, const uint32_t* targets, uint64_t first_row, uint64_t n_rows, uint32_t* indeg,
                        uint64_t* counts, void* stream);

/* The rows of nbr of the same nodes: for slot s the entries nbr_off[s] .. nbr_off[s] + indeg[s] - 1, in the order of the
 * node's row of targets, so no atomics are needed.  An entry at num_nbr or past it is not written.  n_rows == 0 and
 * num_nbr == 0 are valid no-ops. */
int ammsb_cores_adjacency(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                          const uint64_t* offsets, const uint32_t* targets, uint64_t first_row, uint64_t n_rows,
                          const uint32_t* indeg, const uint64_t* nbr_off, uint64_t num_nbr, uint32_t* nbr, void* stream);

/* Appends every slot with deg[s] == level to queue at *tail, lowers *next_level to the smallest deg > level, counts[2] += 1.
 * num_slots == 0 is a valid no-op. */
int ammsb_cores_scan(uint64_t num_slots, uint32_t level, const uint32_t* deg, uint32_t* queue, uint64_t* tail,
                     uint32_t* next_level, uint64_t* counts, void* stream);

/* One sub-round over queue[head .. tail) at `level` (above); counts[3] += 1.  head == tail is a valid no-op. */
int ammsb_cores_peel(uint64_t num_slots, uint32_t level, uint64_t head, uint64_t tail_now, const uint64_t* nbr_off,
                     const uint32_t* indeg, const uint32_t* nbr, uint64_t num_nbr, uint32_t* deg, uint32_t* queue,
                     uint64_t* tail, uint64_t* counts, void* stream);

/* After the peel, core = deg.  Two launches:
 *   cores_finish_communities  per slot: members += 1, inlinks2 += indeg, isolated += (core == 0), a 32-bit atomic max into
 *                             degeneracy
 *   cores_finish_nodes        a group of lanes per node over its slots: best_core, best_comm, in_nucleus, and nucleus += 1
 *                             at every slot whose core is its community's degeneracy
 * members, inlinks2, degeneracy, nucleus, isolated [num_cols] are zeroed by the caller; best_core, best_comm, in_nucleus
 * [num_rows] are written whole.  num_slots == 0 and num_rows == 0 are valid. */
int ammsb_cores_finish(uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                       const uint16_t* slot_comm, const uint32_t* indeg, const uint32_t* core, uint64_t* members,
                       uint64_t* inlinks2, uint32_t* degeneracy, uint64_t* nucleus, uint64_t* isolated, uint32_t* best_core,
                       int32_t* best_comm, uint32_t* in_nucleus, void* stream);

/* Name of the kernel form the calling thread's last successful call launched last ("" before the first):
 *   cores_degrees_w1 / _w2    a group of lanes (the smallest power of two >= W; above K = 4096 a wave with two words per
 *                             lane) owns a node; the exclusive prefix sum of the words' population counts by shuffles
 *                             gives every lane the slot of its word's first bit; for each target the lane ANDs the
 *                             target's word with its own and counts, four bits of a word per walk of the row
 *   cores_adjacency_w1 / _w2  the same groups and walks; the slot of (b, k) is base[b] plus the population count of b's
 *                             bits below k, the words before the lane's by the same prefix sum over b's row
 *   cores_scan, cores_peel, cores_finish_nodes (the last launch of finish) */
const char* ammsb_cores_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_cores_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_CORES_H_ */
