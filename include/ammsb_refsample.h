/* libammsb_refsample.so: the reference's rand_r mini-batch stream, drawn on the device.
 *
 * What mcmc::sampleNode / sampleNodeLink / sampleNodeNonLink + ExtractNodesFromMiniBatch produce on one host thread
 * (mcmc/sample.cc:249-303, learner.cc:162-173: one rand_r stream, two std::unordered_sets whose iteration order
 * becomes the edge and the node order) is reproduced here bit for bit from the same Sample::seed, without a
 * host-to-device copy of edges or nodes per mini-batch:
 *   - glibc's rand_r is three steps of a 32-bit LCG, so candidate j's draw is reached by jump-ahead in O(log j);
 *   - libstdc++'s unordered_set iteration order (identity hash, unique keys) is a sequence of sorts, one per "epoch"
 *     of constant bucket count: (list so far) ++ (the epoch's new keys), ordered by (position at which the key's
 *     bucket first became non-empty, descending; own position, descending).  The epoch table is recorded at creation
 *     from a real std::unordered_set, so it is the table of the libstdc++ this library was built against.
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged.
 * Every function returns 0 on success unless stated; ammsb_refsample_last_error() has the text of the last failure. */
#ifndef AMMSB_REFSAMPLE_H_
#define AMMSB_REFSAMPLE_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ammsb_refsample ammsb_refsample;

enum { AMMSB_REFSAMPLE_NODE = 0, AMMSB_REFSAMPLE_NODE_LINK = 1, AMMSB_REFSAMPLE_NODE_NONLINK = 2 };

/* what a mini-batch reports to the host (host-mapped pinned memory, written by the last kernel of the chain) */
typedef struct {
  uint32_t n_edges;    /* edges written */
  uint32_t n_nodes;    /* nodes written */
  uint32_t consumed;   /* non-link: rand_r calls after the one that chose u (index of the m-th kept candidate + 1) */
  uint32_t shortfall;  /* 1: fewer than m kept candidates among those drawn -- NOT a valid mini-batch */
} ammsb_refsample_result;

/* ---- host helpers (no device needed) ---- */

/* glibc's rand_r restated: advances *state, returns the value */
uint32_t ammsb_refsample_rand_r(uint32_t* state);
/* the state after `calls` further rand_r calls, by square-and-multiply on the LCG's affine map */
uint32_t ammsb_refsample_jump(uint32_t state, uint64_t calls);
/* Epochs of constant bucket count of a std::unordered_set that receives max_items unique keys: epoch e holds the
 * insert positions [ends[e-1], ends[e]) (ends[-1] = 0) under buckets[e] buckets.  Returns the number of epochs (also
 * when it exceeds cap: only cap entries are written). */
uint32_t ammsb_refsample_epochs(uint64_t max_items, uint64_t* ends, uint64_t* buckets, uint32_t cap);
/* The epoch procedure on the host, as the device runs it: iteration order of an unordered_set<uint64_t> (or
 * <uint32_t>: same hash) that received keys[0..n) in order; duplicates allowed.  Returns the number of keys in out. */
uint64_t ammsb_refsample_host_order(const uint64_t* keys, uint64_t n, uint64_t* out);
/* The host's share of one mini-batch (sample.cc:249-303): the coin of `Node`, then u -- for a link mini-batch the
 * whole retry loop of sampleNodeLink (a vertex without training edges or a repeated one consumes a call).
 * degree: [N] training degrees.  *seed advances exactly as far as the reference's has when u is known. */
int ammsb_refsample_choose(int strategy, uint64_t N, const uint32_t* degree, uint32_t* seed, uint32_t* link,
                           uint32_t* u);

/* ---- device ---- */

/* capacity: most candidates a non-link call may draw (multiple of 256; ammsb_minibatch_candidates_for);
 * max_items: longest edge or node list (>= m + 1 and >= largest degree + 1).  Allocates the workspace and the
 * pinned result once; nothing is allocated per call. */
int ammsb_refsample_create(int device, uint64_t N, uint32_t m, uint32_t capacity, uint32_t max_items,
                           ammsb_refsample** out);
void ammsb_refsample_destroy(ammsb_refsample* h);
const char* ammsb_refsample_last_error(const ammsb_refsample* h);
uint32_t ammsb_refsample_num_epochs(const ammsb_refsample* h);
/* where the chain's last kernel writes (valid once the stream has passed the call) */
const ammsb_refsample_result* ammsb_refsample_result_ptr(const ammsb_refsample* h);

/* sampleNodeNonLink after u is known: state = rand_r state after u's call; candidates j = 0 .. n_candidates-1 are the
 * following calls.  edges_out: [>= m], nodes_out: [>= m + 1].  heldout_set may be NULL. */
int ammsb_refsample_nonlink(ammsb_refsample* h, uint32_t u, uint32_t state, uint32_t n_candidates,
                            const ammsb_set* training_set, const ammsb_set* heldout_set, uint64_t* edges_out,
                            uint32_t* nodes_out, void* stream);
/* sampleNodeLink after u is known: the n = degree(u) training edges of u.  The CSR must list neighbours in the host
 * Graph's adjacency order and hold no self-loop.  edges_out: [>= n], nodes_out: [>= n + 1]. */
int ammsb_refsample_link(ammsb_refsample* h, const uint64_t* csr_offsets, const uint32_t* csr_targets, uint32_t u,
                         uint32_t n, uint64_t* edges_out, uint32_t* nodes_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_REFSAMPLE_H_ */
