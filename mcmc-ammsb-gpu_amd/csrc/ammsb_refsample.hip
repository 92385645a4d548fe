// libammsb_refsample.so (include/ammsb_refsample.h): the reference's rand_r mini-batch stream on the device.
//
// A non-link mini-batch is five launches on the caller's stream:
//   rs_draw    candidate j = rand_r call j after u's, reached by jump-ahead on the LCG; v_j = r % N, valid iff
//              Canon(u, v_j) is in neither cuckoo set (v_j == u IS valid, as in the reference); registers
//              (v_j -> min j) in an open-addressing table (the scheme of ammsb_minibatch.hip);
//   rs_count   kept = valid and first occurrence of its v; per-block counts;
//   rs_write   the first m kept candidates, in candidate order, become the insertion sequence; the m-th one's
//              index + 1 is `consumed`;
//   rs_finish  leaves the table empty for the next call;
//   rs_order   ONE 1024-thread block: unordered_set iteration order of the edge sequence (epoch procedure below),
//              the node sequence min(e0), max(e0), min(e1), ... reduced to first occurrences, its order, the result.
// A link mini-batch is rs_link (Canon(u, v) in CSR order) + rs_order.
//
// The epoch procedure (one epoch = a run of inserts under one bucket count, table recorded from a real
// std::unordered_set at creation): S = (list so far) ++ (the epoch's new keys), L = |S|;
//   first[b] = min position in S of a key of bucket b               (atomicMin)
//   cnt[b]   = keys of bucket b                                      (atomicAdd: the final count is what is read)
//   P[p]     = sum of cnt[bucket(q)] over q < p with first[bucket(q)] == q   (exclusive prefix over positions)
//   rank(p)  = (L - P[first[b]] - cnt[b]) + #{q in bucket b : q > p}    -- buckets by first position descending,
//              inside a bucket by position descending; the members of a bucket are collected in the slice
//              [P[first[b]], + cnt[b]) of a scratch array (which slot a member takes depends on arrival order; the
//              count over the slice does not), so a chain of any length is ranked correctly.
// Nothing read depends on the order in which atomics land.  Why one block: the phases of an epoch are separated by
// barriers, 13 epochs x 5 phases x 2 lists at m = 65536; as separate launches that is ~130 kernel boundaries per
// mini-batch, as one block ~130 block barriers.  All arrays are global workspace (65 537 positions x several arrays do
// not fit 160 KB of LDS); a phase boundary is an agent-scope fence + barrier + fence so that no stale L1 line is read.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <unordered_set>
#include <vector>

#include "../../include/ammsb_refsample.h"
#include "ammsb_dev.h"

using namespace ammsb;

namespace {

constexpr int RS_BLOCK = 256;     // draw / count / write
constexpr int RS_ORDER_NT = 1024;  // the ordering block
constexpr uint64_t EMPTY = ~0ull;
constexpr uint32_t NOPOS = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------------------ rand_r
constexpr uint32_t LCG_A = 1103515245u, LCG_C = 12345u;

// glibc rand_r: three LCG steps, 11 + 10 + 10 bits from bit 16 up of the three states
__host__ __device__ inline uint32_t rand_r_step(uint32_t& s) {
  s = s * LCG_A + LCG_C;
  uint32_t r = (s >> 16) & 2047u;
  s = s * LCG_A + LCG_C;
  r = (r << 10) ^ ((s >> 16) & 1023u);
  s = s * LCG_A + LCG_C;
  r = (r << 10) ^ ((s >> 16) & 1023u);
  return r;
}

// state after k LCG steps: the affine map x -> a x + c raised to the k-th power, square-and-multiply
__host__ __device__ inline uint32_t lcg_jump(uint32_t s, uint64_t k) {
  uint32_t a = LCG_A, c = LCG_C, ra = 1u, rc = 0u;
  while (k) {
    if (k & 1) {
      ra = a * ra;
      rc = a * rc + c;
    }
    c = a * c + c;
    a = a * a;
    k >>= 1;
  }
  return ra * s + rc;
}

// ------------------------------------------------------------------------------------------ workspace
struct Epoch {
  uint32_t end;   // insert positions [previous end, end) happen under this bucket count
  uint32_t nb;    // bucket count
  FastMod mod;    // key % nb without a 64-bit division
};

struct RsWork {
  uint64_t* table;    // [H] (v << 32 | j), EMPTY = all ones
  uint32_t* cand;     // [capacity] v_j | valid << 31
  uint32_t* blk;      // [capacity / RS_BLOCK + 1] per-block keep counts
  uint32_t* stat;     // [2] kept candidates of the call, consumed
  uint64_t* seq;      // [max_items] insertion sequence (edges, then nodes)
  uint64_t* list_a;   // [max_items] ping
  uint64_t* list_b;   // [max_items] pong
  uint32_t* first;    // [max_nb]
  uint32_t* cnt;      // [max_nb]
  uint32_t* fill;     // [max_nb]
  uint32_t* bkt;      // [max_items]
  uint32_t* pre;      // [max_items] P
  uint32_t* members;  // [max_items]
  const Epoch* epochs;
  uint32_t n_epochs, max_items, H;
};

inline uint32_t table_size(uint32_t C) {
  uint32_t h = 1024;
  while (h < 4u * C) h <<= 1;
  return h;
}

__device__ __forceinline__ uint32_t mix32(uint32_t x) {  // table slot hash (murmur3 finaliser)
  x ^= x >> 16;
  x *= 0x85ebca6bu;
  x ^= x >> 13;
  x *= 0xc2b2ae35u;
  x ^= x >> 16;
  return x;
}

// ------------------------------------------------------------------------------------------ draw
__global__ __launch_bounds__(RS_BLOCK) void rs_draw_kernel(RsWork w, uint32_t n_cand, uint32_t state, uint32_t u,
                                                           uint32_t N, DevSet training, DevSet heldout,
                                                           int has_heldout) {
  const uint32_t j = blockIdx.x * RS_BLOCK + threadIdx.x;
  if (j >= n_cand) return;
  uint32_t s = lcg_jump(state, 3ull * j);
  const uint32_t v = rand_r_step(s) % N;
  const uint64_t e = make_edge(u, v);
  const bool valid = !set_has(training, e) && !(has_heldout && set_has(heldout, e));
  w.cand[j] = v | (valid ? 0x80000000u : 0u);
  if (!valid) return;
  // "first occurrence of its edge" is keyed on v alone: u is the same for every candidate of a call, so e = Canon(u, v)
  // and v determine each other
  const uint64_t packed = ((uint64_t)v << 32) | j;
  uint32_t h = mix32(v) & (w.H - 1);
  for (uint32_t probes = 0; probes < w.H; ++probes) {  // H >= 4 * capacity: the table can never fill up
    const unsigned long long old = atomicCAS(reinterpret_cast<unsigned long long*>(&w.table[h]),
                                             (unsigned long long)EMPTY, (unsigned long long)packed);
    if (old == EMPTY) break;
    if ((uint32_t)(old >> 32) == v) {
      atomicMin(reinterpret_cast<unsigned long long*>(&w.table[h]), (unsigned long long)packed);
      break;
    }
    h = (h + 1) & (w.H - 1);
  }
}

__device__ __forceinline__ bool rs_keep(const RsWork& w, uint32_t n_cand, uint32_t j) {
  if (j >= n_cand) return false;
  const uint32_t c = w.cand[j];
  if (!(c >> 31)) return false;
  const uint32_t v = c & 0x7fffffffu;
  uint32_t h = mix32(v) & (w.H - 1);
  for (uint32_t probes = 0; probes < w.H; ++probes) {
    const uint64_t t = __hip_atomic_load(&w.table[h], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)(t >> 32) == v) return (uint32_t)t == j;
    if (t == EMPTY) return false;  // cannot happen: this candidate inserted its v or met it
    h = (h + 1) & (w.H - 1);
  }
  return false;
}

template <int NT>
__device__ __forceinline__ uint32_t block_flag_scan(uint32_t flag, uint32_t* total) {
  __shared__ uint32_t wsum[NT / 64];
  const unsigned long long ball = __ballot(flag != 0);
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint32_t before = __popcll(ball & ((1ull << lane) - 1));
  if (lane == 0) wsum[wv] = __popcll(ball);
  __syncthreads();
  uint32_t off = 0, tot = 0;
  for (int i = 0; i < NT / 64; ++i) {
    if (i < (int)wv) off += wsum[i];
    tot += wsum[i];
  }
  *total = tot;
  return off + before;
}

__global__ __launch_bounds__(RS_BLOCK) void rs_count_kernel(RsWork w, uint32_t n_cand) {
  const uint32_t j = blockIdx.x * RS_BLOCK + threadIdx.x;
  uint32_t total;
  block_flag_scan<RS_BLOCK>(rs_keep(w, n_cand, j) ? 1u : 0u, &total);
  if (threadIdx.x == 0) w.blk[blockIdx.x] = total;
}

// every block sums the counts of the blocks before it (a few hundred at most), as ammsb_minibatch.hip does
__global__ __launch_bounds__(RS_BLOCK) void rs_write_kernel(RsWork w, uint32_t n_cand, uint32_t u, uint32_t m) {
  __shared__ uint32_t part[RS_BLOCK / 64];
  uint32_t before = 0;
  for (uint32_t i = threadIdx.x; i < blockIdx.x; i += RS_BLOCK) before += w.blk[i];
  for (int d = 32; d > 0; d >>= 1) before += __shfl_down(before, d, 64);
  if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = before;
  __syncthreads();
  uint32_t base = 0;
  for (int i = 0; i < RS_BLOCK / 64; ++i) base += part[i];
  const uint32_t j = blockIdx.x * RS_BLOCK + threadIdx.x;
  const bool keep = rs_keep(w, n_cand, j);
  uint32_t total;
  const uint32_t rank = base + block_flag_scan<RS_BLOCK>(keep ? 1u : 0u, &total);
  if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) w.stat[0] = base + total;
  if (keep && rank < m) {  // m <= max_items: checked at the call
    w.seq[rank] = make_edge(u, w.cand[j] & 0x7fffffffu);
    if (rank == m - 1) w.stat[1] = j + 1;
  }
}

__global__ void rs_finish_kernel(uint64_t* table, uint32_t H) {
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x, nthreads = gridDim.x * blockDim.x;
  for (uint32_t h = tid; h < H; h += nthreads) table[h] = EMPTY;
}

__global__ void rs_link_kernel(RsWork w, const uint64_t* offsets, const uint32_t* targets, uint32_t u, uint32_t n) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t == 0) {
    w.stat[0] = n;
    w.stat[1] = 0;
  }
  if (t >= n) return;  // n <= max_items: checked at the call
  w.seq[t] = make_edge(u, targets[offsets[u] + t]);
}

// ------------------------------------------------------------------------------------------ order
// phase boundary of the ordering block: everything written before it (plain stores and atomics) is what every thread
// reads after it -- release, barrier, acquire (the acquire drops this CU's L1 lines)
__device__ __forceinline__ void rs_phase() {
  __threadfence();
  __syncthreads();
  __threadfence();
}

__device__ __forceinline__ uint32_t ld_u32(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// exclusive prefix sum of x over the block's threads plus a running carry (all threads call it)
__device__ __forceinline__ uint32_t block_sum_scan(uint32_t x, uint32_t* carry, uint32_t* wsum) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t inc = x;
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    if ((int)lane >= d) inc += t;
  }
  if (lane == 63) wsum[wv] = inc;
  __syncthreads();
  uint32_t off = *carry, tot = 0;
  for (int i = 0; i < RS_ORDER_NT / 64; ++i) {
    if (i < (int)wv) off += wsum[i];
    tot += wsum[i];
  }
  __syncthreads();
  if (threadIdx.x == 0) *carry += tot;
  __syncthreads();
  return off + inc - x;
}

// unordered_set iteration order of the n unique keys w.seq[0..n); returns the buffer that holds it
__device__ uint64_t* rs_order_list(const RsWork& w, uint32_t n, uint32_t* carry, uint32_t* wsum) {
  uint64_t *cur = w.list_a, *nxt = w.list_b;
  const uint32_t tid = threadIdx.x;
  uint32_t start = 0;
  for (uint32_t e = 0; e < w.n_epochs && start < n; ++e) {
    const Epoch ep = w.epochs[e];
    const uint32_t L = ep.end < n ? ep.end : n, nb = ep.nb;
    for (uint32_t b = tid; b < nb; b += RS_ORDER_NT) {
      w.first[b] = NOPOS;
      w.cnt[b] = 0;
      w.fill[b] = 0;
    }
    for (uint32_t p = start + tid; p < L; p += RS_ORDER_NT) cur[p] = w.seq[p];
    if (tid == 0) *carry = 0;
    rs_phase();
    for (uint32_t p = tid; p < L; p += RS_ORDER_NT) {
      const uint32_t b = (uint32_t)fast_mod(cur[p], ep.mod);
      w.bkt[p] = b;
      atomicMin(&w.first[b], p);
      atomicAdd(&w.cnt[b], 1u);
    }
    rs_phase();
    for (uint32_t p0 = 0; p0 < L; p0 += RS_ORDER_NT) {
      const uint32_t p = p0 + tid;
      uint32_t head = 0;
      if (p < L) {
        const uint32_t b = w.bkt[p];
        if (ld_u32(&w.first[b]) == p) head = ld_u32(&w.cnt[b]);
      }
      const uint32_t ex = block_sum_scan(head, carry, wsum);
      if (p < L) w.pre[p] = ex;
    }
    rs_phase();
    for (uint32_t p = tid; p < L; p += RS_ORDER_NT) {
      const uint32_t b = w.bkt[p];
      if (ld_u32(&w.cnt[b]) > 1) {
        const uint32_t slot = w.pre[ld_u32(&w.first[b])] + atomicAdd(&w.fill[b], 1u);
        if (slot < w.max_items) w.members[slot] = p;
      }
    }
    rs_phase();
    for (uint32_t p = tid; p < L; p += RS_ORDER_NT) {
      const uint32_t b = w.bkt[p], c = ld_u32(&w.cnt[b]), base = w.pre[ld_u32(&w.first[b])];
      uint32_t larger = 0;
      if (c > 1)
        for (uint32_t i = 0; i < c && base + i < w.max_items; ++i) larger += ld_u32(&w.members[base + i]) > p ? 1u : 0u;
      const uint32_t rank = L - base - c + larger;
      if (rank < w.max_items) nxt[rank] = cur[p];
    }
    rs_phase();
    uint64_t* t = cur;
    cur = nxt;
    nxt = t;
    start = L;
  }
  return cur;
}

__global__ __launch_bounds__(RS_ORDER_NT) void rs_order_kernel(RsWork w, uint32_t u, uint32_t m, uint32_t n_cand,
                                                               uint64_t* edges_out, uint32_t* nodes_out,
                                                               ammsb_refsample_result* result) {
  __shared__ uint32_t carry, wsum[RS_ORDER_NT / 64], self_at;
  const uint32_t tid = threadIdx.x;
  const uint32_t kept = w.stat[0];
  const uint32_t n = kept < m ? kept : m;  // a link mini-batch passes m = its edge count
  const bool shortfall = kept < m;
  if (tid == 0) self_at = NOPOS;
  const uint64_t* el = rs_order_list(w, n, &carry, wsum);
  // edges out; the node sequence min(e0), max(e0), min(e1), ... without repeats.  Every edge has u at one end and
  // the other ends are distinct, so: e0 gives (min, max) -- one entry if it is (u, u) -- and every later edge its
  // other end, except a later (u, u), which gives nothing.
  const uint64_t self = ((uint64_t)u << 32) | u;
  for (uint32_t i = tid; i < n; i += RS_ORDER_NT) {
    const uint64_t e = el[i];
    edges_out[i] = e;
    if (e == self) self_at = i;  // at most one: keys are unique
  }
  __syncthreads();
  const uint32_t z = self_at;
  const uint32_t n_nodes = n == 0 ? 0 : n + 1 - (z != NOPOS ? 1u : 0u);
  for (uint32_t i = tid; i < n; i += RS_ORDER_NT) {
    const uint64_t e = el[i];
    const uint32_t lo = (uint32_t)(e >> 32), hi = (uint32_t)e;
    if (i == 0) {
      w.seq[0] = lo;
      if (hi != lo) w.seq[1] = hi;
    } else if (e != self) {
      w.seq[i + 1 - (z < i ? 1u : 0u)] = lo == u ? hi : lo;  // <= n < max_items
    }
  }
  rs_phase();
  const uint64_t* nl = rs_order_list(w, n_nodes, &carry, wsum);
  for (uint32_t i = tid; i < n_nodes; i += RS_ORDER_NT) nodes_out[i] = (uint32_t)nl[i];
  if (tid == 0) {
    result->n_edges = n;
    result->n_nodes = n_nodes;
    result->consumed = shortfall ? n_cand : w.stat[1];
    result->shortfall = shortfall ? 1u : 0u;
  }
}

// ------------------------------------------------------------------------------------------ host helpers
void epoch_table(uint64_t max_items, std::vector<uint64_t>* ends, std::vector<uint64_t>* buckets) {
  std::unordered_set<uint64_t> s;
  uint64_t prev = 0;
  for (uint64_t i = 0; i < max_items; ++i) {
    s.insert(i);
    const uint64_t bc = s.bucket_count();  // a rehash happens before the insert that triggers it
    if (bc != prev) {
      if (i > 0) ends->push_back(i);
      buckets->push_back(bc);
      prev = bc;
    }
  }
  if (max_items > 0) ends->push_back(max_items);
}

}  // namespace

struct ammsb_refsample {
  int device;
  uint64_t N;
  uint32_t m, capacity, max_items;
  RsWork w;
  void* dev_block;
  ammsb_refsample_result* result;
  uint32_t n_epochs;
  char err[256];
};

#define RS_FAIL(h, code, ...)                                      \
  do {                                                             \
    if (h) snprintf((h)->err, sizeof((h)->err), __VA_ARGS__);      \
    return code;                                                   \
  } while (0)

extern "C" {

uint32_t ammsb_refsample_rand_r(uint32_t* state) { return rand_r_step(*state); }

uint32_t ammsb_refsample_jump(uint32_t state, uint64_t calls) { return lcg_jump(state, 3 * calls); }

uint32_t ammsb_refsample_epochs(uint64_t max_items, uint64_t* ends, uint64_t* buckets, uint32_t cap) {
  std::vector<uint64_t> e, b;
  epoch_table(max_items, &e, &b);
  for (size_t i = 0; i < e.size() && i < cap; ++i) {
    if (ends) ends[i] = e[i];
    if (buckets) buckets[i] = b[i];
  }
  return (uint32_t)e.size();
}

uint64_t ammsb_refsample_host_order(const uint64_t* keys, uint64_t n, uint64_t* out) {
  if (!keys || !out) return 0;
  std::vector<uint64_t> seq;  // first occurrences, in order
  {
    std::vector<uint64_t> sorted(keys, keys + n);
    std::sort(sorted.begin(), sorted.end());
    std::vector<uint8_t> seen(n, 0);
    for (uint64_t i = 0; i < n; ++i) {
      const size_t at = std::lower_bound(sorted.begin(), sorted.end(), keys[i]) - sorted.begin();
      if (!seen[at]) {
        seen[at] = 1;
        seq.push_back(keys[i]);
      }
    }
  }
  std::vector<uint64_t> ends, buckets;
  epoch_table(seq.size(), &ends, &buckets);
  std::vector<uint64_t> cur(seq.size()), nxt(seq.size());
  uint64_t start = 0;
  for (size_t e = 0; e < ends.size(); ++e) {
    const uint64_t L = ends[e], nb = buckets[e];
    for (uint64_t p = start; p < L; ++p) cur[p] = seq[p];
    std::vector<uint64_t> first(nb, ~0ull), cnt(nb, 0), pre(L + 1, 0);
    for (uint64_t p = 0; p < L; ++p) {
      const uint64_t b = cur[p] % nb;
      if (first[b] == ~0ull) first[b] = p;
      ++cnt[b];
    }
    for (uint64_t p = 0; p < L; ++p) pre[p + 1] = pre[p] + (first[cur[p] % nb] == p ? cnt[cur[p] % nb] : 0);
    std::vector<uint64_t> seen_after(nb, 0);  // walking positions downwards: same-bucket keys with a larger position
    for (uint64_t p = L; p-- > 0;) {
      const uint64_t b = cur[p] % nb;
      nxt[L - pre[first[b]] - cnt[b] + seen_after[b]] = cur[p];
      ++seen_after[b];
    }
    cur.swap(nxt);
    start = L;
  }
  std::copy(cur.begin(), cur.end(), out);
  return cur.size();
}

int ammsb_refsample_choose(int strategy, uint64_t N, const uint32_t* degree, uint32_t* seed, uint32_t* link,
                           uint32_t* u) {
  if (!degree || !seed || !link || !u || N == 0 || N >= (1ull << 31)) return -1;
  bool is_link;
  switch (strategy) {
    case AMMSB_REFSAMPLE_NODE: is_link = (rand_r_step(*seed) % 2) != 0; break;  // sample.cc:297
    case AMMSB_REFSAMPLE_NODE_LINK: is_link = true; break;
    case AMMSB_REFSAMPLE_NODE_NONLINK: is_link = false; break;
    default: return -1;
  }
  *link = is_link ? 1u : 0u;
  if (!is_link) {
    *u = (uint32_t)(rand_r_step(*seed) % N);
    return 0;
  }
  // sampleNodeLink's loop; it would never end on a graph without edges, and neither should a caller get here with one.
  // The LCG has period 2^32: if no vertex with an edge turned up in that many calls none ever will.
  for (uint64_t calls = 0; calls < (1ull << 32); ++calls) {
    const uint32_t v = (uint32_t)(rand_r_step(*seed) % N);
    // sample.cc:254-263 skips a vertex already in `tried`.  The degrees do not change during a call, so a vertex that
    // comes up again had no edge the first time either and fails this test again: `tried` changes nothing here.
    if (degree[v] > 0) {
      *u = v;
      return 0;
    }
  }
  return -2;
}

int ammsb_refsample_create(int device, uint64_t N, uint32_t m, uint32_t capacity, uint32_t max_items,
                           ammsb_refsample** out) {
  if (!out) return AMMSB_EINVAL;
  *out = nullptr;
  if (N == 0 || N >= (1ull << 31) || m == 0 || max_items < m + 1 || max_items > (1u << 30) ||
      capacity % RS_BLOCK != 0 || capacity > 0x40000000u)
    return AMMSB_EINVAL;
  if (hipSetDevice(device) != hipSuccess) return AMMSB_ENODEV;
  std::vector<uint64_t> ends, buckets;
  epoch_table(max_items, &ends, &buckets);
  std::vector<Epoch> ep(ends.size());
  uint64_t max_nb = 1;
  for (size_t i = 0; i < ends.size(); ++i) {
    if (buckets[i] >= (1ull << 32)) return AMMSB_EINVAL;
    ep[i] = Epoch{(uint32_t)ends[i], (uint32_t)buckets[i], fast_mod_init(buckets[i])};
    max_nb = std::max(max_nb, buckets[i]);
  }
  ammsb_refsample* h = new ammsb_refsample();
  h->device = device;
  h->N = N;
  h->m = m;
  h->capacity = capacity;
  h->max_items = max_items;
  h->n_epochs = (uint32_t)ep.size();
  h->err[0] = 0;
  const uint32_t H = table_size(capacity ? capacity : 1);
  size_t off = 0;
  auto take = [&off](size_t bytes) {
    const size_t at = off;
    off += (bytes + 255) / 256 * 256;
    return at;
  };
  const size_t o_table = take(sizeof(uint64_t) * H), o_cand = take(sizeof(uint32_t) * (capacity + 1)),
               o_blk = take(sizeof(uint32_t) * (capacity / RS_BLOCK + 2)), o_stat = take(sizeof(uint32_t) * 2),
               o_seq = take(sizeof(uint64_t) * max_items), o_la = take(sizeof(uint64_t) * max_items),
               o_lb = take(sizeof(uint64_t) * max_items), o_first = take(sizeof(uint32_t) * max_nb),
               o_cnt = take(sizeof(uint32_t) * max_nb), o_fill = take(sizeof(uint32_t) * max_nb),
               o_bkt = take(sizeof(uint32_t) * max_items), o_pre = take(sizeof(uint32_t) * max_items),
               o_mem = take(sizeof(uint32_t) * max_items), o_ep = take(sizeof(Epoch) * ep.size());
  char* base = nullptr;
  if (hipMalloc(reinterpret_cast<void**>(&base), off) != hipSuccess ||
      hipHostMalloc(reinterpret_cast<void**>(&h->result), sizeof(ammsb_refsample_result), hipHostMallocDefault) !=
          hipSuccess) {
    if (base) (void)hipFree(base);
    delete h;
    return AMMSB_EHIP;
  }
  memset(h->result, 0, sizeof(*h->result));
  h->dev_block = base;
  bool ok = hipMemset(base, 0, off) == hipSuccess;
  ok = ok && hipMemset(base + o_table, 0xFF, sizeof(uint64_t) * H) == hipSuccess;  // the empty table
  ok = ok && hipMemcpy(base + o_ep, ep.data(), sizeof(Epoch) * ep.size(), hipMemcpyHostToDevice) == hipSuccess;
  ok = ok && hipDeviceSynchronize() == hipSuccess;
  if (!ok) {
    ammsb_refsample_destroy(h);
    return AMMSB_EHIP;
  }
  RsWork& w = h->w;
  w.table = reinterpret_cast<uint64_t*>(base + o_table);
  w.cand = reinterpret_cast<uint32_t*>(base + o_cand);
  w.blk = reinterpret_cast<uint32_t*>(base + o_blk);
  w.stat = reinterpret_cast<uint32_t*>(base + o_stat);
  w.seq = reinterpret_cast<uint64_t*>(base + o_seq);
  w.list_a = reinterpret_cast<uint64_t*>(base + o_la);
  w.list_b = reinterpret_cast<uint64_t*>(base + o_lb);
  w.first = reinterpret_cast<uint32_t*>(base + o_first);
  w.cnt = reinterpret_cast<uint32_t*>(base + o_cnt);
  w.fill = reinterpret_cast<uint32_t*>(base + o_fill);
  w.bkt = reinterpret_cast<uint32_t*>(base + o_bkt);
  w.pre = reinterpret_cast<uint32_t*>(base + o_pre);
  w.members = reinterpret_cast<uint32_t*>(base + o_mem);
  w.epochs = reinterpret_cast<const Epoch*>(base + o_ep);
  w.n_epochs = h->n_epochs;
  w.max_items = max_items;
  w.H = H;
  *out = h;
  return AMMSB_OK;
}

void ammsb_refsample_destroy(ammsb_refsample* h) {
  if (!h) return;
  if (h->dev_block) (void)hipFree(h->dev_block);
  if (h->result) (void)hipHostFree(h->result);
  delete h;
}

const char* ammsb_refsample_last_error(const ammsb_refsample* h) { return h ? h->err : "null handle"; }

uint32_t ammsb_refsample_num_epochs(const ammsb_refsample* h) { return h ? h->n_epochs : 0; }

const ammsb_refsample_result* ammsb_refsample_result_ptr(const ammsb_refsample* h) { return h ? h->result : nullptr; }

int ammsb_refsample_nonlink(ammsb_refsample* h, uint32_t u, uint32_t state, uint32_t n_candidates,
                            const ammsb_set* training_set, const ammsb_set* heldout_set, uint64_t* edges_out,
                            uint32_t* nodes_out, void* stream) {
  if (!h) return AMMSB_EINVAL;
  if (!training_set || !edges_out || !nodes_out) RS_FAIL(h, AMMSB_EINVAL, "%s: null argument", __func__);
  if (!training_set->slots || training_set->num_bins == 0 || training_set->prime_idx >= 4)
    RS_FAIL(h, AMMSB_EINVAL, "%s: bad training set", __func__);
  if (heldout_set && (!heldout_set->slots || heldout_set->num_bins == 0 || heldout_set->prime_idx >= 4))
    RS_FAIL(h, AMMSB_EINVAL, "%s: bad held-out set", __func__);
  if (u >= h->N) RS_FAIL(h, AMMSB_EINVAL, "%s: bad vertex", __func__);
  if (n_candidates == 0 || n_candidates > h->capacity || n_candidates % RS_BLOCK != 0)
    RS_FAIL(h, AMMSB_EINVAL, "%s: candidates exceed the workspace capacity", __func__);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint32_t nb = n_candidates / RS_BLOCK;
  const ammsb_set none = {nullptr, 1, 0};
  rs_draw_kernel<<<nb, RS_BLOCK, 0, s>>>(h->w, n_candidates, state, u, (uint32_t)h->N, dev_set(*training_set),
                                         dev_set(heldout_set ? *heldout_set : none), heldout_set ? 1 : 0);
  rs_count_kernel<<<nb, RS_BLOCK, 0, s>>>(h->w, n_candidates);
  rs_write_kernel<<<nb, RS_BLOCK, 0, s>>>(h->w, n_candidates, u, h->m);
  rs_finish_kernel<<<64, 256, 0, s>>>(h->w.table, h->w.H);
  rs_order_kernel<<<1, RS_ORDER_NT, 0, s>>>(h->w, u, h->m, n_candidates, edges_out, nodes_out, h->result);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) RS_FAIL(h, AMMSB_EHIP, "%s: %s", __func__, hipGetErrorString(e));
  return AMMSB_OK;
}

int ammsb_refsample_link(ammsb_refsample* h, const uint64_t* csr_offsets, const uint32_t* csr_targets, uint32_t u,
                         uint32_t n, uint64_t* edges_out, uint32_t* nodes_out, void* stream) {
  if (!h) return AMMSB_EINVAL;
  if (!csr_offsets || !csr_targets || !edges_out || !nodes_out) RS_FAIL(h, AMMSB_EINVAL, "%s: null argument", __func__);
  if (u >= h->N || n == 0) RS_FAIL(h, AMMSB_EINVAL, "%s: vertex has no training edge", __func__);
  if (n + 1 > h->max_items) RS_FAIL(h, AMMSB_EINVAL, "%s: degree exceeds the workspace (max_items)", __func__);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  rs_link_kernel<<<(n + 255) / 256, 256, 0, s>>>(h->w, csr_offsets, csr_targets, u, n);
  rs_order_kernel<<<1, RS_ORDER_NT, 0, s>>>(h->w, u, n, 0, edges_out, nodes_out, h->result);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) RS_FAIL(h, AMMSB_EHIP, "%s: %s", __func__, hipGetErrorString(e));
  return AMMSB_OK;
}

}  // extern "C"
