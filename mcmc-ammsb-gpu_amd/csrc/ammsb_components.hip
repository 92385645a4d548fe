// libammsb_components.so (include/ammsb_components.h): the connected components of every detected community inside the
// graph of an edge list, by a lock-free union-find over the memberships ("slots": node by node, communities ascending).
//
//   components_own_w1 / _w2     a group of lanes per node (the smallest power of two >= W; a wave with two words per lane
//                               above K = 4096): the population count of the row.
//   components_slots_w1 / _w2   the same groups: the exclusive prefix sum of the words' population counts by shuffles, then
//                               every lane walks its bits: slot_node, slot_comm, parent[s] = s.
//   components_edges_w1 / _w2   the edge pass of ammsb_modularity.hip with other work per edge: a group owns an edge over a
//                               persistent grid and requests the next edge's words before this one's unions.  Both rows'
//                               prefix sums in one scan (packed 16 + 16 bits: a row has at most 8192 bits), then a lane
//                               walks the set bits of Sa_word & Sb_word and unites the two slots of each bit.
//   components_finish_*         five launches (the header lists them); the kernel boundary makes the unions visible.
//
// The union-find: parent[x] <= x always, find halves paths, unite hooks the larger root under the smaller by a 32-bit
// compare-and-swap.  Indices only decrease, so no cycle can form, and no lane ever waits for another: there is no lock.
// Two things are specific to this machine:
//   stale reads    the L2s of the eight XCDs are not coherent with each other, so a load of parent[] may return an older
//                  value.  Every value parent[x] ever held is a member of x's set that is <= x, so find stays correct: it
//                  may stop at a slot that is no longer a root, and then the compare-and-swap fails.  The retry continues
//                  FROM THE VALUE THE ATOMIC RETURNED, never from a fresh load of parent[x], which could repeat the stale
//                  value for ever; every failed hook therefore moves to a strictly smaller index.  Loads and halving stores
//                  of parent are relaxed agent-scope atomics (they bypass the CU's L1), not plain accesses.
//   bounded loops  a find or hook that takes more than MAX_STEPS = 2^20 steps stops, counts[3] += 1, and that union stays
//                  undone; the hosts raise on it.
//
// The mask is read through mask_word() of ammsb_postfit.h alone (bits past K cleared), and no slot >= num_slots or
// community >= K is used as an index: the mask and base are public buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_components.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int C_WAVES = 4;  // waves per block
constexpr int C_BLOCK = 64 * C_WAVES;
constexpr int C_TRIPS = 2;  // items a group takes before another block is worth it: the second trip's loads are in flight
constexpr uint32_t MAX_STEPS = AMMSB_COMPONENTS_MAX_STEPS;

struct Args {
  const u64* mask;
  uint32_t rows, K, W;
  uint32_t gshift;  // w1: log2 of the lanes that own an item, the smallest power of two >= W
  const u64* base;
  u64 M;  // slots
  const u64* edges;
  uint64_t first, n;  // slots: the node range; edges: n keys
  uint32_t* own;
  uint32_t* slot_node;
  uint16_t* slot_comm;
  uint32_t* parent;
  u64* counts;
};

struct Finish {
  uint32_t rows, K, gshift;
  const u64* base;
  u64 M;
  const uint32_t* slot_node;
  const uint16_t* slot_comm;
  uint32_t* parent;
  uint32_t* root;
  uint32_t* size;
  u64 *members, *components, *singletons, *best;
  uint32_t* largest;
  int32_t* largest_root;
  uint32_t* stray;
  u64* counts;
};

// the sum of v over the lanes of a group of G
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t G) {
  for (uint32_t o = G >> 1; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o, 64);  // o < G: stays inside the group
  return v;
}

// the sum of v over the lanes before this one in its group of G (gl: the lane's place in it)
__device__ __forceinline__ uint32_t group_before(uint32_t v, uint32_t G, uint32_t gl) {
  uint32_t inc = v;
  for (uint32_t o = 1; o < G; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)inc, o, 64);
    if (gl >= o) inc += t;  // (a lane nearer than o to its group's start takes nothing from the group before)
  }
  return inc - v;
}

// ------------------------------------------------------------------------------------------ the union-find
__device__ __forceinline__ uint32_t load_parent(uint32_t* parent, uint32_t x) {
  return __hip_atomic_load(&parent[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The root of x as this lane can see it, halving the path on the way: a value that may be stale, but is a member of x's set
// that is <= x.  steps counts across the calls of one union; false: the fuse.
__device__ __forceinline__ bool find(uint32_t* parent, uint32_t& x, uint32_t& steps) {
  uint32_t p = load_parent(parent, x);
  while (p < x) {  // (p > x is no state this library makes: it ends the walk as a root would)
    if (++steps > MAX_STEPS) return false;
    const uint32_t g = load_parent(parent, p);
    if (g < p) __hip_atomic_store(&parent[x], g, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // g <= p < x: x is no root
    x = g < p ? g : p;
    p = g < p ? load_parent(parent, g) : p;
  }
  return true;
}

// false: the fuse, and the union is left undone
__device__ __forceinline__ bool unite(uint32_t* parent, uint32_t a, uint32_t b) {
  uint32_t steps = 0;
  if (!find(parent, a, steps) || !find(parent, b, steps)) return false;
  while (a != b) {
    if (++steps > MAX_STEPS) return false;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    // hook the larger root under the smaller
    uint32_t seen = a;
    if (__hip_atomic_compare_exchange_strong(&parent[a], &seen, b, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
      return true;
    if (seen >= a) return false;  // (no state this library makes)
    // a was no root: go on from what the atomic saw there (< a), not from a load that may still show a as a root
    a = seen;
    if (!find(parent, a, steps)) return false;
  }
  return true;
}

// ------------------------------------------------------------------------------------------ own, slots
template <int WPL>
__device__ __forceinline__ void own_body(const Args& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  for (uint64_t rb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw; rb < a.rows; rb += stride) {
    const uint64_t r = rb + slot;
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) o += r < a.rows ? (uint32_t)__popcll(mask_word(a, (uint32_t)r, gl + 64u * i)) : 0u;
    o = group_sum(o, G);
    if (r < a.rows && gl == 0) a.own[r] = o;
  }
}

__global__ __launch_bounds__(C_BLOCK) void components_own_w1(Args a) { own_body<1>(a); }
__global__ __launch_bounds__(C_BLOCK) void components_own_w2(Args a) { own_body<2>(a); }

template <int WPL>
__device__ __forceinline__ void slots_body(const Args& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  for (uint64_t rb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw; rb < a.n; rb += stride) {
    const bool have = rb + slot < a.n;
    const uint32_t r = (uint32_t)(a.first + rb + slot);  // (< rows < 2^32 where have)
    u64 x[WPL];
    uint32_t before = 0;  // the bits of the row in the words before the lane's word i
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      x[i] = have ? mask_word(a, r, gl + 64u * i) : 0ull;
      const uint32_t c = (uint32_t)__popcll(x[i]);
      const uint32_t ex = group_before(c, G, gl);
      const uint32_t mine = before + ex;
      if (i + 1 < WPL) before += (uint32_t)__shfl((int)(ex + c), 63, 64);  // (WPL == 2: G == 64, the last lane holds the total)
      u64 s = (have ? a.base[r] : 0ull) + mine;
      for (u64 bits = x[i]; bits; bits &= bits - 1, ++s) {
        if (s >= a.M) break;  // (a base that is not this mask's)
        a.slot_node[s] = r;
        a.slot_comm[s] = (uint16_t)(64u * (gl + 64u * i) + (uint32_t)__builtin_ctzll(bits));
        a.parent[s] = (uint32_t)s;
      }
    }
  }
}

__global__ __launch_bounds__(C_BLOCK) void components_slots_w1(Args a) { slots_body<1>(a); }
__global__ __launch_bounds__(C_BLOCK) void components_slots_w2(Args a) { slots_body<2>(a); }

// ------------------------------------------------------------------------------------------ edges
template <int WPL>
struct Ends {
  bool exists, ok;  // the lane's group has an edge; both its ends are < num_rows
  u64 bu, bv;       // base of both ends
  u64 x[WPL], y[WPL];
};

// the edge of the lane's group, the lane's words of both rows and the first slot of both ends (zeros where there is
// nothing to read)
template <int WPL>
__device__ __forceinline__ void head(const Args& a, uint64_t p, uint32_t gl, Ends<WPL>& e) {
  e.exists = p < a.n;
  e.ok = false;
  uint32_t u = 0, v = 0;
  if (e.exists) {
    const u64 key = a.edges[p];
    u = (uint32_t)(key >> 32);
    v = (uint32_t)key;
    e.ok = u < a.rows && v < a.rows;
  }
  e.bu = e.ok ? a.base[u] : 0ull;
  e.bv = e.ok ? a.base[v] : 0ull;
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    e.x[i] = e.ok ? mask_word(a, u, gl + 64u * i) : 0ull;
    e.y[i] = e.ok ? mask_word(a, v, gl + 64u * i) : 0ull;
  }
}

template <int WPL>
__device__ __forceinline__ void edges_body(const Args& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  uint64_t pb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw;  // the wave's first edge: wave-uniform
  u64 valid = 0, skipped = 0;   // of this wave's edges: wave-uniform
  u64 shared = 0, giveups = 0;  // of this lane
  Ends<WPL> e;
  head<WPL>(a, pb + slot, gl, e);
  for (; pb < a.n; pb += stride) {
    const bool exists = e.exists, ok = e.ok;
    const u64 bu = e.bu, bv = e.bv;
    u64 x[WPL], y[WPL];
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      x[i] = e.x[i];
      y[i] = e.y[i];
    }
    head<WPL>(a, pb + stride + slot, gl, e);  // the next edge's words are on their way during the unions
    valid += (u64)__popcll(__ballot(ok && gl == 0));
    skipped += (u64)__popcll(__ballot(exists && !ok && gl == 0));
    uint32_t before = 0;  // both rows' bits in the words before the lane's word i, packed: a's low, b's << 16 (each <= 8192)
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const uint32_t c = (uint32_t)__popcll(x[i]) | ((uint32_t)__popcll(y[i]) << 16);
      const uint32_t ex = group_before(c, G, gl);
      const uint32_t mine = before + ex;
      if (i + 1 < WPL) before += (uint32_t)__shfl((int)(ex + c), 63, 64);  // (WPL == 2: G == 64)
      const u64 sa0 = bu + (mine & 0xFFFFu), sb0 = bv + (mine >> 16);
      const u64 both = x[i] & y[i];
      shared += (u64)__popcll(both);
      for (u64 bits = both; bits; bits &= bits - 1) {
        const u64 below = (bits & (0ull - bits)) - 1ull;  // the bits under the lowest set one
        const u64 sa = sa0 + (u64)__popcll(x[i] & below), sb = sb0 + (u64)__popcll(y[i] & below);
        if (sa >= a.M || sb >= a.M) continue;  // (a base that is not this mask's)
        if (!unite(a.parent, (uint32_t)sa, (uint32_t)sb)) ++giveups;
      }
    }
  }
  shared = wave_sum_u64(shared);
  giveups = wave_sum_u64(giveups);
  if (lane == 0) {
    if (valid) atomicAdd(&a.counts[0], valid);
    if (skipped) atomicAdd(&a.counts[1], skipped);
    if (shared) atomicAdd(&a.counts[2], shared);
    if (giveups) atomicAdd(&a.counts[3], giveups);
  }
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(C_BLOCK) void components_edges_w1(Args a) { edges_body<1>(a); }
__global__ __launch_bounds__(C_BLOCK) void components_edges_w2(Args a) { edges_body<2>(a); }

// ------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(C_BLOCK) void components_finish_roots(Finish f) {
  const u64 stride = (u64)gridDim.x * C_BLOCK;
  u64 giveups = 0;
  for (u64 s = (u64)blockIdx.x * C_BLOCK + threadIdx.x; s < f.M; s += stride) {
    uint32_t r = (uint32_t)s, steps = 0;
    if (!find(f.parent, r, steps)) {
      ++giveups;
      r = (uint32_t)s;
    }
    f.root[s] = r;  // (<= s)
    f.size[s] = 0;
  }
  if (giveups) atomicAdd(&f.counts[3], giveups);
}

__global__ __launch_bounds__(C_BLOCK) void components_finish_sizes(Finish f) {
  const u64 stride = (u64)gridDim.x * C_BLOCK;
  for (u64 s = (u64)blockIdx.x * C_BLOCK + threadIdx.x; s < f.M; s += stride) atomicAdd(&f.size[f.root[s]], 1u);
}

__global__ __launch_bounds__(C_BLOCK) void components_finish_slots(Finish f) {
  const u64 stride = (u64)gridDim.x * C_BLOCK;
  for (u64 s = (u64)blockIdx.x * C_BLOCK + threadIdx.x; s < f.M; s += stride) {
    const uint32_t r = f.root[s];  // the root slot; a root slot's own entry stays a slot until its own thread is here
    const uint32_t sz = f.size[r];  // (only non-root slots' entries are written in this launch)
    const uint32_t node = f.slot_node[r];
    if (r == s) {
      const uint32_t k = f.slot_comm[s];
      if (k < f.K) {
        atomicAdd(&f.members[k], (u64)sz);
        atomicAdd(&f.components[k], 1ull);
        if (sz == 1u) atomicAdd(&f.singletons[k], 1ull);
        const u64 cand = ((u64)sz << 32) | (u64)(0xFFFFFFFFu - node);
        // (best only grows, so an older value can only let an atomic through that changes nothing)
        if (__hip_atomic_load(&f.best[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < cand) atomicMax(&f.best[k], cand);
      }
    } else {
      f.size[s] = sz;
    }
    f.root[s] = node;
  }
}

__global__ __launch_bounds__(C_BLOCK) void components_finish_best(Finish f) {
  const uint32_t k = blockIdx.x * C_BLOCK + threadIdx.x;
  if (k >= f.K) return;
  const u64 b = f.best[k];
  f.largest[k] = (uint32_t)(b >> 32);
  f.largest_root[k] = b ? (int32_t)(0xFFFFFFFFu - (uint32_t)b) : -1;  // (a root is a node id < 2^32 - 1 wherever M > 0)
}

// a group of lanes per node (of the size the other passes use: a node has at most 64 slots per lane)
__global__ __launch_bounds__(C_BLOCK) void components_finish_stray(Finish f) {
  const int lane = threadIdx.x & 63;
  const uint32_t G = 1u << f.gshift, gl = lane & (G - 1u), slot = lane >> f.gshift, epw = 64u >> f.gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  for (uint64_t rb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw; rb < f.rows; rb += stride) {
    const uint64_t r = rb + slot;
    uint32_t n = 0;
    if (r < f.rows) {
      u64 lo = f.base[r], hi = f.base[r + 1];
      hi = hi < f.M ? hi : f.M;
      for (u64 s = lo + gl; s < hi; s += G) {
        const uint32_t k = f.slot_comm[s];
        n += (k < f.K && f.root[s] != 0xFFFFFFFFu - (uint32_t)f.best[k]) ? 1u : 0u;
      }
    }
    n = group_sum(n, G);
    if (r < f.rows && gl == 0) f.stray[r] = n;
  }
}

// ------------------------------------------------------------------------------------------ host

const char* check_shape(uint64_t num_rows, uint32_t K, uint64_t num_slots) {
  if (K == 0 || K > AMMSB_COMPONENTS_MAX_COLS) return "num_cols outside 1..8192";
  if (num_rows >> 32) return "2^32 rows or more";
  if (num_slots >= AMMSB_COMPONENTS_MAX_SLOTS) return "2^32 slots or more";
  return nullptr;
}

uint32_t group_shift(uint32_t num_cols) {
  const uint32_t W = (num_cols + 63u) / 64u;
  uint32_t g = 0;
  while ((1u << g) < W && g < 6) ++g;
  return g;
}

void shape(Args* a, const uint64_t* mask, uint64_t num_rows, uint32_t num_cols) {
  *a = Args();
  a->mask = reinterpret_cast<const u64*>(mask);
  a->rows = (uint32_t)num_rows;
  a->K = num_cols;
  a->W = (num_cols + 63u) / 64u;
  a->gshift = group_shift(num_cols);
}

// blocks of a grid of groups over n items
unsigned group_grid(uint64_t n, uint32_t num_cols, uint32_t gshift) {
  const uint64_t epw = num_cols <= AMMSB_COMPONENTS_W1_MAX_COLS ? (64u >> gshift) : 1u;
  return persistent_grid(n, (uint64_t)C_WAVES * epw * C_TRIPS);
}

#define REQUIRE(ptr, bytes)                                                    \
  do {                                                                         \
    if (!(ptr)) return fail(AMMSB_EINVAL, #ptr " is NULL");                    \
    if (misaligned(ptr, bytes)) return fail(AMMSB_EINVAL, #ptr " is not " #bytes "-byte aligned"); \
  } while (0)

}  // namespace

extern "C" const char* ammsb_components_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_components_last_error(void) { return g_last_error; }

extern "C" int ammsb_components_own(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, uint32_t* own, void* stream) {
  if (const char* bad = check_shape(num_rows, num_cols, 0)) return fail(AMMSB_EINVAL, bad);
  if (num_rows == 0) return AMMSB_OK;
  REQUIRE(mask, 8);
  REQUIRE(own, 4);
  Args a;
  shape(&a, mask, num_rows, num_cols);
  a.own = own;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(group_grid(num_rows, num_cols, a.gshift)), block(C_BLOCK);
  if (num_cols <= AMMSB_COMPONENTS_W1_MAX_COLS) {
    hipLaunchKernelGGL(components_own_w1, grid, block, 0, s, a);
    return launched("components_own_w1");
  }
  hipLaunchKernelGGL(components_own_w2, grid, block, 0, s, a);
  return launched("components_own_w2");
}

extern "C" int ammsb_components_slots(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                                      uint64_t num_slots, uint64_t first_row, uint64_t n_rows, uint32_t* slot_node,
                                      uint16_t* slot_comm, uint32_t* parent, void* stream) {
  if (const char* bad = check_shape(num_rows, num_cols, num_slots)) return fail(AMMSB_EINVAL, bad);
  if (first_row > num_rows || n_rows > num_rows - first_row) return fail(AMMSB_EINVAL, "the node range is not inside num_rows");
  if (n_rows == 0) return AMMSB_OK;
  REQUIRE(mask, 8);
  REQUIRE(base, 8);
  REQUIRE(slot_node, 4);
  REQUIRE(slot_comm, 2);
  REQUIRE(parent, 4);
  Args a;
  shape(&a, mask, num_rows, num_cols);
  a.base = reinterpret_cast<const u64*>(base);
  a.M = num_slots;
  a.first = first_row;
  a.n = n_rows;
  a.slot_node = slot_node;
  a.slot_comm = slot_comm;
  a.parent = parent;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(group_grid(n_rows, num_cols, a.gshift)), block(C_BLOCK);
  if (num_cols <= AMMSB_COMPONENTS_W1_MAX_COLS) {
    hipLaunchKernelGGL(components_slots_w1, grid, block, 0, s, a);
    return launched("components_slots_w1");
  }
  hipLaunchKernelGGL(components_slots_w2, grid, block, 0, s, a);
  return launched("components_slots_w2");
}

extern "C" int ammsb_components_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                                      uint64_t num_slots, const uint64_t* edges, uint64_t n, uint32_t* parent,
                                      uint64_t* counts, void* stream) {
  if (const char* bad = check_shape(num_rows, num_cols, num_slots)) return fail(AMMSB_EINVAL, bad);
  if (n >= AMMSB_COMPONENTS_MAX_EDGES) return fail(AMMSB_EINVAL, "2^31 edges or more");
  REQUIRE(counts, 8);
  if (n == 0) return AMMSB_OK;
  REQUIRE(edges, 8);
  if (num_rows > 0) {  // (without a node no key is valid and nothing but the keys is read)
    REQUIRE(mask, 8);
    REQUIRE(base, 8);
  }
  if (num_slots > 0) REQUIRE(parent, 4);
  Args a;
  shape(&a, mask, num_rows, num_cols);
  a.base = reinterpret_cast<const u64*>(base);
  a.M = num_slots;
  a.edges = reinterpret_cast<const u64*>(edges);
  a.n = n;
  a.parent = parent;
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(group_grid(n, num_cols, a.gshift)), block(C_BLOCK);
  if (num_cols <= AMMSB_COMPONENTS_W1_MAX_COLS) {
    hipLaunchKernelGGL(components_edges_w1, grid, block, 0, s, a);
    return launched("components_edges_w1");
  }
  hipLaunchKernelGGL(components_edges_w2, grid, block, 0, s, a);
  return launched("components_edges_w2");
}

extern "C" int ammsb_components_finish(uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                                       const uint32_t* slot_node, const uint16_t* slot_comm, uint32_t* parent, uint32_t* root,
                                       uint32_t* size, uint64_t* members, uint64_t* components, uint64_t* singletons,
                                       uint64_t* best, uint32_t* largest, int32_t* largest_root, uint32_t* stray,
                                       uint64_t* counts, void* stream) {
  if (const char* bad = check_shape(num_rows, num_cols, num_slots)) return fail(AMMSB_EINVAL, bad);
  REQUIRE(members, 8);
  REQUIRE(components, 8);
  REQUIRE(singletons, 8);
  REQUIRE(best, 8);
  REQUIRE(largest, 4);
  REQUIRE(largest_root, 4);
  REQUIRE(counts, 8);
  if (num_rows > 0) {
    REQUIRE(base, 8);
    REQUIRE(stray, 4);
  }
  if (num_slots > 0) {
    if (num_rows == 0) return fail(AMMSB_EINVAL, "slots without a node");
    REQUIRE(slot_node, 4);
    REQUIRE(slot_comm, 2);
    REQUIRE(parent, 4);
    REQUIRE(root, 4);
    REQUIRE(size, 4);
  }
  Finish f;
  f.rows = (uint32_t)num_rows;
  f.K = num_cols;
  f.gshift = num_cols <= AMMSB_COMPONENTS_W1_MAX_COLS ? group_shift(num_cols) : 6u;
  f.base = reinterpret_cast<const u64*>(base);
  f.M = num_slots;
  f.slot_node = slot_node;
  f.slot_comm = slot_comm;
  f.parent = parent;
  f.root = root;
  f.size = size;
  f.members = reinterpret_cast<u64*>(members);
  f.components = reinterpret_cast<u64*>(components);
  f.singletons = reinterpret_cast<u64*>(singletons);
  f.best = reinterpret_cast<u64*>(best);
  f.largest = largest;
  f.largest_root = largest_root;
  f.stray = stray;
  f.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(C_BLOCK);
  if (num_slots > 0) {
    const dim3 grid(persistent_grid(num_slots, (uint64_t)C_BLOCK * C_TRIPS));
    hipLaunchKernelGGL(components_finish_roots, grid, block, 0, s, f);
    if (int rc = launched("components_finish_roots")) return rc;
    hipLaunchKernelGGL(components_finish_sizes, grid, block, 0, s, f);
    if (int rc = launched("components_finish_sizes")) return rc;
    hipLaunchKernelGGL(components_finish_slots, grid, block, 0, s, f);
    if (int rc = launched("components_finish_slots")) return rc;
  }
  hipLaunchKernelGGL(components_finish_best, dim3((num_cols + C_BLOCK - 1) / C_BLOCK), block, 0, s, f);
  if (int rc = launched("components_finish_best")) return rc;
  if (num_rows == 0) return AMMSB_OK;
  hipLaunchKernelGGL(components_finish_stray, dim3(persistent_grid(num_rows, (uint64_t)C_WAVES * (64u >> f.gshift) * C_TRIPS)),
                     block, 0, s, f);
  return launched("components_finish_stray");
}
