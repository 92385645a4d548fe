// libammsb_cores.so (include/ammsb_cores.h): the k-core decomposition of the subgraph every detected community induces in a
// simple CSR adjacency, over the slot numbering of ammsb_components.h.
//
//   cores_degrees_w1 / _w2     a group of lanes per node (the smallest power of two >= W; a wave with two words per lane
//                              above K = 4096).  The exclusive prefix sum of the words' population counts by shuffles gives
//                              the slot of a word's first bit.  A walk of the node's row handles up to WALK = 4 bits of
//                              every lane's word in registers (a lane of a sparse cover has one or two), so a group walks
//                              the row ceil(most bits in a word / 4) times; the next target's words are requested before
//                              this target's are used.
//   cores_adjacency_w1 / _w2   the same walks; per target the prefix sum over the target's row gives base[b] + the bits of
//                              b below k.  The fill order is the row order: a register cursor per bit, no atomics.
//   cores_scan                 all slots: deg == level -> the queue (one atomic per wave), min of the deg > level.
//   cores_peel                 16 lanes per queued slot read its row of nbr side by side and lower the neighbours.
//   cores_finish_*             two launches (the header lists them).
//
// Nothing here waits: no lane polls a queue, spins on a flag or meets a grid-wide barrier.  The one retry loop is the
// compare-and-swap of lower(), which continues from the value the atomic returned and ends when that value is <= level;
// each failed swap is another lane's successful decrement of the same word, so it is bounded by the slot's degree.
//
// The mask is read through mask_word() of ammsb_postfit.h alone (bits past K cleared).  base, offsets, targets, nbr_off
// and nbr are public buffers: no slot >= num_slots, target >= num_rows, entry >= num_nbr or community >= K is used as an
// index.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_cores.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int C_WAVES = 4;  // waves per block
constexpr int C_BLOCK = 64 * C_WAVES;
constexpr int C_TRIPS = 2;  // items a group takes before another block is worth it
constexpr int WALK = 4;     // bits of a word that one walk of the row keeps in registers
constexpr uint32_t PEEL_LANES = AMMSB_CORES_PEEL_LANES;
constexpr uint32_t NONE = 0xFFFFFFFFu;

struct Build {
  const u64* mask;
  uint32_t rows, K, W;
  uint32_t gshift;  // w1: log2 of the lanes that own a node, the smallest power of two >= W
  const u64* base;
  u64 M;
  const u64* offsets;
  const uint32_t* targets;
  uint64_t first, n;  // the node range
  uint32_t* indeg;    // degrees: written; adjacency: read
  const u64* nbr_off;
  u64 num_nbr;
  uint32_t* nbr;
  u64* counts;
};

struct Peel {
  u64 M;
  uint32_t level;
  u64 head, tail_now;
  const u64* nbr_off;
  const uint32_t* indeg;
  const uint32_t* nbr;
  u64 num_nbr;
  uint32_t* deg;
  uint32_t* queue;
  u64* tail;
  uint32_t* next_level;
  u64* counts;
};

struct Finish {
  uint32_t rows, K, gshift;
  const u64* base;
  u64 M;
  const uint16_t* slot_comm;
  const uint32_t* indeg;
  const uint32_t* core;
  u64 *members, *inlinks2, *nucleus, *isolated;
  uint32_t* degeneracy;
  uint32_t* best_core;
  int32_t* best_comm;
  uint32_t* in_nucleus;
};

// the sum / the maximum of v over the lanes of a group of G
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t G) {
  for (uint32_t o = G >> 1; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o, 64);  // o < G: stays inside the group
  return v;
}

__device__ __forceinline__ uint32_t group_max(uint32_t v, uint32_t G) {
  for (uint32_t o = G >> 1; o > 0; o >>= 1) {
    const uint32_t t = (uint32_t)__shfl_xor((int)v, (int)o, 64);
    v = t > v ? t : v;
  }
  return v;
}

__device__ __forceinline__ u64 group_max_u64(u64 v, uint32_t G) {
  for (uint32_t o = G >> 1; o > 0; o >>= 1) {
    const u64 t = __shfl_xor(v, (int)o, 64);
    v = t > v ? t : v;
  }
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

// ------------------------------------------------------------------------------------------ degrees, adjacency
// target j of a row and the lane's words of its mask row (zeros past the row's end or for a target that is no node)
template <int WPL>
struct Target {
  uint32_t b;
  bool ok;
  u64 y[WPL];
};

template <int WPL>
__device__ __forceinline__ void fetch(const Build& a, u64 j, u64 hi, uint32_t gl, Target<WPL>& t) {
  t.b = j < hi ? a.targets[j] : NONE;
  t.ok = j < hi && t.b < a.rows;
#pragma unroll
  for (int i = 0; i < WPL; ++i) t.y[i] = t.ok ? mask_word(a, t.b, gl + 64u * i) : 0ull;
}

// The lanes of a group walk their node's row together (the trip counts below are the same in every lane of a group; the
// groups of a wave differ, and the shuffles only read inside the group).
template <int WPL, bool FILL>
__device__ __forceinline__ void build_body(const Build& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  u64 slots = 0, links = 0;  // of this lane's bits
  for (uint64_t rb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw; rb < a.n; rb += stride) {
    const bool have = rb + slot < a.n;
    const uint32_t r = (uint32_t)(a.first + rb + slot);  // (< rows < 2^32 where have)
    u64 rest[WPL], s0[WPL];  // the bits of the lane's words no walk has handled yet; the slot of each word's first bit
    uint32_t before = 0, most = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      rest[i] = have ? mask_word(a, r, gl + 64u * i) : 0ull;
      const uint32_t c = (uint32_t)__popcll(rest[i]);
      const uint32_t ex = group_before(c, G, gl);
      s0[i] = (have ? a.base[r] : 0ull) + before + ex;
      if (i + 1 < WPL) before += (uint32_t)__shfl((int)(ex + c), 63, 64);  // (WPL == 2: G == 64, the last lane holds the total)
      most = c > most ? c : most;
    }
    most = group_max(most, G);
    u64 lo = have ? a.offsets[r] : 0ull, hi = have ? a.offsets[r + 1] : 0ull;
    hi = hi > lo ? hi : lo;  // (offsets that do not ascend: an empty row)
    for (uint32_t done = 0; done < most; done += WALK) {
      u64 m[WPL][WALK];         // the bit each register stands for, 0: none
      uint32_t cnt[WPL][WALK];  // its neighbours so far
      u64 at[WPL][WALK];        // FILL: where its row of nbr starts
      uint32_t room[WPL][WALK];  // FILL: the entries its row has
#pragma unroll
      for (int i = 0; i < WPL; ++i)
#pragma unroll
        for (int q = 0; q < WALK; ++q) {
          m[i][q] = rest[i] & (0ull - rest[i]);
          rest[i] ^= m[i][q];
          cnt[i][q] = 0;
          at[i][q] = 0;
          room[i][q] = 0;
          const u64 s = s0[i] + done + q;
          if (FILL && m[i][q] && s < a.M) {
            at[i][q] = a.nbr_off[s];
            room[i][q] = a.indeg[s];
          }
        }
      Target<WPL> nx;
      fetch<WPL>(a, lo, hi, gl, nx);
      for (u64 j = lo; j < hi; ++j) {
        const Target<WPL> t = nx;
        fetch<WPL>(a, j + 1, hi, gl, nx);  // on its way while this target is counted
        uint32_t tbefore = 0;               // FILL: the bits of b's row in the words before the lane's word i
#pragma unroll
        for (int i = 0; i < WPL; ++i) {
          u64 tb0 = 0;
          if (FILL) {
            const uint32_t c = (uint32_t)__popcll(t.y[i]);
            const uint32_t ex = group_before(c, G, gl);
            tb0 = (t.ok ? a.base[t.b] : 0ull) + tbefore + ex;
            if (i + 1 < WPL) tbefore += (uint32_t)__shfl((int)(ex + c), 63, 64);
          }
#pragma unroll
          for (int q = 0; q < WALK; ++q) {
            if (t.y[i] & m[i][q]) {
              if (FILL) {
                const u64 ts = tb0 + (u64)__popcll(t.y[i] & (m[i][q] - 1ull));
                const u64 e = at[i][q] + cnt[i][q];
                if (cnt[i][q] < room[i][q] && e < a.num_nbr && ts < a.M) a.nbr[e] = (uint32_t)ts;
              }
              ++cnt[i][q];
            }
          }
        }
      }
      if (!FILL) {
#pragma unroll
        for (int i = 0; i < WPL; ++i)
#pragma unroll
          for (int q = 0; q < WALK; ++q) {
            const u64 s = s0[i] + done + q;
            if (m[i][q] && s < a.M) {
              a.indeg[s] = cnt[i][q];
              ++slots;
              links += cnt[i][q];
            }
          }
      }
    }
  }
  if (!FILL) {
    slots = wave_sum_u64(slots);
    links = wave_sum_u64(links);
    if (lane == 0) {
      if (slots) atomicAdd(&a.counts[0], slots);
      if (links) atomicAdd(&a.counts[1], links);
    }
  }
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(C_BLOCK) void cores_degrees_w1(Build a) { build_body<1, false>(a); }
__global__ __launch_bounds__(C_BLOCK) void cores_degrees_w2(Build a) { build_body<2, false>(a); }
__global__ __launch_bounds__(C_BLOCK) void cores_adjacency_w1(Build a) { build_body<1, true>(a); }
__global__ __launch_bounds__(C_BLOCK) void cores_adjacency_w2(Build a) { build_body<2, true>(a); }

// ------------------------------------------------------------------------------------------ the peel
__device__ __forceinline__ void append(const Peel& p, uint32_t s) {
  const u64 pos = atomicAdd(p.tail, 1ull);
  if (pos < p.M) p.queue[pos] = s;  // (every slot is appended once, so pos < M; a tail that is not this queue's is not followed)
}

__global__ __launch_bounds__(C_BLOCK) void cores_scan(Peel p) {
  const int lane = threadIdx.x & 63;
  const u64 stride = (u64)gridDim.x * C_BLOCK;
  uint32_t low = NONE;  // the smallest deg > level this lane saw
  // (the bound is wave-uniform, so that the ballot below meets all 64 lanes)
  for (u64 sb = (u64)blockIdx.x * C_BLOCK + (threadIdx.x & ~63u); sb < p.M; sb += stride) {
    const u64 s = sb + lane;
    const uint32_t d = s < p.M ? p.deg[s] : NONE;
    const bool leaves = s < p.M && d == p.level;
    if (s < p.M && d > p.level && d < low) low = d;
    const u64 who = __ballot(leaves);
    if (who) {  // one atomic per wave: the first lane takes the places of all
      u64 pos0 = 0;
      const int first = __builtin_ctzll(who);
      if (lane == first) pos0 = atomicAdd(p.tail, (u64)__popcll(who));
      pos0 = __shfl(pos0, first, 64);
      const u64 pos = pos0 + (u64)__popcll(who & ((1ull << lane) - 1ull));
      if (leaves && pos < p.M) p.queue[pos] = (uint32_t)s;
    }
  }
  for (int o = 32; o > 0; o >>= 1) {  // the wave's minimum
    const uint32_t t = (uint32_t)__shfl_xor((int)low, o, 64);
    low = t < low ? t : low;
  }
  if (lane == 0 && low != NONE) atomicMin(p.next_level, low);
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&p.counts[2], 1ull);
}

// deg[t] > level: one less, and the lane that takes it to `level` appends t.  Starts from a load that may be stale (never
// below the true value: deg only decreases) and goes on from what the atomic returned.
__device__ __forceinline__ void lower(const Peel& p, uint32_t t) {
  uint32_t d = __hip_atomic_load(&p.deg[t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (d > p.level) {
    uint32_t seen = d;
    if (__hip_atomic_compare_exchange_strong(&p.deg[t], &seen, d - 1u, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_AGENT)) {
      if (d - 1u == p.level) append(p, t);
      return;
    }
    if (seen >= d) return;  // (no state this library makes: a word that grew)
    d = seen;
  }
}

__global__ __launch_bounds__(C_BLOCK) void cores_peel(Peel p) {
  const uint32_t gl = threadIdx.x & (PEEL_LANES - 1u);
  const u64 per_block = C_BLOCK / PEEL_LANES, stride = (u64)gridDim.x * per_block;
  for (u64 i = p.head + (u64)blockIdx.x * per_block + threadIdx.x / PEEL_LANES; i < p.tail_now; i += stride) {
    const uint32_t s = p.queue[i];
    if (s >= p.M) continue;
    const u64 lo = p.nbr_off[s];
    const uint32_t len = p.indeg[s];
    for (u64 j = gl; j < len; j += PEEL_LANES) {
      if (lo + j >= p.num_nbr) break;
      const uint32_t t = p.nbr[lo + j];
      if (t < p.M) lower(p, t);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&p.counts[3], 1ull);
}

// ------------------------------------------------------------------------------------------ finish
__global__ __launch_bounds__(C_BLOCK) void cores_finish_communities(Finish f) {
  const u64 stride = (u64)gridDim.x * C_BLOCK;
  for (u64 s = (u64)blockIdx.x * C_BLOCK + threadIdx.x; s < f.M; s += stride) {
    const uint32_t k = f.slot_comm[s];
    if (k >= f.K) continue;
    const uint32_t c = f.core[s], d = f.indeg[s];
    atomicAdd(&f.members[k], 1ull);
    if (d) atomicAdd(&f.inlinks2[k], (u64)d);
    if (c == 0) atomicAdd(&f.isolated[k], 1ull);
    // (degeneracy only grows, so an older value can only let an atomic through that changes nothing)
    if (__hip_atomic_load(&f.degeneracy[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < c) atomicMax(&f.degeneracy[k], c);
  }
}

// a group of lanes per node (of the size the build passes use: a node has at most 64 slots per lane)
__global__ __launch_bounds__(C_BLOCK) void cores_finish_nodes(Finish f) {
  const int lane = threadIdx.x & 63;
  const uint32_t G = 1u << f.gshift, gl = lane & (G - 1u), slot = lane >> f.gshift, epw = 64u >> f.gshift;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES * epw;
  for (uint64_t rb = ((uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6)) * epw; rb < f.rows; rb += stride) {
    const uint64_t r = rb + slot;
    u64 best = 0;  // (core << 32) | (0xFFFFFFFF - k): the largest core, the lowest community among equals; 0: no slot
    uint32_t inner = 0;
    if (r < f.rows) {
      u64 lo = f.base[r], hi = f.base[r + 1];
      hi = hi < f.M ? hi : f.M;
      for (u64 s = lo + gl; s < hi; s += G) {
        const uint32_t k = f.slot_comm[s];
        if (k >= f.K) continue;
        const uint32_t c = f.core[s], top = f.degeneracy[k];
        const u64 cand = ((u64)c << 32) | (u64)(NONE - k);
        best = cand > best ? cand : best;
        if (c == top) {
          atomicAdd(&f.nucleus[k], 1ull);
          inner += top > 0 ? 1u : 0u;
        }
      }
    }
    best = group_max_u64(best, G);
    inner = group_sum(inner, G);
    if (r < f.rows && gl == 0) {
      f.best_core[r] = (uint32_t)(best >> 32);
      f.best_comm[r] = best ? (int32_t)(NONE - (uint32_t)best) : -1;  // (k < 8192: the low half of a slot's word is never 0)
      f.in_nucleus[r] = inner;
    }
  }
}

// ------------------------------------------------------------------------------------------ host
const char* check_shape(uint64_t num_rows, uint32_t K, uint64_t num_slots) {
  if (K == 0 || K > AMMSB_CORES_MAX_COLS) return "num_cols outside 1..8192";
  if (num_rows >> 32) return "2^32 rows or more";
  if (num_slots >= AMMSB_CORES_MAX_SLOTS) return "2^32 slots or more";
  return nullptr;
}

uint32_t group_shift(uint32_t num_cols) {
  const uint32_t W = (num_cols + 63u) / 64u;
  uint32_t g = 0;
  while ((1u << g) < W && g < 6) ++g;
  return g;
}

// blocks of a grid of groups over n nodes
unsigned group_grid(uint64_t n, uint32_t num_cols, uint32_t gshift) {
  const uint64_t epw = num_cols <= AMMSB_CORES_W1_MAX_COLS ? (64u >> gshift) : 1u;
  return persistent_grid(n, (uint64_t)C_WAVES * epw * C_TRIPS);
}

#define REQUIRE(ptr, bytes)                                                    \
  do {                                                                         \
    if (!(ptr)) return fail(AMMSB_EINVAL, #ptr " is NULL");                    \
    if (misaligned(ptr, bytes)) return fail(AMMSB_EINVAL, #ptr " is not " #bytes "-byte aligned"); \
  } while (0)

// what degrees and adjacency share: the checks, the argument struct; AMMSB_OK with *go = false: a valid no-op
int build_args(Build* a, bool* go, const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
               uint64_t num_slots, const uint64_t* offsets, const uint32_t* targets, uint64_t first_row, uint64_t n_rows) {
  *go = false;
  if (const char* bad = check_shape(num_rows, num_cols, num_slots)) return fail(AMMSB_EINVAL, bad);
  if (first_row > num_rows || n_rows > num_rows - first_row) return fail(AMMSB_EINVAL, "the node range is not inside num_rows");
  if (n_rows == 0) return AMMSB_OK;
  REQUIRE(mask, 8);
  REQUIRE(base, 8);
  REQUIRE(offsets, 8);
  REQUIRE(targets, 4);
  *a = Build();
  a->mask = reinterpret_cast<const u64*>(mask);
  a->rows = (uint32_t)num_rows;
  a->K = num_cols;
  a->W = (num_cols + 63u) / 64u;
  a->gshift = group_shift(num_cols);
  a->base = reinterpret_cast<const u64*>(base);
  a->M = num_slots;
  a->offsets = reinterpret_cast<const u64*>(offsets);
  a->targets = targets;
  a->first = first_row;
  a->n = n_rows;
  *go = true;
  return AMMSB_OK;
}

}  // namespace

extern "C" const char* ammsb_cores_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_cores_last_error(void) { return g_last_error; }

extern "C" int ammsb_cores_degrees(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                                   uint64_t num_slots, const uint64_t* offsets, const uint32_t* targets, uint64_t first_row,
                                   uint64_t n_rows, uint32_t* indeg, uint64_t* counts, void* stream) {
  Build a;
  bool go;
  if (int rc = build_args(&a, &go, mask, num_rows, num_cols, base, num_slots, offsets, targets, first_row, n_rows)) return rc;
  if (!go || num_slots == 0) return AMMSB_OK;
  REQUIRE(indeg, 4);
  REQUIRE(counts, 8);
  a.indeg = indeg;
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(group_grid(n_rows, num_cols, a.gshift)), block(C_BLOCK);
  if (num_cols <= AMMSB_CORES_W1_MAX_COLS) {
    hipLaunchKernelGGL(cores_degrees_w1, grid, block, 0, s, a);
    return launched("cores_degrees_w1");
  }
  hipLaunchKernelGGL(cores_degrees_w2, grid, block, 0, s, a);
  return launched("cores_degrees_w2");
}

extern "C" int ammsb_cores_adjacency(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* base,
                                     uint64_t num_slots, const uint64_t* offsets, const uint32_t* targets, uint64_t first_row,
                                     uint64_t n_rows, const uint32_t* indeg, const uint64_t* nbr_off, uint64_t num_nbr,
                                     uint32_t* nbr, void* stream) {
  Build a;
  bool go;
  if (int rc = build_args(&a, &go, mask, num_rows, num_cols, base, num_slots, offsets, targets, first_row, n_rows)) return rc;
  if (num_nbr >= AMMSB_CORES_MAX_NBR) return fail(AMMSB_EINVAL, "2^32 entries of nbr or more");
  if (!go || num_slots == 0 || num_nbr == 0) return AMMSB_OK;
  REQUIRE(indeg, 4);
  REQUIRE(nbr_off, 8);
  REQUIRE(nbr, 4);
  a.indeg = const_cast<uint32_t*>(indeg);  // (read only in this pass)
  a.nbr_off = reinterpret_cast<const u64*>(nbr_off);
  a.num_nbr = num_nbr;
  a.nbr = nbr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(group_grid(n_rows, num_cols, a.gshift)), block(C_BLOCK);
  if (num_cols <= AMMSB_CORES_W1_MAX_COLS) {
    hipLaunchKernelGGL(cores_adjacency_w1, grid, block, 0, s, a);
    return launched("cores_adjacency_w1");
  }
  hipLaunchKernelGGL(cores_adjacency_w2, grid, block, 0, s, a);
  return launched("cores_adjacency_w2");
}

extern "C" int ammsb_cores_scan(uint64_t num_slots, uint32_t level, const uint32_t* deg, uint32_t* queue, uint64_t* tail,
                                uint32_t* next_level, uint64_t* counts, void* stream) {
  if (num_slots >= AMMSB_CORES_MAX_SLOTS) return fail(AMMSB_EINVAL, "2^32 slots or more");
  REQUIRE(tail, 8);
  REQUIRE(next_level, 4);
  REQUIRE(counts, 8);
  if (num_slots == 0) return AMMSB_OK;
  REQUIRE(deg, 4);
  REQUIRE(queue, 4);
  Peel p = Peel();
  p.M = num_slots;
  p.level = level;
  p.deg = const_cast<uint32_t*>(deg);  // (read only in this pass)
  p.queue = queue;
  p.tail = reinterpret_cast<u64*>(tail);
  p.next_level = next_level;
  p.counts = reinterpret_cast<u64*>(counts);
  hipLaunchKernelGGL(cores_scan, dim3(persistent_grid(num_slots, (uint64_t)C_BLOCK * C_TRIPS)), dim3(C_BLOCK), 0,
                     static_cast<hipStream_t>(stream), p);
  return launched("cores_scan");
}

extern "C" int ammsb_cores_peel(uint64_t num_slots, uint32_t level, uint64_t head, uint64_t tail_now, const uint64_t* nbr_off,
                                const uint32_t* indeg, const uint32_t* nbr, uint64_t num_nbr, uint32_t* deg, uint32_t* queue,
                                uint64_t* tail, uint64_t* counts, void* stream) {
  if (num_slots >= AMMSB_CORES_MAX_SLOTS) return fail(AMMSB_EINVAL, "2^32 slots or more");
  if (num_nbr >= AMMSB_CORES_MAX_NBR) return fail(AMMSB_EINVAL, "2^32 entries of nbr or more");
  if (head > tail_now || tail_now > num_slots) return fail(AMMSB_EINVAL, "head .. tail is not inside the queue");
  REQUIRE(tail, 8);
  REQUIRE(counts, 8);
  if (head == tail_now) return AMMSB_OK;
  REQUIRE(nbr_off, 8);
  REQUIRE(indeg, 4);
  REQUIRE(deg, 4);
  REQUIRE(queue, 4);
  if (num_nbr > 0) REQUIRE(nbr, 4);
  Peel p = Peel();
  p.M = num_slots;
  p.level = level;
  p.head = head;
  p.tail_now = tail_now;
  p.nbr_off = reinterpret_cast<const u64*>(nbr_off);
  p.indeg = indeg;
  p.nbr = nbr;
  p.num_nbr = num_nbr;
  p.deg = deg;
  p.queue = queue;
  p.tail = reinterpret_cast<u64*>(tail);
  p.counts = reinterpret_cast<u64*>(counts);
  hipLaunchKernelGGL(cores_peel, dim3(persistent_grid(tail_now - head, (uint64_t)(C_BLOCK / PEEL_LANES) * C_TRIPS)),
                     dim3(C_BLOCK), 0, static_cast<hipStream_t>(stream), p);
  return launched("cores_peel");
}

extern "C" int ammsb_cores_finish(uint64_t num_rows, uint32_t num_cols, const uint64_t* base, uint64_t num_slots,
                                  const uint16_t* slot_comm, const uint32_t* indeg, const uint32_t* core, uint64_t* members,
                                  uint64_t* inlinks2, uint32_t* degeneracy, uint64_t* nucleus, uint64_t* isolated,
                                  uint32_t* best_core, int32_t* best_comm, uint32_t* in_nucleus, void* stream) {
  if (const char* bad = check_shape(num_rows, num_cols, num_slots)) return fail(AMMSB_EINVAL, bad);
  REQUIRE(members, 8);
  REQUIRE(inlinks2, 8);
  REQUIRE(degeneracy, 4);
  REQUIRE(nucleus, 8);
  REQUIRE(isolated, 8);
  if (num_rows > 0) {
    REQUIRE(base, 8);
    REQUIRE(best_core, 4);
    REQUIRE(best_comm, 4);
    REQUIRE(in_nucleus, 4);
  }
  if (num_slots > 0) {
    if (num_rows == 0) return fail(AMMSB_EINVAL, "slots without a node");
    REQUIRE(slot_comm, 2);
    REQUIRE(indeg, 4);
    REQUIRE(core, 4);
  }
  if (num_rows == 0) return AMMSB_OK;
  Finish f = Finish();
  f.rows = (uint32_t)num_rows;
  f.K = num_cols;
  f.gshift = num_cols <= AMMSB_CORES_W1_MAX_COLS ? group_shift(num_cols) : 6u;
  f.base = reinterpret_cast<const u64*>(base);
  f.M = num_slots;
  f.slot_comm = slot_comm;
  f.indeg = indeg;
  f.core = core;
  f.members = reinterpret_cast<u64*>(members);
  f.inlinks2 = reinterpret_cast<u64*>(inlinks2);
  f.degeneracy = degeneracy;
  f.nucleus = reinterpret_cast<u64*>(nucleus);
  f.isolated = reinterpret_cast<u64*>(isolated);
  f.best_core = best_core;
  f.best_comm = best_comm;
  f.in_nucleus = in_nucleus;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(C_BLOCK);
  if (num_slots > 0) {
    hipLaunchKernelGGL(cores_finish_communities, dim3(persistent_grid(num_slots, (uint64_t)C_BLOCK * C_TRIPS)), block, 0, s, f);
    if (int rc = launched("cores_finish_communities")) return rc;
  }
  hipLaunchKernelGGL(cores_finish_nodes, dim3(persistent_grid(num_rows, (uint64_t)C_WAVES * (64u >> f.gshift) * C_TRIPS)), block, 0,
                     s, f);
  return launched("cores_finish_nodes");
}
