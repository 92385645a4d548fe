// libammsb_modularity.so (include/ammsb_modularity.h): the integer sums of the overlapping modularity of the detected cover
// against an edge list, in 2^-62 fixed point in 128 bits.
//
//   modularity_edges_w1 / _w2   the edge pass of ammsb_quality.hip with other work per edge: a group of lanes (the smallest
//                               power of two >= W; a wave with two words per lane above K = 4096) owns an edge over a
//                               persistent grid and requests the next edge's words before this one's atomics.  The group
//                               sums the population counts of both rows by shuffles; a lane whose two words share a bit
//                               divides 2^62 by O_a O_b and adds the quotient to IN[k] for every bit of the AND; the
//                               group's first lane adds 1 to the degree of both ends.  Bounded by the atomics: one or two
//                               64-bit atomics per community that holds both ends, two 32-bit atomics per edge.
//   modularity_nodes_w1 / _w2   a group of lanes per node with deg > 0: O_a, one division, the 96-bit product deg floor(2^62
//                               / O_a), one 128-bit add per set bit.  Bounded by the atomics as well: one per membership.
//
// A 128-bit add is an atomic add of the low part that returns the old low word, and an atomic add of the high part plus
// the carry (old + low wrapped) where that is not zero.  The low word goes through one sequence of adds whatever their
// order, so the carries sum to the number of times it wrapped.
//
// The mask is read through mask_word() of ammsb_postfit.h alone (bits past K cleared).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_modularity.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int M_WAVES = 4;  // waves per block
constexpr int M_BLOCK = 64 * M_WAVES;
constexpr int M_TRIPS = 2;  // items a group takes before another block is worth it: the second trip's loads are in flight
constexpr u64 FRAC = 1ull << AMMSB_MODULARITY_FRAC_BITS;

struct Args {
  const u64* mask;
  uint32_t rows, K, W;
  uint32_t gshift;  // w1: log2 of the lanes that own an item, the smallest power of two >= W
  const u64* edges;
  uint64_t n;
  uint32_t* degree;  // edges: added to; nodes: read
  u64* acc;          // edges: internal; nodes: volume
  u64* counts;
};

// acc[2k], acc[2k + 1] += (hi, lo) modulo 2^128
__device__ __forceinline__ void add128(u64* acc, uint32_t k, u64 lo, u64 hi) {
  const u64 old = atomicAdd(&acc[2u * k], lo);
  hi += (u64)(old + lo < old);  // (hi < 2^32: no wrap of its own)
  if (hi) atomicAdd(&acc[2u * k + 1u], hi);
}

// (lo, hi) to every community of the lane's word w
__device__ __forceinline__ void walk128(u64* acc, u64 bits, uint32_t w, u64 lo, u64 hi) {
  for (; bits; bits &= bits - 1) add128(acc, 64u * w + (uint32_t)__builtin_ctzll(bits), lo, hi);  // (< K: live_bits)
}

// the sum of v over the lanes of a group of G
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t G) {
  for (uint32_t o = G >> 1; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, (int)o, 64);  // o < G: stays inside the group
  return v;
}

template <int WPL>
struct Ends {
  bool exists, ok;  // the lane's group has an edge; both its ends are < num_rows
  uint32_t u, v;
  u64 x[WPL], y[WPL];
};

// the edge of the lane's group and the lane's words of both rows (zeros where there is nothing to read)
template <int WPL>
__device__ __forceinline__ void head(const Args& a, uint64_t p, uint32_t gl, Ends<WPL>& e) {
  e.exists = p < a.n;
  e.ok = false;
  e.u = e.v = 0;
  if (e.exists) {
    const u64 key = a.edges[p];
    e.u = (uint32_t)(key >> 32);
    e.v = (uint32_t)key;
    e.ok = e.u < a.rows && e.v < a.rows;
  }
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    e.x[i] = e.ok ? mask_word(a, e.u, gl + 64u * i) : 0ull;
    e.y[i] = e.ok ? mask_word(a, e.v, gl + 64u * i) : 0ull;
  }
}

template <int WPL>
__device__ __forceinline__ void edges_body(const Args& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * M_WAVES * epw;
  uint64_t pb = ((uint64_t)blockIdx.x * M_WAVES + (threadIdx.x >> 6)) * epw;  // the wave's first edge: wave-uniform
  u64 valid = 0, skipped = 0;  // of this wave's edges: wave-uniform
  Ends<WPL> e;
  head<WPL>(a, pb + slot, gl, e);
  for (; pb < a.n; pb += stride) {
    const bool exists = e.exists, ok = e.ok;
    const uint32_t u = e.u, v = e.v;
    u64 both[WPL], any = 0;
    uint32_t oa = 0, ob = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      both[i] = e.x[i] & e.y[i];
      any |= both[i];
      oa += (uint32_t)__popcll(e.x[i]);
      ob += (uint32_t)__popcll(e.y[i]);
    }
    head<WPL>(a, pb + stride + slot, gl, e);  // the next edge's words are on their way during the atomics
    oa = group_sum(oa, G);
    ob = group_sum(ob, G);
    valid += (u64)__popcll(__ballot(ok && gl == 0));
    skipped += (u64)__popcll(__ballot(exists && !ok && gl == 0));
    if (ok && gl == 0) {  // (u, v < rows)
      atomicAdd(&a.degree[u], 1u);
      atomicAdd(&a.degree[v], 1u);
    }
    if (any) {  // a shared community: O_a, O_b >= 1, and their product is at most 2^26
      const u64 w = FRAC / ((u64)oa * ob);
#pragma unroll
      for (int i = 0; i < WPL; ++i) walk128(a.acc, both[i], gl + 64u * i, w, 0);
    }
  }
  if (lane == 0) {
    if (valid) atomicAdd(&a.counts[0], valid);
    if (skipped) atomicAdd(&a.counts[1], skipped);
  }
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(M_BLOCK) void modularity_edges_w1(Args a) { edges_body<1>(a); }
__global__ __launch_bounds__(M_BLOCK) void modularity_edges_w2(Args a) { edges_body<2>(a); }

template <int WPL>
__device__ __forceinline__ void nodes_body(const Args& a) {
  const int lane = threadIdx.x & 63;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  const uint64_t stride = (uint64_t)gridDim.x * M_WAVES * epw;
  for (uint64_t rb = ((uint64_t)blockIdx.x * M_WAVES + (threadIdx.x >> 6)) * epw; rb < a.rows; rb += stride) {
    const uint64_t r = rb + slot;
    const uint32_t deg = r < a.rows ? a.degree[r] : 0u;
    u64 x[WPL];
    uint32_t o = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      x[i] = deg ? mask_word(a, (uint32_t)r, gl + 64u * i) : 0ull;
      o += (uint32_t)__popcll(x[i]);
    }
    o = group_sum(o, G);
    if (o) {  // (deg > 0 as well: without it no word was read)
      const u64 f = FRAC / (u64)o, lo = (u64)deg * f, hi = __umul64hi((u64)deg, f);  // deg f < 2^94
#pragma unroll
      for (int i = 0; i < WPL; ++i) walk128(a.acc, x[i], gl + 64u * i, lo, hi);
    }
  }
}

__global__ __launch_bounds__(M_BLOCK) void modularity_nodes_w1(Args a) { nodes_body<1>(a); }
__global__ __launch_bounds__(M_BLOCK) void modularity_nodes_w2(Args a) { nodes_body<2>(a); }

const char* check_shape(uint64_t num_rows, uint32_t K) {
  if (K == 0 || K > AMMSB_MODULARITY_MAX_COLS) return "num_cols outside 1..8192";
  if (num_rows >> 32) return "2^32 rows or more";
  return nullptr;
}


void shape(Args* a, const uint64_t* mask, uint64_t num_rows, uint32_t num_cols) {
  a->mask = reinterpret_cast<const u64*>(mask);
  a->rows = (uint32_t)num_rows;
  a->K = num_cols;
  a->W = (num_cols + 63u) / 64u;
  a->gshift = 0;
  while ((1u << a->gshift) < a->W && a->gshift < 6) ++a->gshift;
}

}  // namespace

extern "C" const char* ammsb_modularity_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_modularity_last_error(void) { return g_last_error; }

extern "C" int ammsb_modularity_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges,
                                      uint64_t n, uint32_t* degree, uint64_t* internal, uint64_t* counts, void* stream) {
  if (n > 0 && !mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (n > 0 && !edges) return fail(AMMSB_EINVAL, "edges is NULL");
  if (!degree) return fail(AMMSB_EINVAL, "degree is NULL");
  if (!internal) return fail(AMMSB_EINVAL, "internal is NULL");
  if (!counts) return fail(AMMSB_EINVAL, "counts is NULL");
  if (const char* bad = check_shape(num_rows, num_cols)) return fail(AMMSB_EINVAL, bad);
  if (n >= AMMSB_MODULARITY_MAX_EDGES) return fail(AMMSB_EINVAL, "2^31 edges or more");
  if (misaligned(degree, 4)) return fail(AMMSB_EINVAL, "degree is not 4-byte aligned");
  if (misaligned(internal, 8)) return fail(AMMSB_EINVAL, "internal is not 8-byte aligned");
  if (misaligned(counts, 8)) return fail(AMMSB_EINVAL, "counts is not 8-byte aligned");
  if (n == 0) return AMMSB_OK;

  Args a;
  shape(&a, mask, num_rows, num_cols);
  a.edges = reinterpret_cast<const u64*>(edges);
  a.n = n;
  a.degree = degree;
  a.acc = reinterpret_cast<u64*>(internal);
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(M_BLOCK);
  if (num_cols <= AMMSB_MODULARITY_W1_MAX_COLS) {
    const dim3 grid(persistent_grid(n, (uint64_t)M_WAVES * (64u >> a.gshift) * M_TRIPS));
    hipLaunchKernelGGL(modularity_edges_w1, grid, block, 0, s, a);
    return launched("modularity_edges_w1");
  }
  const dim3 grid(persistent_grid(n, (uint64_t)M_WAVES * M_TRIPS));
  hipLaunchKernelGGL(modularity_edges_w2, grid, block, 0, s, a);
  return launched("modularity_edges_w2");
}

extern "C" int ammsb_modularity_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint32_t* degree,
                                      uint64_t* volume, void* stream) {
  if (num_rows > 0 && !mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (num_rows > 0 && !degree) return fail(AMMSB_EINVAL, "degree is NULL");
  if (!volume) return fail(AMMSB_EINVAL, "volume is NULL");
  if (const char* bad = check_shape(num_rows, num_cols)) return fail(AMMSB_EINVAL, bad);
  if (misaligned(degree, 4)) return fail(AMMSB_EINVAL, "degree is not 4-byte aligned");
  if (misaligned(volume, 8)) return fail(AMMSB_EINVAL, "volume is not 8-byte aligned");
  if (num_rows == 0) return AMMSB_OK;

  Args a;
  shape(&a, mask, num_rows, num_cols);
  a.edges = nullptr;
  a.n = 0;
  a.degree = const_cast<uint32_t*>(degree);  // (read only)
  a.acc = reinterpret_cast<u64*>(volume);
  a.counts = nullptr;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 block(M_BLOCK);
  if (num_cols <= AMMSB_MODULARITY_W1_MAX_COLS) {
    const dim3 grid(persistent_grid(num_rows, (uint64_t)M_WAVES * (64u >> a.gshift) * M_TRIPS));
    hipLaunchKernelGGL(modularity_nodes_w1, grid, block, 0, s, a);
    return launched("modularity_nodes_w1");
  }
  const dim3 grid(persistent_grid(num_rows, (uint64_t)M_WAVES * M_TRIPS));
  hipLaunchKernelGGL(modularity_nodes_w2, grid, block, 0, s, a);
  return launched("modularity_nodes_w2");
}
