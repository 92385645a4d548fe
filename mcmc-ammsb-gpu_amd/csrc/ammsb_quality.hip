// libammsb_quality.so (include/ammsb_quality.h): per community the edges of a list that lie inside it (both ends are
// members) and the edges that leave it (exactly one end is), membership being pi[a, k] >= thr.
//
// Two passes, so that an edge costs K / 4 bytes and not the 8 K bytes of two rows of pi:
//   quality_mask_*   streams pi once, a wave per row, and writes W = ceil(K / 64) 64-bit words of membership bits per
//                    row: a compare and a __ballot give the 64 bits of one register slot of the wave.
//   quality_edges_*  a group of lanes per edge ANDs and XORs the two rows' words, counts the bits for `shared` and walks
//                    them into u32 counters private to the block in LDS (internal[K], boundary[K], uncovered, skipped),
//                    flushed with one 64-bit vector atomic per non-zero counter when the block has run out of edges.
//
// The mask's layout (private: the header promises only that it is a function of (num_rows, num_cols)).  Row r holds
// words r W .. r W + W - 1.  With F = 4 (K / 256), the words of the whole chunks of 256 columns:
//   word w < F,  bit j  <->  column 256 (w >> 2) + 4 j + (w & 3)      what lane j holds in component w & 3 of its
//                                                                     16-byte load number w >> 2: the ballot as it is
//   word w >= F, bit j  <->  column 64 w + j                          the ragged tail, in column order
// and bits of columns >= K are zero.  Both mask forms write exactly these words; col_of() is the inverse.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_quality.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int Q_WAVES = 4;  // waves per block
constexpr int Q_BLOCK = 64 * Q_WAVES;
constexpr int Q_TRIPS = 4;  // edges a group takes before another block is worth its 2 K + 2 counters' zeroing and flush

// ------------------------------------------------------------------------------------------ the mask pass
struct MaskArgs {
  ammsb_rpm pi;
  float thr;
  u64* mask;
};

// up to 4 float4 per lane: columns 1024 ch + 256 i + 4 lane + c of the row; registers past the row hold -1, which is
// below every threshold the entry point lets through
__device__ __forceinline__ void load_chunk(const MaskArgs& a, uint32_t row, int ch, int nvK, int lane, float4 (&x)[4]) {
  const float4* p = reinterpret_cast<const float4*>(postfit_row(a.pi, row)) + ch * 256 + lane;
  const int nv = min(nvK - 4 * ch, 4);
  const float4 none = {-1.f, -1.f, -1.f, -1.f};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    x[i] = none;
    if (i < nv) x[i] = p[i * 64];
  }
}

__global__ __launch_bounds__(Q_BLOCK) void quality_mask_fast(MaskArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = K >> 6;
  const int nvK = (int)(K >> 8), nch = (nvK + 3) >> 2;
  const uint64_t rows = a.pi.num_rows, stride = (uint64_t)gridDim.x * Q_WAVES;
  uint64_t r = (uint64_t)blockIdx.x * Q_WAVES + (threadIdx.x >> 6);
  float4 x[4];
  if (r < rows) load_chunk(a, (uint32_t)r, 0, nvK, lane, x);
  for (; r < rows; r += stride) {
    u64 w0 = 0, w1 = 0;
    for (int ch = 0; ch < nch; ++ch) {
      u64 b[16];
#pragma unroll
      for (int t = 0; t < 16; ++t) b[t] = __ballot(comp(x[t >> 2], t & 3) >= a.thr);
      // the registers are free: the next chunk, or the next row's first, before the words are placed and stored
      if (ch + 1 < nch) load_chunk(a, (uint32_t)r, ch + 1, nvK, lane, x);
      else if (r + stride < rows) load_chunk(a, (uint32_t)(r + stride), 0, nvK, lane, x);
#pragma unroll
      for (int t = 0; t < 16; ++t) place(w0, w1, 16u * ch + t, b[t], lane);
    }
    store_bit_row(a.mask, r, W, w0, w1, lane);
  }
}

__global__ __launch_bounds__(Q_BLOCK) void quality_mask_generic(MaskArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = (K + 63u) >> 6, F = 4u * (K >> 8);
  const uint64_t rows = a.pi.num_rows, stride = (uint64_t)gridDim.x * Q_WAVES;
  for (uint64_t r = (uint64_t)blockIdx.x * Q_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const float* p = postfit_row(a.pi, (uint32_t)r);
    u64 w0 = 0, w1 = 0;
    for (uint32_t t = 0; t < W; ++t) {
      const uint32_t col = slot_col(t < F, t, (uint32_t)lane);
      const float v = col < K ? p[col] : -1.0f;
      place(w0, w1, t, __ballot(v >= a.thr), lane);
    }
    store_bit_row(a.mask, r, W, w0, w1, lane);
  }
}

// ------------------------------------------------------------------------------------------ the edge pass
struct EdgeArgs {
  const u64* mask;
  uint32_t rows, K, W;
  uint32_t gshift;  // log2 of the lanes that own an edge: the smallest power of two >= W, at most 64
  const u64* edges;
  uint64_t n;
  u64* counts;
  int32_t* shared;
};

__device__ __forceinline__ uint32_t col_of(uint32_t w, uint32_t j, uint32_t F) {
  return slot_col(w < F, w, j);
}

template <int WPL>
struct Ends {
  bool exists, ok;  // the lane's group has an edge; both its ends are < num_rows
  u64 x[WPL], y[WPL];
};

// the edge of the lane's group and the lane's words of both rows (zeros where there is nothing to read)
template <int WPL>
__device__ __forceinline__ void head(const EdgeArgs& a, uint64_t p, uint32_t gl, Ends<WPL>& e) {
  e.exists = p < a.n;
  e.ok = false;
  uint32_t u = 0, v = 0;
  if (e.exists) {
    const u64 key = a.edges[p];
    u = (uint32_t)(key >> 32);
    v = (uint32_t)key;
    e.ok = u < a.rows && v < a.rows;
  }
#pragma unroll
  for (int i = 0; i < WPL; ++i) {
    const uint32_t w = gl + 64u * i;
    e.x[i] = 0;
    e.y[i] = 0;
    if (e.ok && w < a.W) {
      e.x[i] = a.mask[(uint64_t)u * a.W + w];
      e.y[i] = a.mask[(uint64_t)v * a.W + w];
    }
  }
}

__device__ __forceinline__ void walk(u64 bits, uint32_t w, uint32_t F, uint32_t* counters) {
  while (bits) {
    atomicAdd(&counters[col_of(w, (uint32_t)__builtin_ctzll(bits), F)], 1u);
    bits &= bits - 1;
  }
}

template <int WPL>
__device__ __forceinline__ void edges_body(const EdgeArgs& a, uint32_t* lds) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = a.K, F = 4u * (K >> 8), ncnt = 2u * K + 2u;
  const uint32_t gshift = WPL == 1 ? a.gshift : 6u, G = 1u << gshift;
  const uint32_t gl = lane & (G - 1u), slot = lane >> gshift, epw = 64u >> gshift;
  if (a.counts) zero_counters<Q_BLOCK>(lds, ncnt);
  const uint64_t stride = (uint64_t)gridDim.x * Q_WAVES * epw;
  uint64_t pb = ((uint64_t)blockIdx.x * Q_WAVES + (threadIdx.x >> 6)) * epw;  // the wave's first edge: wave-uniform
  Ends<WPL> e;
  head<WPL>(a, pb + slot, gl, e);
  for (; pb < a.n; pb += stride) {
    const uint64_t p = pb + slot;
    const bool exists = e.exists, ok = e.ok;
    u64 both[WPL], one[WPL], any = 0;
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      both[i] = e.x[i] & e.y[i];
      one[i] = e.x[i] ^ e.y[i];
      any |= both[i];
      cnt += __popcll(both[i]);
    }
    head<WPL>(a, pb + stride + slot, gl, e);  // the next edge's words are on their way during the bit walk
    if (a.shared) {
      for (uint32_t o = G >> 1; o > 0; o >>= 1) cnt += __shfl_xor(cnt, (int)o, 64);  // o < G: stays inside the group
      if (gl == 0 && exists) a.shared[p] = ok ? cnt : -1;
    }
    if (a.counts) {
      const u64 holders = __ballot(any != 0);
      const u64 mine = G == 64u ? holders : (holders >> (slot << gshift)) & ((1ull << G) - 1ull);
      if (gl == 0 && exists) {
        if (!ok) atomicAdd(&lds[2u * K + 1u], 1u);
        else if (mine == 0) atomicAdd(&lds[2u * K], 1u);
      }
#pragma unroll
      for (int i = 0; i < WPL; ++i) {
        walk(both[i], gl + 64u * i, F, lds);
        walk(one[i], gl + 64u * i, F, lds + K);
      }
    }
  }
  if (a.counts) flush_counters<Q_BLOCK>(lds, ncnt, a.counts);
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(Q_BLOCK) void quality_edges_w1(EdgeArgs a) {
  extern __shared__ uint32_t lds[];
  edges_body<1>(a, lds);
}

__global__ __launch_bounds__(Q_BLOCK) void quality_edges_w2(EdgeArgs a) {
  extern __shared__ uint32_t lds[];
  edges_body<2>(a, lds);
}

bool shape_ok(uint64_t num_rows, uint64_t num_cols) {
  return num_cols >= 1 && num_cols <= AMMSB_QUALITY_MAX_COLS && !(num_rows >> 32);
}

}  // namespace

extern "C" const char* ammsb_quality_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_quality_last_error(void) { return g_last_error; }

extern "C" uint64_t ammsb_quality_mask_bytes(uint64_t num_rows, uint32_t num_cols) {
  if (!shape_ok(num_rows, num_cols)) return 0;
  return num_rows * ((num_cols + 63u) / 64u) * sizeof(uint64_t);
}

extern "C" int ammsb_quality_mask(const ammsb_rpm* pi, float thr, uint64_t* mask, void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (!(thr >= 0.0f && thr < INFINITY)) return fail(AMMSB_EINVAL, "thr negative, NaN or infinite");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_QUALITY_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (reinterpret_cast<uintptr_t>(mask) & 7) return fail(AMMSB_EINVAL, "mask is not 8-byte aligned");
  if (pi->num_rows == 0) return AMMSB_OK;

  MaskArgs a;
  a.pi = *pi;
  a.thr = thr;
  a.mask = reinterpret_cast<u64*>(mask);
  const dim3 grid(persistent_grid(pi->num_rows, Q_WAVES)), block(Q_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name;
  if (pi->num_cols % 256 == 0 && aligned) {
    name = "quality_mask_fast";
    hipLaunchKernelGGL(quality_mask_fast, grid, block, 0, s, a);
  } else {
    name = "quality_mask_generic";
    hipLaunchKernelGGL(quality_mask_generic, grid, block, 0, s, a);
  }
  return launched(name);
}

extern "C" int ammsb_quality_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges,
                                   uint64_t n, uint64_t* counts, int32_t* shared, void* stream) {
  if (n > 0 && !mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (n > 0 && !edges) return fail(AMMSB_EINVAL, "edges is NULL");
  if (!counts && !shared) return fail(AMMSB_EINVAL, "no output");
  if (num_cols == 0 || num_cols > AMMSB_QUALITY_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (num_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (n == 0) return AMMSB_OK;

  EdgeArgs a;
  a.mask = reinterpret_cast<const u64*>(mask);
  a.rows = (uint32_t)num_rows;
  a.K = num_cols;
  a.W = (num_cols + 63u) / 64u;
  a.gshift = 0;
  while ((1u << a.gshift) < a.W && a.gshift < 6) ++a.gshift;
  a.edges = reinterpret_cast<const u64*>(edges);
  a.n = n;
  a.counts = reinterpret_cast<u64*>(counts);
  a.shared = shared;
  const dim3 grid(persistent_grid(n, (uint64_t)Q_WAVES * (64u >> a.gshift) * Q_TRIPS)), block(Q_BLOCK);
  const size_t lds = counts ? (size_t)(2u * num_cols + 2u) * sizeof(uint32_t) : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name;
  if (a.W <= 64) {
    name = "quality_edges_w1";
    hipLaunchKernelGGL(quality_edges_w1, grid, block, lds, s, a);
  } else {
    name = "quality_edges_w2";
    // 2 K + 2 counters are just over the default 64 KiB of dynamic LDS at K = 8192: once per process
    static const hipError_t big =
        hipFuncSetAttribute(reinterpret_cast<const void*>(&quality_edges_w2), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)((2u * AMMSB_QUALITY_MAX_COLS + 2u) * sizeof(uint32_t)));
    if (big != hipSuccess) return hip_fail(name, big);
    hipLaunchKernelGGL(quality_edges_w2, grid, block, lds, s, a);
  }
  return launched(name);
}
