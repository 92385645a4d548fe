// libammsb_average.so (include/ammsb_average.h): the lazy running mean of pi over the chain, and the eager binary64 mean of
// beta.
//
// average_rows_v4 / _s1   a group of lanes per row (the smallest power of two >= ceil(K / 4), at most a wave), blocks of 4
//                         waves persistent over a grid-stride of rows.  The group's first lane claims the row -- an atomic
//                         exchange of last[a] for a node list, which may name a row many times, a plain load and store for
//                         a row range, which cannot -- and hands `old` to the group with one shuffle.  w == 0 (somebody
//                         else claimed it in this call, or nothing ran since the last flush) touches no row data; old == 0
//                         copies pi to mean without reading mean; otherwise mean += (w / n) (pi - mean) in four separately
//                         rounded operations.  Nothing is reused: a flushed row is 4 K bytes of pi read, 4 K of mean read
//                         and 4 K of mean written, so the loads of four trips are issued before the first is consumed and
//                         the kernel is bounded by what the memory system delivers for scattered 4 K-byte rows.  _v4 moves
//                         16 bytes per lane (K a multiple of 4, aligned blocks), _s1 4 bytes (everything else).
// average_vector          mean64 += (double(x) - mean64) / n, one element per lane: beta's 2K floats.
// average_round           binary64 -> binary32, once per read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_average.h"
#include "ammsb_postfit.h"

namespace {

constexpr int AV_BLOCK = 256;
constexpr int AV_AHEAD = 4;  // trips of a group whose loads are in flight together

struct Rows {
  ammsb_rpm pi, mean;
  uint32_t* last;
  const uint32_t* nodes;
  uint64_t first, count;
  uint32_t n, gshift;
};

// the four operations of the header, each rounded by itself whatever the contraction setting of the build
__device__ __forceinline__ float fold(float m, float p, float r) { return __fadd_rn(m, __fmul_rn(r, __fsub_rn(p, m))); }

__device__ __forceinline__ float4 fold(const float4& m, const float4& p, float r) {
  return {fold(m.x, p.x, r), fold(m.y, p.y, r), fold(m.z, p.z, r), fold(m.w, p.w, r)};
}

// One row in units of T (float4 or float): unit u of the row for u = gl, gl + G, ... < units.
template <class T>
__device__ __forceinline__ void flush_row(const T* p, T* m, uint32_t units, uint32_t gl, uint32_t G, bool first, float ratio) {
  for (uint32_t u0 = gl; u0 < units; u0 += AV_AHEAD * G) {
    T pv[AV_AHEAD], mv[AV_AHEAD];
#pragma unroll
    for (int i = 0; i < AV_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) {
        pv[i] = p[u];
        if (!first) mv[i] = m[u];
      }
    }
#pragma unroll
    for (int i = 0; i < AV_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) m[u] = first ? pv[i] : fold(mv[i], pv[i], ratio);
    }
  }
}

template <bool LIST, bool VEC>
__device__ __forceinline__ void flush_rows(const Rows& a) {
  const uint32_t G = 1u << a.gshift;
  const uint32_t lane = threadIdx.x & 63u, gl = threadIdx.x & (G - 1u);
  const uint32_t per_block = (uint32_t)AV_BLOCK >> a.gshift;
  const uint64_t stride = (uint64_t)gridDim.x * per_block;
  const uint32_t N = (uint32_t)a.pi.num_rows, K = (uint32_t)a.pi.num_cols;
  const float fn = (float)a.n;
  // the same number of trips in every lane: the shuffle below needs the group's first lane to be there
  const uint64_t trips = (a.count + stride - 1) / stride;
  uint64_t r = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> a.gshift);
  for (uint64_t t = 0; t < trips; ++t, r += stride) {
    uint32_t row = 0, old = a.n;  // old == n: nothing to do
    bool ok = r < a.count;
    if (ok) {
      row = LIST ? a.nodes[r] : (uint32_t)(a.first + r);
      ok = row < N;
    }
    if (ok && gl == 0) {
      if (LIST) {
        old = atomicExch(&a.last[row], a.n);
      } else {
        old = a.last[row];
        a.last[row] = a.n;
      }
    }
    old = (uint32_t)__shfl((int)old, (int)(lane & ~(G - 1u)), 64);
    if (ok && old != a.n) {
      const float ratio = __fdiv_rn((float)(a.n - old), fn);
      const float* p = postfit_row(a.pi, row);
      float* m = const_cast<float*>(postfit_row(a.mean, row));
      if (VEC)
        flush_row(reinterpret_cast<const float4*>(p), reinterpret_cast<float4*>(m), K >> 2, gl, G, old == 0, ratio);
      else
        flush_row(p, m, K, gl, G, old == 0, ratio);
    }
  }
}

template <bool LIST>
__global__ __launch_bounds__(AV_BLOCK) void average_rows_v4(Rows a) {
  flush_rows<LIST, true>(a);
}

template <bool LIST>
__global__ __launch_bounds__(AV_BLOCK) void average_rows_s1(Rows a) {
  flush_rows<LIST, false>(a);
}

__global__ __launch_bounds__(AV_BLOCK) void average_vector(const float* x, double* mean64, uint64_t len, uint32_t n) {
  const double dn = (double)n;
  for (uint64_t i = (uint64_t)blockIdx.x * AV_BLOCK + threadIdx.x; i < len; i += (uint64_t)gridDim.x * AV_BLOCK) {
    const double v = (double)x[i];
    if (n == 1u) {
      mean64[i] = v;
    } else {
      const double m = mean64[i];
      mean64[i] = __dadd_rn(m, __ddiv_rn(__dsub_rn(v, m), dn));
    }
  }
}

__global__ __launch_bounds__(AV_BLOCK) void average_round(const double* mean64, float* out32, uint64_t len) {
  for (uint64_t i = (uint64_t)blockIdx.x * AV_BLOCK + threadIdx.x; i < len; i += (uint64_t)gridDim.x * AV_BLOCK)
    out32[i] = __double2float_rn(mean64[i]);
}

// lanes of a group as a shift: the smallest power of two >= ceil(K / 4), at most 64
uint32_t group_shift(uint64_t num_cols) {
  const uint64_t units = (num_cols + 3u) / 4u;
  uint32_t g = 0;
  while ((1ull << g) < units && g < 6) ++g;
  return g;
}

}  // namespace

extern "C" const char* ammsb_average_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_average_last_error(void) { return g_last_error; }

extern "C" int ammsb_average_rows(const ammsb_rpm* pi, const ammsb_rpm* mean, uint32_t* last, const uint32_t* nodes,
                                  uint64_t first, uint64_t count, uint32_t n, void* stream) {
  if (!pi || !mean) return fail(AMMSB_EINVAL, "pi or mean is NULL");
  bool pi_aligned, mean_aligned;
  if (const char* bad = check_rpm(pi, AMMSB_AVERAGE_MAX_COLS, &pi_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(mean, AMMSB_AVERAGE_MAX_COLS, &mean_aligned)) return fail(AMMSB_EINVAL, bad);
  if (pi->num_rows != mean->num_rows || pi->num_cols != mean->num_cols || pi->rows_in_block != mean->rows_in_block ||
      pi->num_blocks != mean->num_blocks)
    return fail(AMMSB_EINVAL, "pi and mean differ in geometry");
  for (uint32_t b = 0; b < pi->num_blocks; ++b)
    if (pi->blocks[b] == mean->blocks[b]) return fail(AMMSB_EINVAL, "pi and mean share a block");
  if (count >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (nodes) {
    if (first != 0) return fail(AMMSB_EINVAL, "a node list with first != 0");
    if (n == 0) return fail(AMMSB_EINVAL, "a node list with n == 0");
    if (misaligned(nodes, 4)) return fail(AMMSB_EINVAL, "nodes is not 4-byte aligned");
  } else if (first > pi->num_rows || count > pi->num_rows - first) {
    return fail(AMMSB_EINVAL, "row range past num_rows");
  }
  if (count == 0 || n == 0) return AMMSB_OK;
  if (!last) return fail(AMMSB_EINVAL, "last is NULL");
  if (misaligned(last, 4)) return fail(AMMSB_EINVAL, "last is not 4-byte aligned");

  Rows a;
  a.pi = *pi;
  a.mean = *mean;
  a.last = last;
  a.nodes = nodes;
  a.first = first;
  a.count = count;
  a.n = n;
  a.gshift = group_shift(pi->num_cols);
  const dim3 grid(persistent_grid(count, (uint64_t)AV_BLOCK >> a.gshift)), block(AV_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = pi->num_cols % 4 == 0 && pi_aligned && mean_aligned;
  const char* name;
  if (vec && nodes) { name = "average_rows_v4<list>"; hipLaunchKernelGGL(average_rows_v4<true>, grid, block, 0, s, a); }
  else if (vec) { name = "average_rows_v4<range>"; hipLaunchKernelGGL(average_rows_v4<false>, grid, block, 0, s, a); }
  else if (nodes) { name = "average_rows_s1<list>"; hipLaunchKernelGGL(average_rows_s1<true>, grid, block, 0, s, a); }
  else { name = "average_rows_s1<range>"; hipLaunchKernelGGL(average_rows_s1<false>, grid, block, 0, s, a); }
  return launched(name);
}

extern "C" int ammsb_average_vector(const float* x, double* mean64, uint64_t len, uint32_t n, void* stream) {
  if (n == 0) return fail(AMMSB_EINVAL, "n == 0");
  if (len >> 32) return fail(AMMSB_EINVAL, "2^32 elements or more");
  if (len == 0) return AMMSB_OK;
  if (!x || !mean64) return fail(AMMSB_EINVAL, "x or mean64 is NULL");
  if (misaligned(x, 4) || misaligned(mean64, 8)) return fail(AMMSB_EINVAL, "x or mean64 is not aligned to its element");
  hipLaunchKernelGGL(average_vector, dim3(persistent_grid(len, AV_BLOCK)), dim3(AV_BLOCK), 0, static_cast<hipStream_t>(stream),
                     x, mean64, len, n);
  return launched("average_vector");
}

extern "C" int ammsb_average_round(const double* mean64, float* out32, uint64_t len, void* stream) {
  if (len >> 32) return fail(AMMSB_EINVAL, "2^32 elements or more");
  if (len == 0) return AMMSB_OK;
  if (!mean64 || !out32) return fail(AMMSB_EINVAL, "mean64 or out32 is NULL");
  if (misaligned(mean64, 8) || misaligned(out32, 4)) return fail(AMMSB_EINVAL, "mean64 or out32 is not aligned to its element");
  hipLaunchKernelGGL(average_round, dim3(persistent_grid(len, AV_BLOCK)), dim3(AV_BLOCK), 0, static_cast<hipStream_t>(stream),
                     mean64, out32, len);
  return launched("average_round");
}
