// libammsb_spread.so (include/ammsb_spread.h): the lazy running mean and variance of pi over the chain, Welford's binary64
// moments of beta, the credible bound mean + z sd, and a row's total variance.  Streaming passes in the shape of
// ammsb_average.hip: nothing is reused, so everything is bounded by what the memory system delivers.
//
// spread_rows_v4 / _s1    the geometry of average_rows_*: a group of lanes per row (the smallest power of two >= ceil(K / 4),
//                         at most a wave), blocks of 4 waves persistent over a grid-stride of rows; the group's first lane
//                         claims the row (atomic exchange of last[a] for a node list, plain load and store for a row range)
//                         and hands `old` to the group with one shuffle.  w == 0 touches no row data; old == 0 copies pi to
//                         mean and zeroes var without reading either; otherwise the nine operations of the header.  A
//                         flushed row is 4 K bytes of pi, mean and var read and 4 K of mean and var written: 20 K bytes
//                         against the mean's 12 K.  The loads of four trips (three streams) are issued before the first is
//                         consumed.  _v4 moves 16 bytes per lane (K a multiple of 4, aligned blocks), _s1 4 bytes.
// spread_vector           Welford in binary64, one element per lane: beta's 2K floats.
// spread_bound_v4 / _s1   out = clamp(mean + z sqrt(var)), the same group-per-row walk over a row range.
// spread_rowsum           per row the binary64 sum of var in the 64-virtual-lane order of ammsb_reduce.h: lane l of the group
//                         reads the columns l, l + G, ... with 4-byte loads (side by side across the group, so a wave's
//                         loads still cover whole lines) and holds up to four virtual lanes; then the butterfly.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_spread.h"
#include "ammsb_postfit.h"

namespace {

constexpr int SP_BLOCK = 256;
constexpr int SP_AHEAD = 4;  // trips of a group whose loads are in flight together

struct Rows {
  ammsb_rpm pi, mean, var;
  uint32_t* last;
  const uint32_t* nodes;
  uint64_t first, count;
  uint32_t n, gshift;
};

struct Bound {
  ammsb_rpm mean, var, out;
  uint64_t first, count;
  float z;
  uint32_t gshift;
};

struct RowSum {
  ammsb_rpm var;
  double* out;
  uint64_t first, count;
  uint32_t gshift;
};

// the operations of the header, each rounded by itself whatever the contraction setting of the build.  m and v are
// replaced by mean' and var'.
__device__ __forceinline__ void merge(float& m, float& v, float p, float r, float s) {
  const float d = __fsub_rn(p, m);
  m = __fadd_rn(m, __fmul_rn(r, d));
  float e = __fmul_rn(d, d);
  e = __fmul_rn(e, s);
  e = __fsub_rn(e, v);
  e = __fmul_rn(r, e);
  v = __fadd_rn(v, e);
}

__device__ __forceinline__ void merge(float4& m, float4& v, const float4& p, float r, float s) {
  merge(m.x, v.x, p.x, r, s);
  merge(m.y, v.y, p.y, r, s);
  merge(m.z, v.z, p.z, r, s);
  merge(m.w, v.w, p.w, r, s);
}

__device__ __forceinline__ void clear(float& v) { v = 0.0f; }
__device__ __forceinline__ void clear(float4& v) { v = {0.0f, 0.0f, 0.0f, 0.0f}; }

// One row in units of T (float4 or float): unit u of the row for u = gl, gl + G, ... < units.
template <class T>
__device__ __forceinline__ void flush_row(const T* p, T* m, T* v, uint32_t units, uint32_t gl, uint32_t G, bool first,
                                          float ratio, float rest) {
  for (uint32_t u0 = gl; u0 < units; u0 += SP_AHEAD * G) {
    T pv[SP_AHEAD], mv[SP_AHEAD], vv[SP_AHEAD];
#pragma unroll
    for (int i = 0; i < SP_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) {
        pv[i] = p[u];
        if (!first) {
          mv[i] = m[u];
          vv[i] = v[u];
        }
      }
    }
#pragma unroll
    for (int i = 0; i < SP_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) {
        if (first) {
          mv[i] = pv[i];
          clear(vv[i]);
        } else {
          merge(mv[i], vv[i], pv[i], ratio, rest);
        }
        m[u] = mv[i];
        v[u] = vv[i];
      }
    }
  }
}

template <bool LIST, bool VEC>
__device__ __forceinline__ void flush_rows(const Rows& a) {
  const uint32_t G = 1u << a.gshift;
  const uint32_t lane = threadIdx.x & 63u, gl = threadIdx.x & (G - 1u);
  const uint32_t per_block = (uint32_t)SP_BLOCK >> a.gshift;
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
      const float rest = __fsub_rn(1.0f, ratio);
      const float* p = postfit_row(a.pi, row);
      float* m = const_cast<float*>(postfit_row(a.mean, row));
      float* v = const_cast<float*>(postfit_row(a.var, row));
      if (VEC)
        flush_row(reinterpret_cast<const float4*>(p), reinterpret_cast<float4*>(m), reinterpret_cast<float4*>(v), K >> 2, gl,
                  G, old == 0, ratio, rest);
      else
        flush_row(p, m, v, K, gl, G, old == 0, ratio, rest);
    }
  }
}

template <bool LIST>
__global__ __launch_bounds__(SP_BLOCK) void spread_rows_v4(Rows a) {
  flush_rows<LIST, true>(a);
}

template <bool LIST>
__global__ __launch_bounds__(SP_BLOCK) void spread_rows_s1(Rows a) {
  flush_rows<LIST, false>(a);
}

__global__ __launch_bounds__(SP_BLOCK) void spread_vector(const float* x, double* mean64, double* m2, uint64_t len, uint32_t n) {
  const double dn = (double)n;
  for (uint64_t i = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x; i < len; i += (uint64_t)gridDim.x * SP_BLOCK) {
    const double v = (double)x[i];
    if (n == 1u) {
      mean64[i] = v;
      m2[i] = 0.0;
    } else {
      const double m = mean64[i];
      const double delta = __dsub_rn(v, m);
      const double mn = __dadd_rn(m, __ddiv_rn(delta, dn));
      mean64[i] = mn;
      m2[i] = __dadd_rn(m2[i], __dmul_rn(delta, __dsub_rn(v, mn)));
    }
  }
}

// The correctly rounded binary32 square root, chosen explicitly: binary64's (always correctly rounded) rounded once more.
// 53 >= 2 * 24 + 2 bits, so the two roundings give what one would.  (__fsqrt_rn is the native approximation in this
// toolchain's headers, and sqrtf() is correctly rounded only under a compile flag's default.)
__device__ __forceinline__ float sqrt_rn(float v) { return __double2float_rn(__builtin_sqrt((double)v)); }

// !(t > 0) covers a NaN from either input and from a negative var
__device__ __forceinline__ float bound(float m, float v, float z) {
  const float t = __fadd_rn(m, __fmul_rn(z, sqrt_rn(v)));
  return t > 0.0f ? fminf(t, 1.0f) : 0.0f;
}

__device__ __forceinline__ float4 bound(const float4& m, const float4& v, float z) {
  return {bound(m.x, v.x, z), bound(m.y, v.y, z), bound(m.z, v.z, z), bound(m.w, v.w, z)};
}

template <class T>
__device__ __forceinline__ void bound_row(const T* m, const T* v, T* o, uint32_t units, uint32_t gl, uint32_t G, float z) {
  for (uint32_t u0 = gl; u0 < units; u0 += SP_AHEAD * G) {
    T mv[SP_AHEAD], vv[SP_AHEAD];
#pragma unroll
    for (int i = 0; i < SP_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) {
        mv[i] = m[u];
        vv[i] = v[u];
      }
    }
#pragma unroll
    for (int i = 0; i < SP_AHEAD; ++i) {
      const uint32_t u = u0 + i * G;
      if (u < units) o[u] = bound(mv[i], vv[i], z);
    }
  }
}

template <bool VEC>
__device__ __forceinline__ void bound_rows(const Bound& a) {
  const uint32_t G = 1u << a.gshift;
  const uint32_t gl = threadIdx.x & (G - 1u);
  const uint32_t per_block = (uint32_t)SP_BLOCK >> a.gshift;
  const uint64_t stride = (uint64_t)gridDim.x * per_block;
  const uint32_t K = (uint32_t)a.mean.num_cols;
  for (uint64_t r = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> a.gshift); r < a.count; r += stride) {
    const uint32_t row = (uint32_t)(a.first + r);  // (first + count <= num_rows < 2^32)
    const float* m = postfit_row(a.mean, row);
    const float* v = postfit_row(a.var, row);
    float* o = const_cast<float*>(postfit_row(a.out, row));
    if (VEC)
      bound_row(reinterpret_cast<const float4*>(m), reinterpret_cast<const float4*>(v), reinterpret_cast<float4*>(o), K >> 2,
                gl, G, a.z);
    else
      bound_row(m, v, o, K, gl, G, a.z);
  }
}

__global__ __launch_bounds__(SP_BLOCK) void spread_bound_v4(Bound a) { bound_rows<true>(a); }
__global__ __launch_bounds__(SP_BLOCK) void spread_bound_s1(Bound a) { bound_rows<false>(a); }

__global__ __launch_bounds__(SP_BLOCK) void spread_rowsum(RowSum a) {
  const uint32_t G = 1u << a.gshift;
  const uint32_t gl = threadIdx.x & (G - 1u);
  const uint32_t per_block = (uint32_t)SP_BLOCK >> a.gshift;
  const uint64_t stride = (uint64_t)gridDim.x * per_block;
  const uint32_t K = (uint32_t)a.var.num_cols;
  // the same number of trips in every lane: the butterfly needs the whole group
  const uint64_t trips = (a.count + stride - 1) / stride;
  uint64_t r = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> a.gshift);
  for (uint64_t t = 0; t < trips; ++t, r += stride) {
    const bool ok = r < a.count;
    // Virtual lane v = j & 63 lives in lane v & (G - 1), as its sum number v >> gshift.  K <= 4 G below a wave, so a lane's
    // i-th column is j = gl + i G with i < 4: sum i where the row has at most 64 columns (G <= 16), sum i & 1 for G = 32,
    // sum 0 for a wave.  The sums past a group's last virtual lane stay 0.0 and add nothing.
    double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
    if (ok) {
      const float* p = postfit_row(a.var, (uint32_t)(a.first + r));
      for (uint32_t j0 = gl; j0 < K; j0 += SP_AHEAD * G) {
        float x[SP_AHEAD];
#pragma unroll
        for (int i = 0; i < SP_AHEAD; ++i) {
          const uint32_t j = j0 + i * G;
          if (j < K) x[i] = p[j];
        }
#pragma unroll
        for (int i = 0; i < SP_AHEAD; ++i) {
          const uint32_t j = j0 + i * G;
          if (j < K) {
            const double d = (double)x[i];
            const uint32_t n = G <= 16u ? (uint32_t)i : G == 32u ? (uint32_t)i & 1u : 0u;
            if (n == 0) s0 = __dadd_rn(s0, d);
            else if (n == 1) s1 = __dadd_rn(s1, d);
            else if (n == 2) s2 = __dadd_rn(s2, d);
            else s3 = __dadd_rn(s3, d);
          }
        }
      }
    }
    // the butterfly: the levels whose partner is another sum of the same lane (distances 2 G and G), then the lanes
    s0 = __dadd_rn(s0, s2);
    s1 = __dadd_rn(s1, s3);
    s0 = __dadd_rn(s0, s1);
    for (uint32_t d = G >> 1; d > 0; d >>= 1) s0 = __dadd_rn(s0, __shfl_xor(s0, (int)d, 64));
    if (ok && gl == 0) a.out[r] = s0;
  }
}

// lanes of a group as a shift: the smallest power of two >= ceil(K / 4), at most 64
// (spread_rowsum's choice of which per-lane sum stands for which virtual lane rests on K <= 4 G below a wave: change the
// two together)
uint32_t group_shift(uint64_t num_cols) {
  const uint64_t units = (num_cols + 3u) / 4u;
  uint32_t g = 0;
  while ((1ull << g) < units && g < 6) ++g;
  return g;
}

bool same_geometry(const ammsb_rpm* a, const ammsb_rpm* b) {
  return a->num_rows == b->num_rows && a->num_cols == b->num_cols && a->rows_in_block == b->rows_in_block &&
         a->num_blocks == b->num_blocks;
}

// (equal geometry) some block of a is a block of b
bool share_a_block(const ammsb_rpm* a, const ammsb_rpm* b) {
  for (uint32_t i = 0; i < a->num_blocks; ++i)
    for (uint32_t j = 0; j < b->num_blocks; ++j)
      if (a->blocks[i] == b->blocks[j]) return true;
  return false;
}

}  // namespace

extern "C" const char* ammsb_spread_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_spread_last_error(void) { return g_last_error; }

extern "C" int ammsb_spread_rows(const ammsb_rpm* pi, const ammsb_rpm* mean, const ammsb_rpm* var, uint32_t* last,
                                 const uint32_t* nodes, uint64_t first, uint64_t count, uint32_t n, void* stream) {
  if (!pi || !mean || !var) return fail(AMMSB_EINVAL, "pi, mean or var is NULL");
  bool pi_aligned, mean_aligned, var_aligned;
  if (const char* bad = check_rpm(pi, AMMSB_SPREAD_MAX_COLS, &pi_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(mean, AMMSB_SPREAD_MAX_COLS, &mean_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(var, AMMSB_SPREAD_MAX_COLS, &var_aligned)) return fail(AMMSB_EINVAL, bad);
  if (!same_geometry(pi, mean) || !same_geometry(pi, var)) return fail(AMMSB_EINVAL, "pi, mean and var differ in geometry");
  if (share_a_block(pi, mean) || share_a_block(pi, var) || share_a_block(mean, var))
    return fail(AMMSB_EINVAL, "two of pi, mean and var share a block");
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
  a.var = *var;
  a.last = last;
  a.nodes = nodes;
  a.first = first;
  a.count = count;
  a.n = n;
  a.gshift = group_shift(pi->num_cols);
  const dim3 grid(persistent_grid(count, (uint64_t)SP_BLOCK >> a.gshift)), block(SP_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = pi->num_cols % 4 == 0 && pi_aligned && mean_aligned && var_aligned;
  const char* name;
  if (vec && nodes) { name = "spread_rows_v4<list>"; hipLaunchKernelGGL(spread_rows_v4<true>, grid, block, 0, s, a); }
  else if (vec) { name = "spread_rows_v4<range>"; hipLaunchKernelGGL(spread_rows_v4<false>, grid, block, 0, s, a); }
  else if (nodes) { name = "spread_rows_s1<list>"; hipLaunchKernelGGL(spread_rows_s1<true>, grid, block, 0, s, a); }
  else { name = "spread_rows_s1<range>"; hipLaunchKernelGGL(spread_rows_s1<false>, grid, block, 0, s, a); }
  return launched(name);
}

extern "C" int ammsb_spread_vector(const float* x, double* mean64, double* m2, uint64_t len, uint32_t n, void* stream) {
  if (n == 0) return fail(AMMSB_EINVAL, "n == 0");
  if (len >> 32) return fail(AMMSB_EINVAL, "2^32 elements or more");
  if (len == 0) return AMMSB_OK;
  if (!x || !mean64 || !m2) return fail(AMMSB_EINVAL, "x, mean64 or m2 is NULL");
  if (misaligned(x, 4) || misaligned(mean64, 8) || misaligned(m2, 8))
    return fail(AMMSB_EINVAL, "x, mean64 or m2 is not aligned to its element");
  if (mean64 == m2) return fail(AMMSB_EINVAL, "mean64 and m2 are the same buffer");
  hipLaunchKernelGGL(spread_vector, dim3(persistent_grid(len, SP_BLOCK)), dim3(SP_BLOCK), 0, static_cast<hipStream_t>(stream), x,
                     mean64, m2, len, n);
  return launched("spread_vector");
}

extern "C" int ammsb_spread_bound(const ammsb_rpm* mean, const ammsb_rpm* var, const ammsb_rpm* out, float z, uint64_t first,
                                  uint64_t count, void* stream) {
  if (!mean || !var || !out) return fail(AMMSB_EINVAL, "mean, var or out is NULL");
  bool mean_aligned, var_aligned, out_aligned;
  if (const char* bad = check_rpm(mean, AMMSB_SPREAD_MAX_COLS, &mean_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(var, AMMSB_SPREAD_MAX_COLS, &var_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(out, AMMSB_SPREAD_MAX_COLS, &out_aligned)) return fail(AMMSB_EINVAL, bad);
  if (!same_geometry(mean, var) || !same_geometry(mean, out)) return fail(AMMSB_EINVAL, "mean, var and out differ in geometry");
  if (share_a_block(out, mean) || share_a_block(out, var)) return fail(AMMSB_EINVAL, "out and an input share a block");
  if (!isfinite(z)) return fail(AMMSB_EINVAL, "z is not finite");
  if (count >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (first > mean->num_rows || count > mean->num_rows - first) return fail(AMMSB_EINVAL, "row range past num_rows");
  if (count == 0) return AMMSB_OK;

  Bound a;
  a.mean = *mean;
  a.var = *var;
  a.out = *out;
  a.first = first;
  a.count = count;
  a.z = z;
  a.gshift = group_shift(mean->num_cols);
  const dim3 grid(persistent_grid(count, (uint64_t)SP_BLOCK >> a.gshift)), block(SP_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean->num_cols % 4 == 0 && mean_aligned && var_aligned && out_aligned) {
    hipLaunchKernelGGL(spread_bound_v4, grid, block, 0, s, a);
    return launched("spread_bound_v4");
  }
  hipLaunchKernelGGL(spread_bound_s1, grid, block, 0, s, a);
  return launched("spread_bound_s1");
}

extern "C" int ammsb_spread_rowsum(const ammsb_rpm* var, double* out, uint64_t first, uint64_t count, void* stream) {
  if (!var) return fail(AMMSB_EINVAL, "var is NULL");
  bool aligned;
  if (const char* bad = check_rpm(var, AMMSB_SPREAD_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (count >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (first > var->num_rows || count > var->num_rows - first) return fail(AMMSB_EINVAL, "row range past num_rows");
  if (count == 0) return AMMSB_OK;
  if (!out) return fail(AMMSB_EINVAL, "out is NULL");
  if (misaligned(out, 8)) return fail(AMMSB_EINVAL, "out is not 8-byte aligned");

  RowSum a;
  a.var = *var;
  a.out = out;
  a.first = first;
  a.count = count;
  a.gshift = group_shift(var->num_cols);
  hipLaunchKernelGGL(spread_rowsum, dim3(persistent_grid(count, (uint64_t)SP_BLOCK >> a.gshift)), dim3(SP_BLOCK), 0,
                     static_cast<hipStream_t>(stream), a);
  return launched("spread_rowsum");
}
