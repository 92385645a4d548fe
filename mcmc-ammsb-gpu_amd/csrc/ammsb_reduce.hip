// libammsb_reduce.so (include/ammsb_reduce.h): the fitted model at K' < K communities -- sources merged, communities dropped.
//
// reduce_select_v4 / _s1  every new community has one source: out[a, j] = pi[a, src[j]], a gather.
// reduce_merge_v4 / _s1   the general plan: out[a, j] = the left-to-right binary32 sum over src[src_off[j] .. src_off[j + 1]).
//                         Both: a group of lanes per row (the smallest power of two >= ceil(K / 4), at most a wave), blocks
//                         persistent over a grid-stride of rows.  The group stages its row of pi in LDS -- the one read of pi,
//                         16 bytes per lane (_v4: K a multiple of 4, aligned blocks) or 4 (_s1) -- and lane l then owns the
//                         output columns l, l + G, ..., so a group's stores lie side by side.  A dropping plan makes two
//                         walks over the staged row: the first adds every t[j] into the lane's binary64 sums (the 64 virtual
//                         lanes of the header: a lane of a narrow group holds up to four of them), the butterfly gives every
//                         lane s, and the second walk recomputes t[j] -- the same operations, so the same bits -- and
//                         stores t[j] / (float) s.  That costs LDS reads, which are plentiful, instead of K' / G registers
//                         or a second staged row, which are not: at K = 8192 a row is 32 KiB, and what limits the rows in
//                         flight per CU is the 160 KiB of LDS (two rows per block of 128 lanes above K = 4096, four per
//                         block of 256 below).
// reduce_theta            one block: theta'[j, i] = the same left-to-right sum of theta[k, i].
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_reduce.h"
#include "ammsb_postfit.h"

namespace {

constexpr int RD_BLOCK = 256;
constexpr int RD_AHEAD = 4;  // loads of a lane in flight together while a row is staged

struct Rows {
  ammsb_rpm pi, out;
  const float* phi;
  float* out_phi;
  const uint32_t* src_off;
  const uint32_t* src;
  unsigned long long* emptied;
  uint64_t first, count;
  uint32_t gshift, drops;
};

// units u = gl, gl + G, ... < units of the row, global -> LDS
template <class T>
__device__ __forceinline__ void stage_row(const T* p, T* s, uint32_t units, uint32_t gl, uint32_t G) {
  for (uint32_t u0 = gl; u0 < units; u0 += RD_AHEAD * G) {
    T v[RD_AHEAD];
#pragma unroll
    for (int i = 0; i < RD_AHEAD; ++i)
      if (u0 + i * G < units) v[i] = p[u0 + i * G];
#pragma unroll
    for (int i = 0; i < RD_AHEAD; ++i)
      if (u0 + i * G < units) s[u0 + i * G] = v[i];
  }
}

// t[j] of the header from the staged row (or from theta, with a stride of 2)
template <bool SELECT>
__device__ __forceinline__ float merged(const float* row, const uint32_t* src_off, const uint32_t* src, uint32_t j,
                                        uint32_t stride = 1) {
  if (SELECT) return row[(size_t)src[j] * stride];
  const uint32_t b = src_off[j], e = src_off[j + 1];
  float t = row[(size_t)src[b] * stride];
  for (uint32_t p = b + 1; p < e; ++p) t = __fadd_rn(t, row[(size_t)src[p] * stride]);
  return t;
}

template <bool VEC, bool SELECT>
__device__ __forceinline__ void reduce_rows(const Rows& a) {
  extern __shared__ float4 rd_lds[];
  const uint32_t G = 1u << a.gshift, gl = threadIdx.x & (G - 1u);
  const uint32_t per_block = blockDim.x >> a.gshift;
  const uint32_t K = (uint32_t)a.pi.num_cols, K2 = (uint32_t)a.out.num_cols;
  float* stage = reinterpret_cast<float*>(rd_lds) + (size_t)(threadIdx.x >> a.gshift) * K;  // (_v4: K % 4 == 0, so 16-byte aligned)
  const uint64_t stride = (uint64_t)gridDim.x * per_block;
  // the same number of trips in every lane of the block: the barriers below need all of them
  const uint64_t trips = (a.count + stride - 1) / stride;
  uint64_t r = (uint64_t)blockIdx.x * per_block + (threadIdx.x >> a.gshift);
  for (uint64_t trip = 0; trip < trips; ++trip, r += stride) {
    const bool ok = r < a.count;
    const uint32_t row = (uint32_t)(a.first + (ok ? r : 0));
    if (ok) {
      const float* p = postfit_row(a.pi, row);
      if (VEC)
        stage_row(reinterpret_cast<const float4*>(p), reinterpret_cast<float4*>(stage), K >> 2, gl, G);
      else
        stage_row(p, stage, K, gl, G);
    }
    __syncthreads();
    if (ok) {
      float* o = const_cast<float*>(postfit_row(a.out, row));
      if (!a.drops) {
        for (uint32_t j = gl; j < K2; j += G) o[j] = merged<SELECT>(stage, a.src_off, a.src, j);
        if (gl == 0) a.out_phi[row] = a.phi[row];
      } else {
        // Virtual lane v = j & 63 lives in lane v & (G - 1), as its sum number (v >> gshift).  K' <= K <= 4 G below a wave,
        // so a lane's i-th column is j = gl + i G with i < 4: sum i where the row has at most 64 columns (G <= 16), sum
        // i & 1 for G = 32, sum 0 for a wave.  The sums past a group's last virtual lane stay 0.0 and add nothing.
        double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
        uint32_t i = 0;
        for (uint32_t j = gl; j < K2; j += G, ++i) {
          const double t = (double)merged<SELECT>(stage, a.src_off, a.src, j);
          const uint32_t n = a.gshift == 6 ? 0u : a.gshift == 5 ? (i & 1u) : i;
          if (n == 0) s0 = __dadd_rn(s0, t);
          else if (n == 1) s1 = __dadd_rn(s1, t);
          else if (n == 2) s2 = __dadd_rn(s2, t);
          else s3 = __dadd_rn(s3, t);
        }
        // the butterfly: the levels whose partner is another sum of the same lane (distances 2 G and G), then the lanes
        s0 = __dadd_rn(s0, s2);
        s1 = __dadd_rn(s1, s3);
        s0 = __dadd_rn(s0, s1);
        for (uint32_t d = G >> 1; d > 0; d >>= 1) s0 = __dadd_rn(s0, __shfl_xor(s0, (int)d, 64));
        const float sf = __double2float_rn(s0);
        if (sf > 0.0f) {
          for (uint32_t j = gl; j < K2; j += G) o[j] = __fdiv_rn(merged<SELECT>(stage, a.src_off, a.src, j), sf);
          if (gl == 0) a.out_phi[row] = __fmul_rn(a.phi[row], sf);
        } else {
          const float u = __fdiv_rn(1.0f, (float)K2);
          for (uint32_t j = gl; j < K2; j += G) o[j] = u;
          if (gl == 0) {
            a.out_phi[row] = a.phi[row];
            atomicAdd(a.emptied, 1ull);
          }
        }
      }
    }
    __syncthreads();  // the next trip overwrites the staged rows
  }
}

__global__ __launch_bounds__(RD_BLOCK) void reduce_select_v4(Rows a) { reduce_rows<true, true>(a); }
__global__ __launch_bounds__(RD_BLOCK) void reduce_select_s1(Rows a) { reduce_rows<false, true>(a); }
__global__ __launch_bounds__(RD_BLOCK) void reduce_merge_v4(Rows a) { reduce_rows<true, false>(a); }
__global__ __launch_bounds__(RD_BLOCK) void reduce_merge_s1(Rows a) { reduce_rows<false, false>(a); }

__global__ __launch_bounds__(RD_BLOCK) void reduce_theta(const float* theta, const uint32_t* src_off, const uint32_t* src,
                                                         uint32_t new_cols, float* out) {
  for (uint32_t e = threadIdx.x; e < 2u * new_cols; e += RD_BLOCK) {
    const uint32_t j = e >> 1, i = e & 1u;
    out[e] = src_off ? merged<false>(theta + i, src_off, src, j, 2) : merged<true>(theta + i, src_off, src, j, 2);
  }
}

// lanes of a group as a shift: the smallest power of two >= ceil(K / 4), at most 64
uint32_t group_shift(uint64_t num_cols) {
  const uint64_t units = (num_cols + 3u) / 4u;
  uint32_t g = 0;
  while ((1ull << g) < units && g < 6) ++g;
  return g;
}

}  // namespace

extern "C" const char* ammsb_reduce_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_reduce_last_error(void) { return g_last_error; }

extern "C" int ammsb_reduce_rows(const ammsb_rpm* pi, const float* phi_sum, const uint32_t* src_off, const uint32_t* src,
                                 uint32_t new_cols, uint32_t drops, const ammsb_rpm* out_pi, float* out_phi_sum,
                                 uint64_t* emptied, uint64_t first, uint64_t count, void* stream) {
  if (!pi || !out_pi) return fail(AMMSB_EINVAL, "pi or out_pi is NULL");
  bool pi_aligned, out_aligned;
  if (const char* bad = check_rpm(pi, AMMSB_REDUCE_MAX_COLS, &pi_aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_rpm(out_pi, AMMSB_REDUCE_MAX_COLS, &out_aligned)) return fail(AMMSB_EINVAL, bad);
  if (pi->num_rows != out_pi->num_rows) return fail(AMMSB_EINVAL, "pi and out_pi differ in rows");
  if (out_pi->num_cols > pi->num_cols) return fail(AMMSB_EINVAL, "more new communities than old ones");
  if (new_cols != out_pi->num_cols) return fail(AMMSB_EINVAL, "new_cols is not out_pi's num_cols");
  for (uint32_t b = 0; b < pi->num_blocks; ++b)
    for (uint32_t c = 0; c < out_pi->num_blocks; ++c)
      if (pi->blocks[b] == out_pi->blocks[c]) return fail(AMMSB_EINVAL, "pi and out_pi share a block");
  for (uint32_t c = 0; c < out_pi->num_blocks; ++c)
    if (misaligned(out_pi->blocks[c], 4)) return fail(AMMSB_EINVAL, "a block of out_pi is not 4-byte aligned");
  for (uint32_t b = 0; b < pi->num_blocks; ++b)
    if (misaligned(pi->blocks[b], 4)) return fail(AMMSB_EINVAL, "a block of pi is not 4-byte aligned");
  if (!phi_sum || !out_phi_sum) return fail(AMMSB_EINVAL, "phi_sum or out_phi_sum is NULL");
  if (!src) return fail(AMMSB_EINVAL, "src is NULL");
  if (drops && !emptied) return fail(AMMSB_EINVAL, "a dropping plan with emptied == NULL");
  if (misaligned(phi_sum, 4) || misaligned(out_phi_sum, 4) || misaligned(src, 4) || misaligned(src_off, 4) ||
      misaligned(emptied, 8))
    return fail(AMMSB_EINVAL, "a pointer is not aligned to its element");
  if (count >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (first > pi->num_rows || count > pi->num_rows - first) return fail(AMMSB_EINVAL, "row range past num_rows");
  if (count == 0) return AMMSB_OK;

  Rows a;
  a.pi = *pi;
  a.out = *out_pi;
  a.phi = phi_sum;
  a.out_phi = out_phi_sum;
  a.src_off = src_off;
  a.src = src;
  a.emptied = reinterpret_cast<unsigned long long*>(emptied);
  a.first = first;
  a.count = count;
  a.gshift = group_shift(pi->num_cols);
  a.drops = drops ? 1u : 0u;
  // a staged row is 4 K bytes and a block's rows share 64 KiB: four rows of at most 4096 columns, two of more
  const uint32_t threads = pi->num_cols > 4096 ? RD_BLOCK / 2 : RD_BLOCK;
  const uint32_t per_block = threads >> a.gshift;
  const size_t lds = (size_t)per_block * pi->num_cols * sizeof(float);
  const dim3 grid(persistent_grid(count, per_block)), block(threads);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const bool vec = pi->num_cols % 4 == 0 && pi_aligned;
  const char* name;
  if (!src_off && vec) { name = "reduce_select_v4"; hipLaunchKernelGGL(reduce_select_v4, grid, block, lds, s, a); }
  else if (!src_off) { name = "reduce_select_s1"; hipLaunchKernelGGL(reduce_select_s1, grid, block, lds, s, a); }
  else if (vec) { name = "reduce_merge_v4"; hipLaunchKernelGGL(reduce_merge_v4, grid, block, lds, s, a); }
  else { name = "reduce_merge_s1"; hipLaunchKernelGGL(reduce_merge_s1, grid, block, lds, s, a); }
  return launched(name);
}

extern "C" int ammsb_reduce_theta(const float* theta, const uint32_t* src_off, const uint32_t* src, uint32_t old_cols,
                                  uint32_t new_cols, float* out_theta, void* stream) {
  if (!theta || !out_theta || !src) return fail(AMMSB_EINVAL, "theta, out_theta or src is NULL");
  if (old_cols == 0 || old_cols > AMMSB_REDUCE_MAX_COLS || new_cols == 0) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (new_cols > old_cols) return fail(AMMSB_EINVAL, "more new communities than old ones");
  if (theta == out_theta) return fail(AMMSB_EINVAL, "theta and out_theta are the same buffer");
  if (misaligned(theta, 4) || misaligned(out_theta, 4) || misaligned(src, 4) || misaligned(src_off, 4))
    return fail(AMMSB_EINVAL, "a pointer is not aligned to its element");
  hipLaunchKernelGGL(reduce_theta, dim3(1), dim3(RD_BLOCK), 0, static_cast<hipStream_t>(stream), theta, src_off, src, new_cols,
                     out_theta);
  return launched("reduce_theta");
}
