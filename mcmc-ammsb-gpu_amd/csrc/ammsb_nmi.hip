// libammsb_nmi.so (include/ammsb_nmi.h): the pair pass of the overlapping NMI over the dense overlap[G, K], slab by
// slab, to one running minimum per ground-truth community and one per detected community.
//
//   nmi_begin                a thread per community: the unconditional entropies, and +inf into both running minima.
//   nmi_fast / nmi_generic   a persistent grid over tiles of T_ROWS rows x CHUNK columns, chunk-major, so that a block
//                    meets the same chunk in consecutive tiles.  A wave owns a row of the tile, lanes own 16 columns of
//                    the chunk: their d and H(Y_k) stay in registers while the block stays in the chunk, and so does a
//                    lane-private minimum per column, offered with one atomic per column when the block leaves the
//                    chunk.  The row's minimum is a wave butterfly and one atomic.  The next tile's row is requested
//                    before this one is worked on.  An entry whose pair cannot qualify (the shortcut of the header)
//                    costs its load and two compares; the others four logarithms in float64.
// The minima are non-negative doubles or +inf: their bits order as u64, and a u64 atomic minimum does not depend on the
// order of arrival.
//
// Which column a slot stands for: nmi_fast loads 16 bytes per lane, so slot j = 4 i + c of lane l is column
// 256 i + 4 l + c of the chunk; nmi_generic loads column 64 j + l.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_nmi.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int N_WAVES = 4;  // waves per block, a row of the tile each
constexpr int N_BLOCK = 64 * N_WAVES;
constexpr uint32_t T_ROWS = N_WAVES;
constexpr uint32_t CHUNK = 1024;  // columns of a tile: 16 per lane
constexpr int SLOTS = CHUNK / 64;
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr unsigned NMI_GRID = MAX_GRID / 4;  // two blocks per CU: eight waves a CU hold their rows and the next ones
constexpr u64 INF_BITS = 0x7FF0000000000000ull;

struct NmiArgs {
  const uint32_t* ov;  // [Gs, K]
  u64 g0, Gs, N;
  const uint32_t* tsize;  // [G]
  const u64* dsize;       // [K]
  uint32_t K;
  const double *HX, *HY;  // [G], [K]
  u64 *cx, *cy;           // the bits of c_truth [G] and c_detected [K]
};

// h(x) = -(x / N) log2(x / N): one division of the integer by N
__device__ __forceinline__ double h_of(u64 x, double n) {
  if (x == 0) return 0.0;
  const double p = (double)x / n;
  return -(p * log2(p));
}

// H of a community of s nodes; s >= N: 0
__device__ __forceinline__ double entropy_of(u64 s, u64 N) {
  if (s >= N) return 0.0;
  const double n = (double)N;
  return h_of(s, n) + h_of(N - s, n);
}

__global__ __launch_bounds__(N_BLOCK) void nmi_begin(u64 N, const uint32_t* tsize, u64 G, const u64* dsize, uint32_t K,
                                                      double* HX, double* HY, u64* cx, u64* cy) {
  const u64 stride = (u64)gridDim.x * N_BLOCK;
  for (u64 i = (u64)blockIdx.x * N_BLOCK + threadIdx.x; i < G + K; i += stride) {
    if (i < G) {
      HX[i] = entropy_of(tsize[i], N);
      cx[i] = INF_BITS;
    } else {
      const u64 k = i - G;
      HY[k] = entropy_of(dsize[k], N);
      cy[k] = INF_BITS;
    }
  }
}

template <bool FAST>
__device__ __forceinline__ uint32_t col_of(uint32_t ch, int j, uint32_t lane) {
  return ch * CHUNK + slot_col(FAST, (uint32_t)j, lane);
}

// the lane's 16 entries of one row of one chunk; a slot past the row holds 0
template <bool FAST>
__device__ __forceinline__ void load_row(const uint32_t* row, uint32_t ch, uint32_t K, uint32_t lane, uint32_t (&o)[SLOTS]) {
  if (FAST) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const uint32_t c0 = ch * CHUNK + 256u * i + 4u * lane;  // K % 4 == 0: the four columns are inside or outside
      uint4 v = {0u, 0u, 0u, 0u};
      if (c0 < K) v = *reinterpret_cast<const uint4*>(row + c0);
      o[4 * i] = v.x;
      o[4 * i + 1] = v.y;
      o[4 * i + 2] = v.z;
      o[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
      const uint32_t c = ch * CHUNK + 64u * j + lane;
      o[j] = c < K ? row[c] : 0u;
    }
  }
}

template <bool FAST>
__device__ __forceinline__ void nmi_body(const NmiArgs& a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t K = a.K;
  const u64 rtiles = (a.Gs + T_ROWS - 1) / T_ROWS, ntiles = rtiles * ((K + CHUNK - 1) / CHUNK);
  const double n = (double)a.N, inf = __longlong_as_double((long long)INF_BITS);
  const long long half = (long long)((a.N + 1) >> 1);  // 2 (t + d) >= N  <=>  d >= ceil(N / 2) - t

  uint32_t cur = NONE;   // the chunk the registers below stand for
  uint32_t d[SLOTS];     // d_k, saturated at 2^32 - 1 (d >= N never qualifies and has H = 0 either way)
  double hy[SLOTS], cmin[SLOTS];
  auto flush = [&]() {
    if (cur == NONE) return;
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) {
      const uint32_t c = col_of<FAST>(cur, j, lane);
      if (cmin[j] < inf && c < K) atomicMin(&a.cy[c], (u64)__double_as_longlong(cmin[j]));
    }
  };

  uint32_t o[SLOTS], on[SLOTS];
  u64 tile = blockIdx.x;
  auto request = [&](u64 tl, uint32_t (&dst)[SLOTS]) {
    const u64 row = (tl % rtiles) * T_ROWS + wave;
    if (tl < ntiles && row < a.Gs) {
      load_row<FAST>(a.ov + row * K, (uint32_t)(tl / rtiles), K, lane, dst);
    } else {
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) dst[j] = 0;
    }
  };
  request(tile, o);
  for (; tile < ntiles; tile += gridDim.x) {
    const uint32_t ch = (uint32_t)(tile / rtiles);
    const u64 row = (tile % rtiles) * T_ROWS + wave;
    if (ch != cur) {
      flush();
      cur = ch;
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) {
        const uint32_t c = col_of<FAST>(ch, j, lane);
        const u64 dk = c < K ? a.dsize[c] : 0;
        d[j] = dk > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)dk;
        hy[j] = c < K ? a.HY[c] : 0.0;
        cmin[j] = inf;
      }
    }
    request(tile + gridDim.x, on);
    if (row < a.Gs) {  // (wave-uniform)
      const u64 g = a.g0 + row;
      const long long t = (long long)a.tsize[g];
      const double hx = a.HX[g];
      const long long need_d = half - t;
      double rmin = inf;
#pragma unroll
      for (int j = 0; j < SLOTS; ++j) {
        const long long oo = (long long)o[j], dd = (long long)d[j];
        // the shortcut: o == 0 and 2 (t + d) < N cannot qualify, unless t == d == 0
        if ((oo != 0 || dd >= need_d || (t | dd) == 0) && col_of<FAST>(ch, j, lane) < K) {
          const long long n10 = t - oo, n01 = dd - oo, n00 = (long long)a.N - t - dd + oo;
          if (n10 >= 0 && n01 >= 0 && n00 >= 0) {
            const double lhs = h_of((u64)oo, n) + h_of((u64)n00, n), rhs = h_of((u64)n01, n) + h_of((u64)n10, n);
            if (lhs >= rhs) {
              const double J = lhs + rhs, vy = J - hy[j], vx = J - hx;
              const double cy_ = vy > 0.0 ? vy : 0.0, cx_ = vx > 0.0 ? vx : 0.0;
              rmin = cy_ < rmin ? cy_ : rmin;
              cmin[j] = cx_ < cmin[j] ? cx_ : cmin[j];
            }
          }
        }
      }
      if (__any(rmin < inf)) {  // (all 64 lanes are here)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const double other = __shfl_xor(rmin, off, 64);
          rmin = other < rmin ? other : rmin;
        }
        if (lane == 0) atomicMin(&a.cx[g], (u64)__double_as_longlong(rmin));
      }
    }
#pragma unroll
    for (int j = 0; j < SLOTS; ++j) o[j] = on[j];
  }
  flush();
}

__global__ __launch_bounds__(N_BLOCK) void nmi_fast(NmiArgs a) { nmi_body<true>(a); }
__global__ __launch_bounds__(N_BLOCK) void nmi_generic(NmiArgs a) { nmi_body<false>(a); }

const char* check_shape(uint64_t N, uint64_t G, uint32_t K) {
  if (K == 0 || K > AMMSB_NMI_MAX_COLS) return "num_cols outside 1..8192";
  if (N == 0 || (N >> 32)) return "num_nodes outside 1..2^32 - 1";
  if (G >> 31) return "2^31 communities or more";
  return nullptr;
}

}  // namespace

extern "C" const char* ammsb_nmi_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_nmi_last_error(void) { return g_last_error; }

extern "C" int ammsb_nmi_begin(uint64_t num_nodes, const uint32_t* truth_size, uint64_t num_truth,
                               const uint64_t* detected_size, uint32_t num_cols, double* H_truth, double* H_detected,
                               double* c_truth, double* c_detected, void* stream) {
  if (!detected_size || !H_detected || !c_detected) return fail(AMMSB_EINVAL, "a detected-side array is NULL");
  if (num_truth > 0 && (!truth_size || !H_truth || !c_truth)) return fail(AMMSB_EINVAL, "a truth-side array is NULL");
  if (const char* bad = check_shape(num_nodes, num_truth, num_cols)) return fail(AMMSB_EINVAL, bad);
  hipLaunchKernelGGL(nmi_begin, dim3(persistent_grid(num_truth + num_cols, N_BLOCK)), dim3(N_BLOCK), 0,
                     static_cast<hipStream_t>(stream), (u64)num_nodes, truth_size, (u64)num_truth,
                     reinterpret_cast<const u64*>(detected_size), num_cols, H_truth, H_detected,
                     reinterpret_cast<u64*>(c_truth), reinterpret_cast<u64*>(c_detected));
  return launched("nmi_begin");
}

extern "C" int ammsb_nmi_accumulate(const uint32_t* overlap, uint64_t g0, uint64_t num_slab_rows, uint64_t num_nodes,
                                    const uint32_t* truth_size, uint64_t num_truth, const uint64_t* detected_size,
                                    uint32_t num_cols, const double* H_truth, const double* H_detected, double* c_truth,
                                    double* c_detected, void* stream) {
  if (!detected_size || !H_detected || !c_detected) return fail(AMMSB_EINVAL, "a detected-side array is NULL");
  if (num_truth > 0 && (!truth_size || !H_truth || !c_truth)) return fail(AMMSB_EINVAL, "a truth-side array is NULL");
  if (const char* bad = check_shape(num_nodes, num_truth, num_cols)) return fail(AMMSB_EINVAL, bad);
  if (g0 > num_truth || num_slab_rows > num_truth - g0) return fail(AMMSB_EINVAL, "the slab ends past the last community");
  if (num_slab_rows > 0 && !overlap) return fail(AMMSB_EINVAL, "overlap is NULL");
  if (num_slab_rows == 0) return AMMSB_OK;

  NmiArgs a;
  a.ov = overlap;
  a.g0 = g0;
  a.Gs = num_slab_rows;
  a.N = num_nodes;
  a.tsize = truth_size;
  a.dsize = reinterpret_cast<const u64*>(detected_size);
  a.K = num_cols;
  a.HX = H_truth;
  a.HY = H_detected;
  a.cx = reinterpret_cast<u64*>(c_truth);
  a.cy = reinterpret_cast<u64*>(c_detected);
  const uint64_t tiles = (num_slab_rows + T_ROWS - 1) / T_ROWS * ((num_cols + CHUNK - 1) / CHUNK);
  const dim3 grid((unsigned)(tiles < NMI_GRID ? tiles : NMI_GRID)), block(N_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_cols % 4 == 0 && (reinterpret_cast<uintptr_t>(overlap) & 15) == 0) {
    hipLaunchKernelGGL(nmi_fast, grid, block, 0, s, a);
    return launched("nmi_fast");
  }
  hipLaunchKernelGGL(nmi_generic, grid, block, 0, s, a);
  return launched("nmi_generic");
}
