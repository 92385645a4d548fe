// libammsb_linkpred.so (include/ammsb_linkpred.h): p(a, b) = eps + sum_k pi[a,k] pi[b,k] (beta_k - eps) for a block of
// (query, candidate) pairs, the T most probable candidates per query, and a list of pairs.
//
// block / top: "Q query rows against a range of rows of pi" is a [Q, K] x [K, n] product, the one dense tile this model
// has, and it runs on the f32-input matrix core (v_mfma_f32_32x32x2_f32).  A block of 4 waves owns a tile of TQ queries
// x TC candidates; per chunk of 32 columns the query rows (scaled by w_k = beta_k - eps on their way into LDS) and the
// candidate rows are staged in LDS, the next chunk's global loads are issued before the current chunk's 32 MFMAs per
// wave.  Each output has ONE accumulator that starts at +0 and takes every k in one fixed order (columns past K are
// zeros in the staging: fma(0, 0, acc) leaves acc alone, and the final + eps maps a -0 to +0), so a score depends on the
// two rows, beta and eps only.  Two wave arrangements, same arithmetic: q128 (Q > 32) puts the 4 waves on 4 x 32
// queries sharing 64 candidates; q32 (Q <= 32, padded) puts them on 4 x 64 candidates sharing 32 queries, which is a
// stream over pi.
//
// top keeps, per wave and per query row, a list of the T best keys in LDS, sorted descending.  key = (score bits mapped
// so that they order as an unsigned integer) << 32 | ~id: larger = better score, then lower id; keys of one query are
// distinct, so "the T largest keys" is a set and no insertion order can change it.  The epilogue tests every score of
// the accumulator tile against the T-th key of its row; only the rare one that passes is looked at further (self, then
// the cuckoo probes, each passing lane for itself) and inserted by the whole wave (lane t holds slot t: one ballot
// finds the position).  A block walks a contiguous run of candidate tiles and leaves its lists in the workspace; linkpred_merge, a wave per query, folds
// the L lists of a query into ids / scores with the same insertion.
//
// pairs: a wave per pair, grid-stride; the next pair's first loads are issued before the current pair is reduced.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_linkpred.h"
#include "ammsb_dev.h"  // set_has(DevSet): the one copy of the cuckoo hash pair, with the fast_mod magic
#include "ammsb_postfit.h"

namespace {

using ammsb::DevSet;
using ammsb::dev_set;
using ammsb::set_has;
using f32x16 = __attribute__((ext_vector_type(16))) float;
typedef unsigned long long u64;

constexpr int LP_BLOCK = 256;        // 4 waves
constexpr int KC = 32;               // columns per chunk
constexpr int LDW = 36;              // LDS row stride in words: 16-byte aligned rows, 16 lanes x float4 hit 64 banks once
constexpr uint32_t NONE = AMMSB_LINKPRED_NONE;
constexpr uint32_t TARGET_GRID = MAX_GRID;  // what a persistent `top` grid aims for

// Is edge e in one of the exclusion sets?  Out of line: reached by the few candidates that pass a list's bar, and the
// epilogue's unrolled register loop stays small.
__device__ __attribute__((noinline)) bool excluded(const DevSet* sets, uint32_t nsets, uint64_t e) {
  if (nsets > 0 && set_has(sets[0], e)) return true;
  return nsets > 1 && set_has(sets[1], e);
}

// binary32 -> u32 that orders like the value (no NaN: pi, beta are finite), and back
__device__ __forceinline__ uint32_t ord_bits(float x) {
  const uint32_t b = __float_as_uint(x);
  return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float ord_value(uint32_t u) {
  return __uint_as_float(u ^ ((u >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

// One key into a descending list of T slots (lane t = slot t; 0 = empty, below every key).  The caller has checked
// key > lst[T - 1].  All 64 lanes call it with the same key.
__device__ __forceinline__ void list_insert(u64* lst, uint32_t T, u64 key, uint32_t lane) {
  const bool in = lane < T;
  const u64 mine = in ? lst[lane] : 0;
  const u64 prev = (in && lane > 0) ? lst[lane - 1] : 0;
  const uint32_t pos = (uint32_t)__popcll(__ballot(in && mine > key));
  if (in && lane >= pos) lst[lane] = lane == pos ? key : prev;
  // other lanes read these slots next (the T-th key, the next insertion's neighbours): DS operations of a wave are
  // ordered in hardware; this tells the compiler not to cache or move the plain LDS accesses across the store
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
}

__device__ __forceinline__ u64 read_lane_u64(u64 v, int l) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((u64)hi << 32) | lo;
}

struct TileArgs {
  ammsb_rpm pi;
  const float* beta;
  float eps;
  const uint32_t* queries;
  uint32_t Q;
  uint32_t cand_lo, cand_n;
  uint32_t nqt, tiles, tiles_per_part;
  float* out;      // block
  uint32_t T, L;   // top
  uint32_t nsets;
  DevSet sets[2];
  u64* ws;
};

// 4 columns k .. k+3 of a row (nullptr: a row that does not exist); columns >= K are zeros
template <bool VEC>
__device__ __forceinline__ float4 load4(const float* rowp, uint32_t k, uint32_t K) {
  float4 v = {0.f, 0.f, 0.f, 0.f};
  if (!rowp) return v;
  if constexpr (VEC) {
    if (k < K) v = *reinterpret_cast<const float4*>(rowp + k);
  } else {
    if (k < K) v.x = rowp[k];
    if (k + 1 < K) v.y = rowp[k + 1];
    if (k + 2 < K) v.z = rowp[k + 2];
    if (k + 3 < K) v.w = rowp[k + 3];
  }
  return v;
}

__device__ __forceinline__ float4 load_w4(const float* beta, float eps, uint32_t k, uint32_t K) {
  float4 w = {0.f, 0.f, 0.f, 0.f};
  if (k < K) w.x = beta[2 * k + 1] - eps;
  if (k + 1 < K) w.y = beta[2 * k + 3] - eps;
  if (k + 2 < K) w.z = beta[2 * k + 5] - eps;
  if (k + 3 < K) w.w = beta[2 * k + 7] - eps;
  return w;
}

// row of the 32x32 accumulator tile that register `reg` of a lane in half `h` holds (column = lane & 31)
__device__ __forceinline__ int acc_row(int reg, int h) { return (reg & 3) + 8 * (reg >> 2) + 4 * h; }

template <bool TOP, bool Q128, bool VEC>
__global__ __launch_bounds__(LP_BLOCK) void linkpred_tile(TileArgs a) {
  constexpr int TQ = Q128 ? 128 : 32, TC = Q128 ? 64 : 256;
  constexpr int PA = TQ / 32, PB = TC / 32;
  __shared__ __attribute__((aligned(16))) float As[TQ * LDW];
  __shared__ __attribute__((aligned(16))) float Bs[TC * LDW];
  __shared__ uint32_t qid[TQ];
  extern __shared__ u64 lists[];  // TOP: [4 waves][32 rows][T]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, h = lane >> 5, col = lane & 31;
  const int wq = Q128 ? wave : 0, wc = Q128 ? 0 : wave;
  const uint32_t K = (uint32_t)a.pi.num_cols, num_rows = (uint32_t)a.pi.num_rows;
  const uint32_t qt = blockIdx.x % a.nqt, part = blockIdx.x / a.nqt;
  const uint32_t T = a.T;
  u64* lst = lists + (size_t)wave * 32 * T;

  if (tid < TQ) {
    const uint32_t i = qt * TQ + tid;
    uint32_t q = NONE;
    if (i < a.Q) {
      q = a.queries[i];
      if (q >= num_rows) q = NONE;
    }
    qid[tid] = q;
  }
  if constexpr (TOP) {
    for (uint32_t s = lane; s < 32 * T; s += 64) lst[s] = 0;
  }
  __syncthreads();

  const int k4 = (tid & 7) * 4, r0 = tid >> 3;
  const float* pa[PA];
#pragma unroll
  for (int p = 0; p < PA; ++p) {
    const uint32_t q = qid[p * 32 + r0];
    pa[p] = q == NONE ? nullptr : postfit_row(a.pi, q);
  }
  const uint32_t nch = (K + KC - 1) / KC;
  const uint32_t tile_end = min(a.tiles, (part + 1) * a.tiles_per_part);

  for (uint32_t tile = part * a.tiles_per_part; tile < tile_end; ++tile) {
    const float* pb[PB];
#pragma unroll
    for (int p = 0; p < PB; ++p) {
      const uint32_t j = tile * TC + p * 32 + r0;
      pb[p] = j < a.cand_n ? postfit_row(a.pi, a.cand_lo + j) : nullptr;
    }
    f32x16 acc[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[nb][r] = 0.f;

    float4 ra[PA], rb[PB], w4;
    auto fetch = [&](uint32_t c) {
      const uint32_t k = c * KC + k4;
      w4 = load_w4(a.beta, a.eps, k, K);
#pragma unroll
      for (int p = 0; p < PA; ++p) ra[p] = load4<VEC>(pa[p], k, K);
#pragma unroll
      for (int p = 0; p < PB; ++p) rb[p] = load4<VEC>(pb[p], k, K);
    };
    fetch(0);
    for (uint32_t c = 0; c < nch; ++c) {
      __syncthreads();  // the previous chunk's fragments have been read by every wave
#pragma unroll
      for (int p = 0; p < PA; ++p) {
        const float4 s = {ra[p].x * w4.x, ra[p].y * w4.y, ra[p].z * w4.z, ra[p].w * w4.w};
        *reinterpret_cast<float4*>(&As[(p * 32 + r0) * LDW + k4]) = s;
      }
#pragma unroll
      for (int p = 0; p < PB; ++p) *reinterpret_cast<float4*>(&Bs[(p * 32 + r0) * LDW + k4]) = rb[p];
      __syncthreads();
      if (c + 1 < nch) fetch(c + 1);
      // lane (col, h) takes columns 16 h + s of the chunk at step s: A[row col][k], B[k][column col]
      float af[16], bf[16];
      const float4* ap = reinterpret_cast<const float4*>(&As[(wq * 32 + col) * LDW + 16 * h]);
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const float4 x = ap[v];
        af[4 * v] = x.x, af[4 * v + 1] = x.y, af[4 * v + 2] = x.z, af[4 * v + 3] = x.w;
      }
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float4* bp = reinterpret_cast<const float4*>(&Bs[(wc * 64 + nb * 32 + col) * LDW + 16 * h]);
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const float4 x = bp[v];
          bf[4 * v] = x.x, bf[4 * v + 1] = x.y, bf[4 * v + 2] = x.z, bf[4 * v + 3] = x.w;
        }
#pragma unroll
        for (int s = 0; s < 16; ++s) acc[nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[s], bf[s], acc[nb], 0, 0, 0);
      }
    }

    // ---- epilogue on the accumulator tile: rows = queries, column (lane & 31) = candidate
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const uint32_t j = tile * TC + wc * 64 + nb * 32 + col;
#pragma unroll
      for (int reg = 0; reg < 16; ++reg) {
        const int row = wq * 32 + acc_row(reg, h);
        const float score = acc[nb][reg] + a.eps;
        if constexpr (!TOP) {
          const uint32_t i = qt * TQ + row;
          if (i < a.Q && j < a.cand_n) a.out[(uint64_t)i * a.cand_n + j] = qid[row] == NONE ? -1.0f : score;
        } else {
          const int lrow = acc_row(reg, h);  // row of this wave's lists
          const uint32_t id = a.cand_lo + j;
          const u64 key = ((u64)ord_bits(score) << 32) | (uint32_t)~id;
          const bool pass = j < a.cand_n && qid[row] != NONE && key > lst[lrow * T + T - 1];
          // the few lanes that pass look at eligibility side by side (self, then the cuckoo probes: their loads
          // overlap across lanes); what is left is inserted one by one, wave-uniform
          bool elig = false;
          if (pass) {
            const uint32_t q = qid[row];
            elig = id != q;
            const u64 e = ((u64)(q < id ? q : id) << 32) | (q < id ? id : q);
            if (elig && a.nsets > 0) elig = !excluded(a.sets, a.nsets, e);
          }
          u64 mask = __ballot(elig);
          while (mask) {
            const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(mask));
            mask &= mask - 1;
            const u64 k = read_lane_u64(key, l);
            const int r = acc_row(reg, l >> 5);
            if (k <= lst[r * T + T - 1]) continue;  // an insertion of this loop has raised the bar
            list_insert(lst + r * T, T, k, lane);
          }
        }
      }
    }
  }

  if constexpr (TOP) {
    const uint32_t l = part * (Q128 ? 1 : 4) + wc;
    for (int r = 0; r < 32; ++r) {
      const uint32_t i = qt * TQ + wq * 32 + r;
      if (i < a.Q && (uint32_t)lane < T) a.ws[((uint64_t)i * a.L + l) * T + lane] = lst[r * T + lane];
    }
  }
}

// The L partial lists of query i -> ids[i, 0..T), scores[i, 0..T).  One wave per query.
__global__ __launch_bounds__(64) void linkpred_merge(const u64* ws, uint32_t L, uint32_t T, uint32_t* ids,
                                                      float* scores) {
  __shared__ u64 lst[AMMSB_LINKPRED_MAX_TOP];
  const uint32_t lane = threadIdx.x, i = blockIdx.x;
  lst[lane] = 0;
  const u64* base = ws + (uint64_t)i * L * T;
  const uint64_t n = (uint64_t)L * T;
  for (uint64_t off = 0; off < n; off += 64) {
    const u64 key = off + lane < n ? base[off + lane] : 0;
    u64 mask = __ballot(key > lst[T - 1]);
    while (mask) {
      const int l = __builtin_amdgcn_readfirstlane((int)__builtin_ctzll(mask));
      mask &= mask - 1;
      const u64 k = read_lane_u64(key, l);
      if (k <= lst[T - 1]) continue;
      list_insert(lst, T, k, lane);
    }
  }
  if (lane < T) {
    const u64 k = lst[lane];
    ids[(uint64_t)i * T + lane] = k ? ~(uint32_t)k : NONE;
    scores[(uint64_t)i * T + lane] = k ? ord_value((uint32_t)(k >> 32)) : 0.0f;
  }
}

// ------------------------------------------------------------------------------------------ pairs
struct PairArgs {
  ammsb_rpm pi;
  const float* beta;
  float eps;
  const u64* edges;
  uint64_t n;
  float* out;
};

struct PairHead {
  const float *pa, *pb;  // nullptr: an end out of range
  float4 x, y;           // VEC: columns 4 lane .. 4 lane + 3 of both rows, already requested
};

template <bool VEC>
__device__ __forceinline__ PairHead pair_head(const PairArgs& a, uint64_t p, uint32_t lane) {
  const u64 e = a.edges[p];
  const uint32_t u = (uint32_t)(e >> 32), v = (uint32_t)e, rows = (uint32_t)a.pi.num_rows;
  PairHead hd;
  const bool ok = u < rows && v < rows;
  hd.pa = ok ? postfit_row(a.pi, u) : nullptr;
  hd.pb = ok ? postfit_row(a.pi, v) : nullptr;
  if constexpr (VEC) {
    hd.x = load4<true>(hd.pa, 4 * lane, (uint32_t)a.pi.num_cols);
    hd.y = load4<true>(hd.pb, 4 * lane, (uint32_t)a.pi.num_cols);
  }
  return hd;
}

__device__ __forceinline__ float dot4(float4 x, float4 w, float4 y, float sum) {
  sum += (x.x * w.x) * y.x;
  sum += (x.y * w.y) * y.y;
  sum += (x.z * w.z) * y.z;
  sum += (x.w * w.w) * y.w;
  return sum;
}

template <bool VEC>
__global__ __launch_bounds__(LP_BLOCK) void linkpred_pairs(PairArgs a) {
  const uint32_t lane = threadIdx.x & 63, K = (uint32_t)a.pi.num_cols;
  const uint64_t stride = (uint64_t)gridDim.x * (LP_BLOCK / 64);
  uint64_t p = (uint64_t)blockIdx.x * (LP_BLOCK / 64) + (threadIdx.x >> 6);
  if (p >= a.n) return;
  PairHead nxt = pair_head<VEC>(a, p, lane);
  for (; p < a.n; p += stride) {
    const PairHead cur = nxt;
    if (p + stride < a.n) nxt = pair_head<VEC>(a, p + stride, lane);  // in flight while this pair is reduced
    float sum = 0.f;
    if (cur.pa) {
      if constexpr (VEC) {
        sum = dot4(cur.x, load_w4(a.beta, a.eps, 4 * lane, K), cur.y, sum);
        for (uint32_t k = 256 + 4 * lane; k < K; k += 256)
          sum = dot4(load4<true>(cur.pa, k, K), load_w4(a.beta, a.eps, k, K), load4<true>(cur.pb, k, K), sum);
      } else {
        for (uint32_t k = lane; k < K; k += 64) sum += (cur.pa[k] * (a.beta[2 * k + 1] - a.eps)) * cur.pb[k];
      }
    }
    // wave_sum_f32() written out: through the helper the kernel's prologue is scheduled in another order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) a.out[p] = cur.pa ? sum + a.eps : -1.0f;
  }
}

// ------------------------------------------------------------------------------------------ host
// the checks every entry shares; *vec: 16-byte loads are possible
int check_model(const ammsb_rpm* pi, const float* beta, float eps, bool* vec) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!beta) return fail(AMMSB_EINVAL, "beta is NULL");
  if (!(eps >= 0.0f && eps < 1.0f)) return fail(AMMSB_EINVAL, "epsilon outside [0, 1)");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_LINKPRED_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  *vec = aligned && pi->num_cols % 4 == 0;
  return AMMSB_OK;
}

int check_range(const ammsb_rpm* pi, uint64_t cand_lo, uint64_t cand_n) {
  if (cand_lo > pi->num_rows || cand_n > pi->num_rows - cand_lo)
    return fail(AMMSB_EINVAL, "candidate range past num_rows");
  // candidate indices inside a tile are 32-bit and the last tile may reach 255 past cand_n
  if (cand_n > 0xFFFFFFFFull - 256) return fail(AMMSB_ERANGE, "more than 2^32 - 257 candidates: cut the range");
  return AMMSB_OK;
}

struct Plan {
  bool q128;
  uint32_t nqt, tiles, tiles_per_part, nparts, L;
};

Plan make_plan(uint32_t Q, uint64_t cand_n, bool persistent) {
  Plan p;
  p.q128 = Q > 32;
  const uint32_t TQ = p.q128 ? 128 : 32, TC = p.q128 ? 64 : 256;
  p.nqt = (Q + TQ - 1) / TQ;
  p.tiles = (uint32_t)((cand_n + TC - 1) / TC);
  if (!persistent) {
    p.tiles_per_part = 1;
    p.nparts = p.tiles;
  } else {
    const uint32_t target = p.nqt >= TARGET_GRID ? 1u : TARGET_GRID / (p.nqt ? p.nqt : 1u);
    p.tiles_per_part = p.tiles ? (p.tiles + target - 1) / target : 1u;
    p.nparts = (p.tiles + p.tiles_per_part - 1) / p.tiles_per_part;
  }
  p.L = p.nparts * (p.q128 ? 1u : 4u);
  return p;
}

template <bool TOP>
const char* launch_tile(const Plan& p, bool vec, const TileArgs& a, size_t lds, hipStream_t s, hipError_t* err) {
  const dim3 grid(p.nqt * p.nparts), block(LP_BLOCK);
  const char* name;
#define LP_LAUNCH(Q128, VEC, NAME)                                                                              \
  do {                                                                                                          \
    name = NAME;                                                                                                \
    *err = lds > 0 ? hipFuncSetAttribute(reinterpret_cast<const void*>(&linkpred_tile<TOP, Q128, VEC>),         \
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)                  \
                   : hipSuccess;                                                                                \
    if (*err == hipSuccess) {                                                                                   \
      hipLaunchKernelGGL((linkpred_tile<TOP, Q128, VEC>), grid, block, lds, s, a);                              \
      *err = hipGetLastError();                                                                                 \
    }                                                                                                           \
  } while (0)
  if (p.q128) {
    if (vec) LP_LAUNCH(true, true, TOP ? "linkpred_top_mfma_q128_v4" : "linkpred_block_mfma_q128_v4");
    else LP_LAUNCH(true, false, TOP ? "linkpred_top_mfma_q128_v1" : "linkpred_block_mfma_q128_v1");
  } else {
    if (vec) LP_LAUNCH(false, true, TOP ? "linkpred_top_mfma_q32_v4" : "linkpred_block_mfma_q32_v4");
    else LP_LAUNCH(false, false, TOP ? "linkpred_top_mfma_q32_v1" : "linkpred_block_mfma_q32_v1");
  }
#undef LP_LAUNCH
  return name;
}

}  // namespace

extern "C" const char* ammsb_linkpred_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_linkpred_last_error(void) { return g_last_error; }

extern "C" uint64_t ammsb_linkpred_top_workspace_bytes(uint32_t Q, uint32_t T, uint64_t cand_n, uint64_t K) {
  (void)K;  // the query rows are staged in LDS, not in the workspace
  const Plan p = make_plan(Q, cand_n, true);
  const uint64_t b = (uint64_t)Q * p.L * T * sizeof(u64);
  return b < 16 ? 16 : b;
}

extern "C" int ammsb_linkpred_block(const ammsb_rpm* pi, const float* beta, float epsilon, const uint32_t* queries,
                                    uint32_t Q, uint64_t cand_lo, uint64_t cand_n, float* out, void* stream) {
  bool vec;
  int rc = check_model(pi, beta, epsilon, &vec);
  if (rc) return rc;
  if ((rc = check_range(pi, cand_lo, cand_n))) return rc;
  if (!queries) return fail(AMMSB_EINVAL, "queries is NULL");
  if (!out) return fail(AMMSB_EINVAL, "out is NULL");
  if (Q == 0 || cand_n == 0) return AMMSB_OK;
  const Plan p = make_plan(Q, cand_n, false);
  if ((uint64_t)p.nqt * p.nparts >> 31) return fail(AMMSB_ERANGE, "more than 2^31 tiles: cut the block");
  TileArgs a = {};
  a.pi = *pi;
  a.beta = beta;
  a.eps = epsilon;
  a.queries = queries;
  a.Q = Q;
  a.cand_lo = (uint32_t)cand_lo;
  a.cand_n = (uint32_t)cand_n;
  a.nqt = p.nqt, a.tiles = p.tiles, a.tiles_per_part = 1;
  a.out = out;
  hipError_t e;
  const char* name = launch_tile<false>(p, vec, a, 0, static_cast<hipStream_t>(stream), &e);
  if (e != hipSuccess) return hip_fail(name, e);
  g_last_kernel = name;
  return AMMSB_OK;
}

extern "C" int ammsb_linkpred_top(const ammsb_rpm* pi, const float* beta, float epsilon, const uint32_t* queries,
                                  uint32_t Q, uint32_t T, const ammsb_set* exclude0, const ammsb_set* exclude1,
                                  uint64_t cand_lo, uint64_t cand_n, uint32_t* ids, float* scores, void* workspace,
                                  uint64_t workspace_bytes, void* stream) {
  bool vec;
  int rc = check_model(pi, beta, epsilon, &vec);
  if (rc) return rc;
  if ((rc = check_range(pi, cand_lo, cand_n))) return rc;
  if (T == 0 || T > AMMSB_LINKPRED_MAX_TOP) return fail(AMMSB_EINVAL, "T outside 1..64");
  if (!queries) return fail(AMMSB_EINVAL, "queries is NULL");
  if (!ids || !scores) return fail(AMMSB_EINVAL, "ids or scores is NULL");
  const ammsb_set* ex[2] = {exclude0, exclude1};
  for (const ammsb_set* s : ex)
    if (s && (!s->slots || s->num_bins == 0 || s->prime_idx > 3)) return fail(AMMSB_EINVAL, "a malformed exclusion set");
  if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 15))
    return fail(AMMSB_EINVAL, "workspace NULL or not 16-byte aligned");
  if (workspace_bytes < ammsb_linkpred_top_workspace_bytes(Q, T, cand_n, pi->num_cols))
    return fail(AMMSB_EINVAL, "workspace too small (ammsb_linkpred_top_workspace_bytes)");
  if (Q == 0) return AMMSB_OK;
  const Plan p = make_plan(Q, cand_n, true);
  TileArgs a = {};
  a.pi = *pi;
  a.beta = beta;
  a.eps = epsilon;
  a.queries = queries;
  a.Q = Q;
  a.cand_lo = (uint32_t)cand_lo;
  a.cand_n = (uint32_t)cand_n;
  a.nqt = p.nqt, a.tiles = p.tiles, a.tiles_per_part = p.tiles_per_part;
  a.T = T, a.L = p.L;
  for (const ammsb_set* s : ex)
    if (s) a.sets[a.nsets++] = dev_set(*s);
  a.ws = static_cast<u64*>(workspace);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name = g_last_kernel;  // cand_n == 0: no tile kernel runs and the name of the last form stays
  hipError_t e;
  if (p.L > 0) {
    name = launch_tile<true>(p, vec, a, (size_t)4 * 32 * T * sizeof(u64), s, &e);
    if (e != hipSuccess) return hip_fail(name, e);
  }
  hipLaunchKernelGGL(linkpred_merge, dim3(Q), dim3(64), 0, s, a.ws, p.L, T, ids, scores);
  e = hipGetLastError();
  if (e != hipSuccess) return hip_fail("linkpred_merge", e);
  g_last_kernel = name;  // the tile form, not the merge
  return AMMSB_OK;
}

extern "C" int ammsb_linkpred_pairs(const ammsb_rpm* pi, const float* beta, float epsilon, const uint64_t* edges,
                                    uint64_t n, float* out, void* stream) {
  bool vec;
  const int rc = check_model(pi, beta, epsilon, &vec);
  if (rc) return rc;
  if (!edges) return fail(AMMSB_EINVAL, "edges is NULL");
  if (!out) return fail(AMMSB_EINVAL, "out is NULL");
  if (n == 0) return AMMSB_OK;
  PairArgs a = {*pi, beta, epsilon, reinterpret_cast<const u64*>(edges), n, out};
  const dim3 grid(persistent_grid(n, LP_BLOCK / 64)), block(LP_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name;
  if (vec) {
    name = "linkpred_pairs_v4";
    hipLaunchKernelGGL(linkpred_pairs<true>, grid, block, 0, s, a);
  } else {
    name = "linkpred_pairs_v1";
    hipLaunchKernelGGL(linkpred_pairs<false>, grid, block, 0, s, a);
  }
  return launched(name);
}
