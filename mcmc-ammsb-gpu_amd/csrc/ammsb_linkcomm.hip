// libammsb_linkcomm.so (include/ammsb_linkcomm.h): per edge (a, b) the T largest terms t_k = (pi[a,k] * pi[b,k]) * beta_k
// with their communities, p(a, b), and per community the number of edges whose largest term it holds.
//
// A wave owns an edge; blocks of 4 waves are persistent over a grid-stride of edges.  It is linkpred_pairs' two-row
// gather with readout_fast's selection on top: a term that is > 0 is a positive binary32, which orders as its bit
// pattern, and the key of (edge, k) is (term bits, ~k) -- larger = larger term, then lower community; keys of one edge
// are distinct, so "the T largest keys" is a set.  A round is every lane's best key BELOW the previous winner (nothing is
// marked as taken), a butterfly max over the term bits (DPP inside a row of 16, two shuffles across rows) and a min
// over the columns of the lanes that hold that value; rounds stop at the first one that finds nothing; lane t keeps
// round t's winner and lanes 0..T-1 store the edge's slots together.
//
// fast (K = 256 nv, 16-byte aligned blocks): lane l holds columns 256 i + 4 l + c of both rows as float4 registers, both
// rows' loads issued together.  The rows are dead once the terms are formed, so the NEXT edge's key and first loads are
// issued into the same registers before this edge's rounds.  K <= 1024: one chunk, beta of the lane's columns stays in
// registers across edges.  K > 1024 (v4_chunked): chunks of 1024 columns; the wave's running list of T keys (lane t =
// slot t) is offered to the rounds of the next chunk as one more element of lane t, and a chunk none of whose terms
// beats the list's T-th key costs one ballot.
// generic: lane l owns columns l, l + 64, ...; scalar loads; the two rows are read again each round (at most 64 KB that
// were just read).
//
// sizes: u32 counters private to the block in LDS (one ds_add per edge), flushed with one 64-bit vector atomic per
// non-zero counter when the block has run out of edges.  Integer adds only: nothing depends on arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ammsb_linkcomm.h"

namespace {

typedef unsigned long long u64;

constexpr int LC_WAVES = 4;  // waves (= edges in flight) per block
constexpr int LC_BLOCK = 64 * LC_WAVES;
constexpr int LC_MAX_GRID = 2048;  // 256 CUs x 8 blocks: past residency a block would only queue
constexpr uint32_t NONE = AMMSB_LINKCOMM_NONE;

thread_local const char* g_last_kernel = "";
thread_local char g_last_error[256] = "";

// TTRowPartitionedMatrix_Row with 64-bit offsets (rpm_row() of ammsb_dev.h): 32-bit block index, 64-bit element offset
__device__ __forceinline__ const float* lc_row(const ammsb_rpm& m, uint32_t row) {
  if (m.num_blocks == 1) return reinterpret_cast<const float*>(m.blocks[0]) + (uint64_t)row * m.num_cols;
  const uint32_t rib = (uint32_t)m.rows_in_block;
  const uint32_t blk = row / rib;
  return reinterpret_cast<const float*>(m.blocks[blk]) + (uint64_t)(row - blk * rib) * m.num_cols;
}

struct Args {
  ammsb_rpm pi;
  const float* beta;
  float eps;
  const u64* edges;
  uint64_t n;
  uint32_t T;  // rounds per edge: 1 in the sizes-only pass
  float min_term;
  uint32_t* ids;
  float* terms;
  float* prob;
  u64* sizes;
};

// ------------------------------------------------------------------------------------------ wave reductions
// Every lane ends with the maximum (csrc/ammsb_readout.hip): lanes of a row of 16 by DPP, rows by two shuffles.  All 64
// lanes are active wherever this is called (control flow around it is wave-uniform).
template <int CTRL>
__device__ __forceinline__ int dpp(int v) {
  return __builtin_amdgcn_update_dpp(v, v, CTRL, 0xf, 0xf, false);
}

__device__ __forceinline__ int wave_max_i32(int v) {
  v = max(v, dpp<0xB1>(v));   // quad_perm [1,0,3,2]
  v = max(v, dpp<0x4E>(v));   // quad_perm [2,3,0,1]
  v = max(v, dpp<0x141>(v));  // row_half_mirror
  v = max(v, dpp<0x140>(v));  // row_mirror
  v = max(v, __shfl_xor(v, 16, 64));
  v = max(v, __shfl_xor(v, 32, 64));
  return v;
}

struct Best {
  int bits;  // term bits of the lane's best eligible element; -1: none
  uint32_t col;
};

// The term of one column as a key half: its bits if it may take a slot, else -1.  Two multiplications in this order
// (-ffp-contract=off: no FMA); a NaN fails both comparisons.
__device__ __forceinline__ int term_bits(float q, float bk, float min_term) {
  const float t = q * bk;
  return (t > 0.0f && t >= min_term) ? __float_as_int(t) : -1;
}

// one element offered to a lane's running best, in ascending column order (strict >: the lower column wins in a lane)
template <bool FIRST>
__device__ __forceinline__ void offer(Best& b, int bits, uint32_t col, int pbits, uint32_t pcol) {
  const bool elig = FIRST || bits < pbits || (bits == pbits && col > pcol);
  if (elig && bits > b.bits) {
    b.bits = bits;
    b.col = col;
  }
}

// The winner of a round among the lanes' bests: false when nothing is left.
__device__ __forceinline__ bool round_winner(const Best& b, int& wbits, uint32_t& wcol) {
  wbits = wave_max_i32(b.bits);
  if (wbits < 0) return false;
  const uint64_t holders = __ballot(b.bits == wbits);
  if (__popcll(holders) == 1) {
    wcol = (uint32_t)__builtin_amdgcn_readlane((int)b.col, (int)__builtin_ctzll(holders));
  } else {  // the same bits in several lanes: the lowest column (columns are < 2^31, so ~col orders as an int)
    wcol = ~(uint32_t)wave_max_i32((int)~(b.bits == wbits ? b.col : 0x7FFFFFFFu));
  }
  return true;
}

// T rounds over what `scan(first, pbits, pcol)` offers; lane t ends with round t's winner in (lbits, lcol), the lanes
// past the last successful round with (-1, NONE).
template <class Scan>
__device__ __forceinline__ void select(Scan&& scan, uint32_t T, int lane, int& lbits, uint32_t& lcol) {
  int nbits = -1, wbits;
  uint32_t ncol = NONE, wcol;
  Best b = scan(true, 0, 0u);
  for (uint32_t t = 0;;) {
    if (!round_winner(b, wbits, wcol)) break;
    if (lane == (int)t) {
      nbits = wbits;
      ncol = wcol;
    }
    if (++t == T) break;
    b = scan(false, wbits, wcol);
  }
  lbits = nbits;
  lcol = ncol;
}

// What a wave leaves behind for edge p: lane t holds slot t, `sum` is the lane's share of sum_k q_k w_k.
__device__ __forceinline__ void finish(const Args& a, uint64_t p, bool ok, int lbits, uint32_t lcol, float sum, int lane,
                                       uint32_t* lds) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
  if (a.ids && lane < (int)a.T) {
    a.ids[p * a.T + lane] = lcol;
    a.terms[p * a.T + lane] = lbits < 0 ? 0.0f : __int_as_float(lbits);
  }
  if (lane == 0) {
    if (a.prob) a.prob[p] = ok ? sum + a.eps : -1.0f;
    if (a.sizes && ok) atomicAdd(&lds[lcol == NONE ? (uint32_t)a.pi.num_cols : lcol], 1u);
  }
}

__device__ __forceinline__ void zero_counters(const Args& a, uint32_t* lds) {
  if (!a.sizes) return;
  for (uint32_t s = threadIdx.x; s <= a.pi.num_cols; s += LC_BLOCK) lds[s] = 0;
  __syncthreads();
}

// block-private counters -> sizes[]: one vector atomic per non-zero counter
__device__ __forceinline__ void flush_counters(const Args& a, const uint32_t* lds) {
  if (!a.sizes) return;
  __syncthreads();
  for (uint32_t s = threadIdx.x; s <= a.pi.num_cols; s += LC_BLOCK) {
    const uint32_t c = lds[s];
    if (c) atomicAdd(&a.sizes[s], (u64)c);
  }
}

// ------------------------------------------------------------------------------------------ fast form
__device__ __forceinline__ float comp(const float4& q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }

template <int NV>
struct Rows {
  bool ok;               // both ends < num_rows
  const float4 *pa, *pb; // lane's first float4 of each row
  float4 x[NV], y[NV];   // the chunk in flight: columns 256 i + 4 lane + c of it
};

// nv float4 per row of the chunk that starts at float4 index `at` of the rows; registers past nv hold zeros (their
// terms are 0: never selected, and they add +-0 to the sum)
template <int NV>
__device__ __forceinline__ void load_chunk(Rows<NV>& r, uint32_t at, int nv) {
  const float4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    r.x[i] = zero;
    r.y[i] = zero;
    if (r.ok && i < nv) {
      r.x[i] = r.pa[at + i * 64];
      r.y[i] = r.pb[at + i * 64];
    }
  }
}

template <int NV>
__device__ __forceinline__ void head(const Args& a, uint64_t p, int lane, int nv, Rows<NV>& r) {
  const u64 e = a.edges[p];
  const uint32_t u = (uint32_t)(e >> 32), v = (uint32_t)e, rows = (uint32_t)a.pi.num_rows;
  r.ok = u < rows && v < rows;
  r.pa = reinterpret_cast<const float4*>(lc_row(a.pi, r.ok ? u : 0u)) + lane;
  r.pb = reinterpret_cast<const float4*>(lc_row(a.pi, r.ok ? v : 0u)) + lane;
  load_chunk<NV>(r, 0, nv);
}

template <int NV, bool CHUNKED>
__global__ __launch_bounds__(LC_BLOCK) void linkcomm_fast(Args a) {
  extern __shared__ uint32_t lds[];
  constexpr int NE = 4 * NV;  // elements per lane and chunk
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols;
  const int nvK = (int)(K >> 8);
  const int nch = CHUNKED ? (nvK + NV - 1) / NV : 1;
  zero_counters(a, lds);
  float bw[CHUNKED ? 1 : NE];  // one chunk: beta of the lane's columns, for every edge
  if constexpr (!CHUNKED) {
#pragma unroll
    for (int j = 0; j < NE; ++j) {
      const uint32_t col = 256u * (j >> 2) + 4u * lane + (j & 3);
      bw[j] = col < K ? a.beta[2 * col + 1] : 0.0f;
    }
  }
  const uint64_t stride = (uint64_t)gridDim.x * LC_WAVES;
  uint64_t p = (uint64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6);
  Rows<NV> r;
  if (p < a.n) head<NV>(a, p, lane, min(nvK, NV), r);
  for (; p < a.n; p += stride) {
    const bool ok = r.ok;
    int lbits = -1;       // the running list: lane t holds slot t
    uint32_t lcol = NONE;
    float sum = 0.0f;
    for (int c = 0; c < nch; ++c) {
      const uint32_t cb = (uint32_t)c * 256u * NV + 4u * lane;
      int tb[NE];
#pragma unroll
      for (int j = 0; j < NE; ++j) {
        float bk;
        if constexpr (CHUNKED) {
          const uint32_t col = cb + 256u * (j >> 2) + (j & 3);
          bk = col < K ? a.beta[2 * col + 1] : 0.0f;
        } else {
          bk = bw[j];
        }
        const float q = comp(r.x[j >> 2], j & 3) * comp(r.y[j >> 2], j & 3);
        tb[j] = term_bits(q, bk, a.min_term);
        sum += q * (bk - a.eps);
      }
      // the rows' registers are free: the next chunk, or the next edge's key and first chunk, before the rounds
      if (c + 1 < nch) load_chunk<NV>(r, (uint32_t)(c + 1) * 64u * NV, min(nvK - (c + 1) * NV, NV));
      else if (p + stride < a.n) head<NV>(a, p + stride, lane, min(nvK, NV), r);
      if constexpr (CHUNKED) {
        if (c > 0) {  // does any term of this chunk beat the list's T-th key?  (its columns are above the list's)
          const int kth = __builtin_amdgcn_readlane(lbits, (int)a.T - 1);
          bool any = false;
#pragma unroll
          for (int j = 0; j < NE; ++j) any = any || tb[j] > kth;
          if (!__ballot(any)) continue;
        }
      }
      const int obits = lbits;
      const uint32_t ocol = lcol;
      auto scan = [&](bool first, int pbits, uint32_t pcol) {
        Best b = {-1, NONE};
        if (first) {
          if constexpr (CHUNKED) offer<true>(b, obits, ocol, 0, 0u);  // lower columns than the chunk's: offered first
#pragma unroll
          for (int j = 0; j < NE; ++j) offer<true>(b, tb[j], cb + 256u * (j >> 2) + (j & 3), 0, 0u);
        } else {
          if constexpr (CHUNKED) offer<false>(b, obits, ocol, pbits, pcol);
#pragma unroll
          for (int j = 0; j < NE; ++j) offer<false>(b, tb[j], cb + 256u * (j >> 2) + (j & 3), pbits, pcol);
        }
        return b;
      };
      select(scan, a.T, lane, lbits, lcol);
    }
    finish(a, p, ok, lbits, lcol, sum, lane, lds);
  }
  flush_counters(a, lds);
}

// ------------------------------------------------------------------------------------------ generic form
__global__ __launch_bounds__(LC_BLOCK) void linkcomm_generic(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, rows = (uint32_t)a.pi.num_rows;
  zero_counters(a, lds);
  const uint64_t stride = (uint64_t)gridDim.x * LC_WAVES;
  for (uint64_t p = (uint64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); p < a.n; p += stride) {
    const u64 e = a.edges[p];
    const uint32_t u = (uint32_t)(e >> 32), v = (uint32_t)e;
    const bool ok = u < rows && v < rows;
    const float* pa = lc_row(a.pi, ok ? u : 0u);
    const float* pb = lc_row(a.pi, ok ? v : 0u);
    const uint32_t k_end = ok ? K : 0u;
    float sum = 0.0f;
    auto scan = [&](bool first, int pbits, uint32_t pcol) {
      Best b = {-1, NONE};
      for (uint32_t col = lane; col < k_end; col += 64) {
        const float bk = a.beta[2 * col + 1];
        const float q = pa[col] * pb[col];
        const int bits = term_bits(q, bk, a.min_term);
        if (first) {
          sum += q * (bk - a.eps);
          offer<true>(b, bits, col, 0, 0u);
        } else {
          offer<false>(b, bits, col, pbits, pcol);
        }
      }
      return b;
    };
    int lbits;
    uint32_t lcol;
    select(scan, a.T, lane, lbits, lcol);
    finish(a, p, ok, lbits, lcol, sum, lane, lds);
  }
  flush_counters(a, lds);
}

int fail(int code, const char* what) {
  snprintf(g_last_error, sizeof(g_last_error), "%s", what);
  return code;
}

}  // namespace

extern "C" const char* ammsb_linkcomm_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_linkcomm_last_error(void) { return g_last_error; }

extern "C" int ammsb_linkcomm_edges(const ammsb_rpm* pi, const float* beta, float epsilon, const uint64_t* edges,
                                    uint64_t n, uint32_t T, float min_term, uint32_t* ids, float* terms, float* prob,
                                    uint64_t* sizes, void* stream) {
  if (n > 0 && !pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (n > 0 && !beta) return fail(AMMSB_EINVAL, "beta is NULL");
  if (n > 0 && !edges) return fail(AMMSB_EINVAL, "edges is NULL");
  if (!ids != !terms) return fail(AMMSB_EINVAL, "ids and terms go together");
  if (!ids && !prob && !sizes) return fail(AMMSB_EINVAL, "no output");
  if (ids && (T == 0 || T > AMMSB_LINKCOMM_MAX_TOP)) return fail(AMMSB_EINVAL, "T outside 1..16");
  if (!(min_term >= 0.0f && min_term < INFINITY)) return fail(AMMSB_EINVAL, "min_term negative, NaN or infinite");
  if (!(epsilon >= 0.0f && epsilon < 1.0f)) return fail(AMMSB_EINVAL, "epsilon outside [0, 1)");
  bool aligned = true;
  if (pi) {
    const uint64_t K = pi->num_cols;
    if (K == 0 || K > AMMSB_LINKCOMM_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
    if (pi->num_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
    if (pi->num_blocks == 0 || pi->num_blocks > AMMSB_RPM_MAX_BLOCKS || pi->rows_in_block == 0 ||
        pi->rows_in_block >> 32 || pi->rows_in_block * pi->num_blocks < pi->num_rows ||
        (pi->num_rows && (pi->num_rows - 1) / pi->rows_in_block >= pi->num_blocks))
      return fail(AMMSB_EINVAL, "the blocks do not cover num_rows");
    for (uint32_t b = 0; b < pi->num_blocks; ++b) {
      if (!pi->blocks[b]) return fail(AMMSB_EINVAL, "a block pointer is NULL");
      aligned = aligned && (reinterpret_cast<uintptr_t>(pi->blocks[b]) & 15) == 0;
    }
  }
  if (n == 0) return AMMSB_OK;

  Args a;
  a.pi = *pi;
  a.beta = beta;
  a.eps = epsilon;
  a.edges = reinterpret_cast<const u64*>(edges);
  a.n = n;
  a.T = ids ? T : 1u;
  a.min_term = min_term;
  a.ids = ids;
  a.terms = terms;
  a.prob = prob;
  a.sizes = reinterpret_cast<u64*>(sizes);
  const uint64_t K = pi->num_cols;
  const uint64_t want = (n + LC_WAVES - 1) / LC_WAVES;
  const dim3 grid((unsigned)(want < (uint64_t)LC_MAX_GRID ? want : (uint64_t)LC_MAX_GRID)), block(LC_BLOCK);
  const size_t lds = sizes ? (size_t)(K + 1) * sizeof(uint32_t) : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name;
  if (K % 256 == 0 && aligned) {
    const unsigned nv = (unsigned)(K / 256);
    if (nv <= 1) { name = "linkcomm_fast_v1"; hipLaunchKernelGGL((linkcomm_fast<1, false>), grid, block, lds, s, a); }
    else if (nv <= 2) { name = "linkcomm_fast_v2"; hipLaunchKernelGGL((linkcomm_fast<2, false>), grid, block, lds, s, a); }
    else if (nv <= 4) { name = "linkcomm_fast_v4"; hipLaunchKernelGGL((linkcomm_fast<4, false>), grid, block, lds, s, a); }
    else { name = "linkcomm_fast_v4_chunked"; hipLaunchKernelGGL((linkcomm_fast<4, true>), grid, block, lds, s, a); }
  } else {
    name = "linkcomm_generic";
    hipLaunchKernelGGL(linkcomm_generic, grid, block, lds, s, a);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_last_error, sizeof(g_last_error), "%s: %s", name, hipGetErrorString(e));
    return AMMSB_EHIP;
  }
  g_last_kernel = name;
  return AMMSB_OK;
}
