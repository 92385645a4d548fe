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

#include "../../include/ammsb_linkcomm.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int LC_WAVES = 4;  // waves (= edges in flight) per block
constexpr int LC_BLOCK = 64 * LC_WAVES;
constexpr uint32_t NONE = AMMSB_LINKCOMM_NONE;

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

// The term of one column as a key half: its bits if it may take a slot, else -1.  Two multiplications in this order
// (-ffp-contract=off: no FMA); a NaN fails both comparisons.
__device__ __forceinline__ int term_bits(float q, float bk, float min_term) {
  const float t = q * bk;
  return (t > 0.0f && t >= min_term) ? __float_as_int(t) : -1;
}

// The winner of a round among the lanes' bests: false when nothing is left.
__device__ __forceinline__ bool round_winner(const Best& b, int& wbits, uint32_t& wcol) {
  wbits = wave_max_i32(b.bits);
  if (wbits < 0) return false;
  wcol = winner_col(b, wbits);
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
  sum = wave_sum_f32(sum);
  if (a.ids && lane < (int)a.T) {
    a.ids[p * a.T + lane] = lcol;
    a.terms[p * a.T + lane] = lbits < 0 ? 0.0f : __int_as_float(lbits);
  }
  if (lane == 0) {
    if (a.prob) a.prob[p] = ok ? sum + a.eps : -1.0f;
    if (a.sizes && ok) atomicAdd(&lds[lcol == NONE ? (uint32_t)a.pi.num_cols : lcol], 1u);
  }
}

// the block's counters: lds[0..K], one per community and lds[K] for "no community"
__device__ __forceinline__ void zero_sizes(const Args& a, uint32_t* lds) {
  if (a.sizes) zero_counters<LC_BLOCK>(lds, Through{a.pi.num_cols});
}

__device__ __forceinline__ void flush_sizes(const Args& a, const uint32_t* lds) {
  if (a.sizes) flush_counters<LC_BLOCK>(lds, Through{a.pi.num_cols}, a.sizes);
}

// ------------------------------------------------------------------------------------------ fast form
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
  r.pa = reinterpret_cast<const float4*>(postfit_row(a.pi, r.ok ? u : 0u)) + lane;
  r.pb = reinterpret_cast<const float4*>(postfit_row(a.pi, r.ok ? v : 0u)) + lane;
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
  zero_sizes(a, lds);
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
  flush_sizes(a, lds);
}

// ------------------------------------------------------------------------------------------ generic form
__global__ __launch_bounds__(LC_BLOCK) void linkcomm_generic(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, rows = (uint32_t)a.pi.num_rows;
  zero_sizes(a, lds);
  const uint64_t stride = (uint64_t)gridDim.x * LC_WAVES;
  for (uint64_t p = (uint64_t)blockIdx.x * LC_WAVES + (threadIdx.x >> 6); p < a.n; p += stride) {
    const u64 e = a.edges[p];
    const uint32_t u = (uint32_t)(e >> 32), v = (uint32_t)e;
    const bool ok = u < rows && v < rows;
    const float* pa = postfit_row(a.pi, ok ? u : 0u);
    const float* pb = postfit_row(a.pi, ok ? v : 0u);
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
  flush_sizes(a, lds);
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
  if (pi)
    if (const char* bad = check_rpm(pi, AMMSB_LINKCOMM_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
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
  const dim3 grid(persistent_grid(n, LC_WAVES)), block(LC_BLOCK);
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
  return launched(name);
}
