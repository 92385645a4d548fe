// libammsb_readout.so (include/ammsb_readout.h): the T strongest communities of every pi row, the number of columns at
// or above a threshold, and per-community sizes -- one streaming pass over the rows.
//
// A wave owns a row; blocks of 4 waves are persistent over a grid-stride of rows.  Selection is T rounds of a
// wave-wide arg-max over (value, column): non-negative binary32 orders as its bit pattern, and "the largest element
// that comes AFTER the previous winner" -- value smaller, or equal with a larger column -- needs no element to be
// marked as taken, so the row stays read-only (registers in the fast form, cache-resident memory in the generic one).
// A round is: every lane's best eligible element (ascending columns, strict >, so the lower column wins inside a lane),
// a butterfly max over the value bits, and a min over the columns of the lanes that hold that value (one readlane when
// it is a single lane, the usual case).  Rounds stop as soon as the wave maximum is < thr or the row is exhausted;
// lane t keeps round t's result and lanes 0..T-1 store the row's slots together.
// The first round also counts: count[a] is a popcount over the ballot of (value >= thr) per column group, sizes[] are
// u32 counters private to the block in LDS (one ds_add per lane that passes), flushed with one 64-bit vector atomic per
// non-zero counter when the block has run out of rows.  Integer adds only: nothing depends on arrival order.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_readout.h"
#include "ammsb_postfit.h"

namespace {

constexpr int RO_WAVES = 4;               // waves (= rows in flight) per block
constexpr int RO_BLOCK = 64 * RO_WAVES;
constexpr uint32_t NONE = AMMSB_READOUT_NONE;

// The winner of a round among the lanes' bests: false when nothing is left or the maximum is below the threshold.
__device__ __forceinline__ bool round_winner(const Best& b, float thr, int& wbits, uint32_t& wcol) {
  wbits = wave_max_i32(b.bits);
  if (wbits < 0 || __int_as_float(wbits) < thr) return false;
  wcol = winner_col(b, wbits);
  return true;
}

struct Out {
  uint32_t* ids;
  float* weights;
  uint32_t* count;
  uint32_t T;  // 0: sizes only
};

// What a wave does with one row once `scan` can produce the lanes' bests: scan(first, pbits, pcol, cnt) returns Best;
// the first call also adds the row's count into cnt and feeds the block's size counters.
template <class Scan>
__device__ __forceinline__ void select_row(Scan&& scan, uint64_t r, const Out& o, float thr, int lane) {
  uint32_t cnt = 0;
  Best b = scan(true, 0, 0u, cnt);
  if (o.T == 0) return;
  uint32_t my_id = NONE;
  int my_w = 0;
  int wbits;
  uint32_t wcol;
  for (uint32_t t = 0;;) {
    if (!round_winner(b, thr, wbits, wcol)) break;
    if (lane == (int)t) {
      my_id = wcol;
      my_w = wbits;
    }
    if (++t == o.T) break;
    uint32_t unused = 0;
    b = scan(false, wbits, wcol, unused);
  }
  if (lane < (int)o.T) {
    o.ids[r * o.T + lane] = my_id;
    o.weights[r * o.T + lane] = __int_as_float(my_w);
  }
  if (lane == 0) o.count[r] = cnt;
}

struct Args {
  ammsb_rpm pi;
  const uint32_t* nodes;
  uint64_t row_lo, n_rows;
  float thr;
  Out out;
  unsigned long long* sizes;
};

// ------------------------------------------------------------------------------------------ fast form
// K = 256 nv, nv <= NV: lane l holds columns 256 i + 4 l + c (i < nv, c < 4) as NV float4 registers; registers past nv
// hold bit pattern -1 (a NaN as a float: never >= thr; as an int below every value: never selected).  The size counter
// of register slot j = 4 i + c of lane l is lds[64 j + l]: a wave's ds_add touches 64 consecutive words.
template <int NV>
__device__ __forceinline__ void load_row(const Args& a, uint64_t r, int nv, int lane, uint32_t num_rows, float4 (&v)[NV],
                                         bool& ok) {
  const uint32_t row = a.nodes ? a.nodes[r] : (uint32_t)(a.row_lo + r);
  ok = row < num_rows;
  const float4 none = {__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)};
  const float4* p = reinterpret_cast<const float4*>(postfit_row(a.pi, ok ? row : 0u)) + lane;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = none;
    if (ok && i < nv) v[i] = p[i * 64];
  }
}

// the column whose size counter is lds[s]
__device__ __forceinline__ uint32_t fast_col_of(uint32_t s) {
  const uint32_t j = s >> 6, l = s & 63;
  return 256 * (j >> 2) + 4 * l + (j & 3);
}

template <int NV>
__global__ __launch_bounds__(RO_BLOCK) void readout_fast(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const int nv = (int)(a.pi.num_cols >> 8);
  const uint32_t num_rows = (uint32_t)a.pi.num_rows;
  unsigned long long* const sizes = a.sizes;
  const bool do_sizes = sizes != nullptr;
  if (do_sizes) zero_counters<RO_BLOCK>(lds, a.pi.num_cols);
  const uint64_t stride = (uint64_t)gridDim.x * RO_WAVES;
  uint64_t r = (uint64_t)blockIdx.x * RO_WAVES + (threadIdx.x >> 6);
  // small rows: the next row's loads are issued before this row's rounds (the other waves of the SIMD cover the rest)
  constexpr bool PREFETCH = NV <= 4;
  float4 v[NV], nxt[PREFETCH ? NV : 1];
  bool ok = false, nxt_ok = false;
  if (r < a.n_rows) load_row<NV>(a, r, nv, lane, num_rows, v, ok);
  for (; r < a.n_rows; r += stride) {
    if constexpr (PREFETCH) {
      if (r + stride < a.n_rows) load_row<NV>(a, r + stride, nv, lane, num_rows, nxt, nxt_ok);
    }
    auto scan = [&](bool first, int pbits, uint32_t pcol, uint32_t& cnt) {
      Best b = {-1, NONE};
      if (first) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const float e = comp(v[i], c);
            const bool pass = e >= a.thr;
            cnt += (uint32_t)__popcll(__ballot(pass));
            if (do_sizes && pass) atomicAdd(&lds[(4 * i + c) * 64 + lane], 1u);
            offer<true>(b, __float_as_int(e), (uint32_t)(256 * i + 4 * lane + c), 0, 0u);
          }
        }
      } else {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
#pragma unroll
          for (int c = 0; c < 4; ++c)
            offer<false>(b, __float_as_int(comp(v[i], c)), (uint32_t)(256 * i + 4 * lane + c), pbits, pcol);
        }
      }
      return b;
    };
    select_row(scan, r, a.out, a.thr, lane);
    if constexpr (PREFETCH) {
#pragma unroll
      for (int i = 0; i < NV; ++i) v[i] = nxt[i];
      ok = nxt_ok;
    } else {
      if (r + stride < a.n_rows) load_row<NV>(a, r + stride, nv, lane, num_rows, v, ok);
    }
  }
  if (do_sizes)
    flush_counters<RO_BLOCK, fast_col_of>(lds, (uint32_t)a.pi.num_cols, sizes);
}

// ------------------------------------------------------------------------------------------ generic form
// any 1 <= K <= 8192: lane l owns columns l, l + 64, ...; scalar loads, the row is read again each round (it is at most
// 32 KB and was just read, so the rounds after the first come out of the cache).  Size counter of column k: lds[k].
__global__ __launch_bounds__(RO_BLOCK) void readout_generic(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols;
  const uint32_t num_rows = (uint32_t)a.pi.num_rows;
  unsigned long long* const sizes = a.sizes;
  const bool do_sizes = sizes != nullptr;
  if (do_sizes) zero_counters<RO_BLOCK>(lds, K);
  const uint64_t stride = (uint64_t)gridDim.x * RO_WAVES;
  for (uint64_t r = (uint64_t)blockIdx.x * RO_WAVES + (threadIdx.x >> 6); r < a.n_rows; r += stride) {
    const uint32_t row = a.nodes ? a.nodes[r] : (uint32_t)(a.row_lo + r);
    const bool ok = row < num_rows;
    const float* p = postfit_row(a.pi, ok ? row : 0u);
    const uint32_t k_end = ok ? K : 0u;
    auto scan = [&](bool first, int pbits, uint32_t pcol, uint32_t& cnt) {
      Best b = {-1, NONE};
      // wave-uniform trip count (the ballot below needs every lane): columns base + lane, base = 0, 64, ...
      for (uint32_t base = 0; base < k_end; base += 64) {
        const uint32_t col = base + lane;
        const bool in = col < k_end;
        const float e = in ? p[col] : __int_as_float(-1);
        if (first) {
          const bool pass = e >= a.thr;
          cnt += (uint32_t)__popcll(__ballot(pass));
          if (do_sizes && pass) atomicAdd(&lds[col], 1u);
          offer<true>(b, __float_as_int(e), col, 0, 0u);
        } else {
          offer<false>(b, __float_as_int(e), col, pbits, pcol);
        }
      }
      return b;
    };
    select_row(scan, r, a.out, a.thr, lane);
  }
  if (do_sizes) flush_counters<RO_BLOCK>(lds, K, sizes);
}

}  // namespace

extern "C" const char* ammsb_readout_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_readout_last_error(void) { return g_last_error; }

extern "C" int ammsb_readout_top(const ammsb_rpm* pi, const uint32_t* nodes, uint64_t row_lo, uint64_t n_rows, uint32_t T,
                                 float thr, uint32_t* ids, float* weights, uint32_t* count, uint64_t* sizes,
                                 void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  const bool tops = ids && weights && count;
  if (!tops && (ids || weights || count)) return fail(AMMSB_EINVAL, "ids, weights and count go together");
  if (!tops && !sizes) return fail(AMMSB_EINVAL, "no output");
  if (tops && (T == 0 || T > AMMSB_READOUT_MAX_TOP)) return fail(AMMSB_EINVAL, "T outside 1..16");
  if (!(thr >= 0.0f)) return fail(AMMSB_EINVAL, "thr negative or NaN");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_READOUT_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (n_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (nodes ? row_lo != 0 : (row_lo > pi->num_rows || n_rows > pi->num_rows - row_lo))
    return fail(AMMSB_EINVAL, nodes ? "a node list with row_lo != 0" : "row range past num_rows");
  if (n_rows == 0) return AMMSB_OK;

  Args a;
  a.pi = *pi;
  a.nodes = nodes;
  a.row_lo = row_lo;
  a.n_rows = n_rows;
  a.thr = thr;
  a.out = {ids, weights, count, tops ? T : 0u};
  a.sizes = reinterpret_cast<unsigned long long*>(sizes);
  const uint64_t K = pi->num_cols;
  const dim3 grid(persistent_grid(n_rows, RO_WAVES)), block(RO_BLOCK);
  const size_t lds = sizes ? (size_t)K * sizeof(uint32_t) : 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const char* name;
  if (K % 256 == 0 && aligned) {
    const unsigned nv = (unsigned)(K / 256);
    if (nv <= 1) { name = "readout_fast<1>"; hipLaunchKernelGGL(readout_fast<1>, grid, block, lds, s, a); }
    else if (nv <= 2) { name = "readout_fast<2>"; hipLaunchKernelGGL(readout_fast<2>, grid, block, lds, s, a); }
    else if (nv <= 4) { name = "readout_fast<4>"; hipLaunchKernelGGL(readout_fast<4>, grid, block, lds, s, a); }
    else if (nv <= 8) { name = "readout_fast<8>"; hipLaunchKernelGGL(readout_fast<8>, grid, block, lds, s, a); }
    else if (nv <= 16) { name = "readout_fast<16>"; hipLaunchKernelGGL(readout_fast<16>, grid, block, lds, s, a); }
    else { name = "readout_fast<32>"; hipLaunchKernelGGL(readout_fast<32>, grid, block, lds, s, a); }
  } else {
    name = "readout_generic";
    hipLaunchKernelGGL(readout_generic, grid, block, lds, s, a);
  }
  return launched(name);
}
