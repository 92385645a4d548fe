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
#include <stdio.h>

#include "../../include/ammsb_readout.h"

namespace {

constexpr int RO_WAVES = 4;               // waves (= rows in flight) per block
constexpr int RO_BLOCK = 64 * RO_WAVES;
constexpr int RO_MAX_GRID = 2048;         // 256 CUs x 8 blocks: past residency a block would only queue
constexpr uint32_t NONE = AMMSB_READOUT_NONE;

thread_local const char* g_last_kernel = "";
thread_local char g_last_error[256] = "";

// TTRowPartitionedMatrix_Row with 64-bit offsets (the few lines of rpm_row() in ammsb_dev.h: row indices are vertex
// ids, so the block index is a 32-bit division; the element offset is 64-bit)
__device__ __forceinline__ const float* ro_row(const ammsb_rpm& m, uint32_t row) {
  if (m.num_blocks == 1) return reinterpret_cast<const float*>(m.blocks[0]) + (uint64_t)row * m.num_cols;
  const uint32_t rib = (uint32_t)m.rows_in_block;
  const uint32_t blk = row / rib;
  return reinterpret_cast<const float*>(m.blocks[blk]) + (uint64_t)(row - blk * rib) * m.num_cols;
}

// ------------------------------------------------------------------------------------------ wave reductions
// Every lane ends with the maximum.  Lanes 0..15 of each row of 16 by DPP (two quad permutes, then the mirrors pair
// quads and halves: a max does not care which partner it meets, only that the groups merge), rows by two shuffles.
// All 64 lanes are active wherever this is called (control flow around it is wave-uniform).
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
  int bits;      // value bits of the lane's best eligible element; -1: none
  uint32_t col;
};

// one element offered to a lane's running best, in ascending column order
template <bool FIRST>
__device__ __forceinline__ void offer(Best& b, int bits, uint32_t col, int pbits, uint32_t pcol) {
  const bool elig = FIRST || bits < pbits || (bits == pbits && col > pcol);
  if (elig && bits > b.bits) {
    b.bits = bits;
    b.col = col;
  }
}

// The winner of a round among the lanes' bests: false when nothing is left or the maximum is below the threshold.
__device__ __forceinline__ bool round_winner(const Best& b, float thr, int& wbits, uint32_t& wcol) {
  wbits = wave_max_i32(b.bits);
  if (wbits < 0 || __int_as_float(wbits) < thr) return false;
  const uint64_t holders = __ballot(b.bits == wbits);
  if (__popcll(holders) == 1) {
    wcol = (uint32_t)__builtin_amdgcn_readlane((int)b.col, (int)__builtin_ctzll(holders));
  } else {  // the same value in several lanes: the lowest column (columns are < 2^31, so ~col orders as an int)
    wcol = ~(uint32_t)wave_max_i32((int)~(b.bits == wbits ? b.col : 0x7FFFFFFFu));
  }
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

// block-private size counters -> sizes[]: one vector atomic per non-zero counter
template <class ColOf>
__device__ __forceinline__ void flush_sizes(const uint32_t* lds, uint32_t slots, unsigned long long* sizes, ColOf&& col_of) {
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < slots; s += RO_BLOCK) {
    const uint32_t c = lds[s];
    if (c) atomicAdd(&sizes[col_of(s)], (unsigned long long)c);
  }
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
__device__ __forceinline__ float comp(const float4& q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }

template <int NV>
__device__ __forceinline__ void load_row(const Args& a, uint64_t r, int nv, int lane, uint32_t num_rows, float4 (&v)[NV],
                                         bool& ok) {
  const uint32_t row = a.nodes ? a.nodes[r] : (uint32_t)(a.row_lo + r);
  ok = row < num_rows;
  const float4 none = {__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1)};
  const float4* p = reinterpret_cast<const float4*>(ro_row(a.pi, ok ? row : 0u)) + lane;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    v[i] = none;
    if (ok && i < nv) v[i] = p[i * 64];
  }
}

template <int NV>
__global__ __launch_bounds__(RO_BLOCK) void readout_fast(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const int nv = (int)(a.pi.num_cols >> 8);
  const uint32_t num_rows = (uint32_t)a.pi.num_rows;
  const bool do_sizes = a.sizes != nullptr;
  if (do_sizes) {
    for (uint32_t s = threadIdx.x; s < a.pi.num_cols; s += RO_BLOCK) lds[s] = 0;
    __syncthreads();
  }
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
    flush_sizes(lds, (uint32_t)a.pi.num_cols, a.sizes, [](uint32_t s) {
      const uint32_t j = s >> 6, l = s & 63;
      return 256 * (j >> 2) + 4 * l + (j & 3);
    });
}

// ------------------------------------------------------------------------------------------ generic form
// any 1 <= K <= 8192: lane l owns columns l, l + 64, ...; scalar loads, the row is read again each round (it is at most
// 32 KB and was just read, so the rounds after the first come out of the cache).  Size counter of column k: lds[k].
__global__ __launch_bounds__(RO_BLOCK) void readout_generic(Args a) {
  extern __shared__ uint32_t lds[];
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols;
  const uint32_t num_rows = (uint32_t)a.pi.num_rows;
  const bool do_sizes = a.sizes != nullptr;
  if (do_sizes) {
    for (uint32_t s = threadIdx.x; s < K; s += RO_BLOCK) lds[s] = 0;
    __syncthreads();
  }
  const uint64_t stride = (uint64_t)gridDim.x * RO_WAVES;
  for (uint64_t r = (uint64_t)blockIdx.x * RO_WAVES + (threadIdx.x >> 6); r < a.n_rows; r += stride) {
    const uint32_t row = a.nodes ? a.nodes[r] : (uint32_t)(a.row_lo + r);
    const bool ok = row < num_rows;
    const float* p = ro_row(a.pi, ok ? row : 0u);
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
  if (do_sizes) flush_sizes(lds, K, a.sizes, [](uint32_t s) { return s; });
}

int fail(int code, const char* what) {
  snprintf(g_last_error, sizeof(g_last_error), "%s", what);
  return code;
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
  const uint64_t K = pi->num_cols;
  if (K == 0 || K > AMMSB_READOUT_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (pi->num_rows >> 32 || n_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (nodes ? row_lo != 0 : (row_lo > pi->num_rows || n_rows > pi->num_rows - row_lo))
    return fail(AMMSB_EINVAL, nodes ? "a node list with row_lo != 0" : "row range past num_rows");
  if (pi->num_blocks == 0 || pi->num_blocks > AMMSB_RPM_MAX_BLOCKS || pi->rows_in_block == 0 ||
      pi->rows_in_block >> 32 || pi->rows_in_block * pi->num_blocks < pi->num_rows ||
      (pi->num_rows && (pi->num_rows - 1) / pi->rows_in_block >= pi->num_blocks))
    return fail(AMMSB_EINVAL, "the blocks do not cover num_rows");
  bool aligned = true;
  for (uint32_t b = 0; b < pi->num_blocks; ++b) {
    if (!pi->blocks[b]) return fail(AMMSB_EINVAL, "a block pointer is NULL");
    aligned = aligned && (reinterpret_cast<uintptr_t>(pi->blocks[b]) & 15) == 0;
  }
  if (n_rows == 0) return AMMSB_OK;

  Args a;
  a.pi = *pi;
  a.nodes = nodes;
  a.row_lo = row_lo;
  a.n_rows = n_rows;
  a.thr = thr;
  a.out = {ids, weights, count, tops ? T : 0u};
  a.sizes = reinterpret_cast<unsigned long long*>(sizes);
  const uint64_t want = (n_rows + RO_WAVES - 1) / RO_WAVES;
  const dim3 grid((unsigned)(want < (uint64_t)RO_MAX_GRID ? want : (uint64_t)RO_MAX_GRID)), block(RO_BLOCK);
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
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    snprintf(g_last_error, sizeof(g_last_error), "%s: %s", name, hipGetErrorString(e));
    return AMMSB_EHIP;
  }
  g_last_kernel = name;
  return AMMSB_OK;
}
