// What every one-object library of csrc/Makefile's ONE shares, refsample alone excepted (it reads no fitted model):
// the descriptor check that decides whether a kernel may issue 16-byte loads, the per-thread error and launch state,
// the wave-wide selection the exactness claims of DESIGN 4.8 and 4.10 rest on, the block-private counters, the row
// addressing, the slot -> column rule of the kernels that read a row either way, and the readers and writers of the
// node-major membership bits that libammsb_connect.so's mask pass makes and five libraries read.
//
// Everything here has internal linkage on purpose (an unnamed namespace; device code is __forceinline__): each
// library is one translation unit, keeps thread_local state of its own and exports nothing but what its header
// declares.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/ammsb.h"

namespace {

// TTRowPartitionedMatrix_Row with 64-bit offsets: row indices are vertex ids, so the block index is a 32-bit division;
// the element offset is 64-bit.  The same lines as rpm_row() of ammsb_dev.h, and not a call of it: with its 64-bit row
// parameter the read-out kernels came out with other register counts (readout_fast<1..4> two more SGPRs,
// readout_generic 32 instead of 35 VGPRs) and other instruction sequences, which a refactor has no business changing.
__device__ __forceinline__ const float* postfit_row(const ammsb_rpm& m, uint32_t row) {
  if (m.num_blocks == 1) return reinterpret_cast<const float*>(m.blocks[0]) + (uint64_t)row * m.num_cols;
  const uint32_t rib = (uint32_t)m.rows_in_block;
  const uint32_t blk = row / rib;
  return reinterpret_cast<const float*>(m.blocks[blk]) + (uint64_t)(row - blk * rib) * m.num_cols;
}

// Which column slot j of lane `lane` stands for, in a kernel whose lanes walk a row (or 64 j-aligned part of one) in
// slots.  The 16-byte form loads float4 number j >> 2 of the lane and takes its component j & 3; the generic form reads
// one element per slot, lanes side by side.  Both forms of a library write the same words, so its readers use this too.
__device__ __forceinline__ uint32_t slot_col(bool fast, uint32_t j, uint32_t lane) {
  return fast ? 256u * (j >> 2) + 4u * lane + (j & 3u) : 64u * j + lane;
}

// ballot (or word) t of a bit row goes to lane t & 63, into its first (t < 64) or second register
__device__ __forceinline__ void place(unsigned long long& w0, unsigned long long& w1, uint32_t t, unsigned long long bits,
                                      int lane) {
  if (lane == (int)(t & 63u)) {
    if (t < 64u) w0 = bits;
    else w1 = bits;
  }
}

// ------------------------------------------------------------------------------------------ host: errors, launches
thread_local const char* g_last_kernel = "";
thread_local char g_last_error[256] = "";

int fail(int code, const char* what) {
  snprintf(g_last_error, sizeof(g_last_error), "%s", what);
  return code;
}

int hip_fail(const char* name, hipError_t e) {
  snprintf(g_last_error, sizeof(g_last_error), "%s: %s", name, hipGetErrorString(e));
  return AMMSB_EHIP;
}

// after a launch: the launch error as the library's error, else `name` is the last kernel form
int launched(const char* name) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return hip_fail(name, e);
  g_last_kernel = name;
  return AMMSB_OK;
}

constexpr uint32_t MAX_GRID = 2048;  // 256 CUs x 8 blocks: past residency a block would only queue

// blocks of a persistent grid over n_items, per_block of them in flight per block
unsigned persistent_grid(uint64_t n_items, uint64_t per_block) {
  const uint64_t want = (n_items + per_block - 1) / per_block;
  return (unsigned)(want < MAX_GRID ? want : MAX_GRID);
}

// The descriptor rules every entry point shares: NULL, or what is wrong.  *aligned16: every block may be read with
// 16-byte loads.
const char* check_rpm(const ammsb_rpm* m, uint64_t max_cols, bool* aligned16) {
  if (m->num_cols == 0 || m->num_cols > max_cols) return "num_cols outside 1..8192";
  if (m->num_rows >> 32) return "2^32 rows or more";
  if (m->num_blocks == 0 || m->num_blocks > AMMSB_RPM_MAX_BLOCKS || m->rows_in_block == 0 || m->rows_in_block >> 32 ||
      m->rows_in_block * m->num_blocks < m->num_rows ||
      (m->num_rows && (m->num_rows - 1) / m->rows_in_block >= m->num_blocks))
    return "the blocks do not cover num_rows";
  bool aligned = true;
  for (uint32_t b = 0; b < m->num_blocks; ++b) {
    if (!m->blocks[b]) return "a block pointer is NULL";
    aligned = aligned && (reinterpret_cast<uintptr_t>(m->blocks[b]) & 15) == 0;
  }
  *aligned16 = aligned;
  return nullptr;
}

// p is not a multiple of `to` bytes (a power of two)
bool misaligned(const void* p, uintptr_t to) { return (reinterpret_cast<uintptr_t>(p) & (to - 1)) != 0; }

// ------------------------------------------------------------------------------------------ wave reductions
// Every lane ends with the maximum.  Lanes 0..15 of each row of 16 by DPP (two quad permutes, then the mirrors pair
// quads and halves: a max does not care which partner it meets, only that the groups merge), rows by two shuffles.
// All 64 lanes are active wherever these are called (control flow around them is wave-uniform).
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

// every lane ends with the sum, added in the butterfly's fixed order
__device__ __forceinline__ float wave_sum_f32(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// every lane ends with the sum
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

__device__ __forceinline__ float comp(const float4& q, int c) { return c == 0 ? q.x : c == 1 ? q.y : c == 2 ? q.z : q.w; }

// ------------------------------------------------------------------------------------------ node-major membership bits
// Row a of the mask is W = ceil(K / 64) 64-bit words; bit k & 63 of word k >> 6 says pi[a, k] >= thr.  connect_mask_* of
// ammsb_connect.hip write it; the edge kernels of connect and the kernels of modularity, roles, triangles and components
// read it, through mask_word() alone.
//
// Bits past K are cleared on read.  The mask is a public buffer, so a reader does not trust the last word of a row: a
// set bit that stands for no community would become an index outside whatever the kernel keeps per community (a cell
// of directed, an accumulator, a counter of ksum / ksq / kmembers or ktri3 / kpart, a slot's community).  A kernel that
// turns a bit of mask_word() into a community k may therefore rely on k < K, which the "(< K: live_bits)" remarks at
// those places refer to.

// the bits of word w that stand for a community
__device__ __forceinline__ unsigned long long live_bits(uint32_t w, uint32_t K) {
  const uint32_t left = K - 64u * w;  // (w < W: > 0)
  return left >= 64u ? ~0ull : (1ull << left) - 1ull;
}

// Word w of node's row, 0 past the row.  `a` is the kernel's own argument struct (each has mask, W and K), not three
// scalars, so that every kernel loads those fields where it did when it had this function to itself.
template <class Args>
__device__ __forceinline__ unsigned long long mask_word(const Args& a, uint32_t node, uint32_t w) {
  return w < a.W ? a.mask[(uint64_t)node * a.W + w] & live_bits(w, a.K) : 0ull;
}

// A wave writes row `row` of W <= 128 words: lane l holds words l (w0) and l + 64 (w1), as place() left them.  The mask
// passes of quality and connect end with it (their words differ, the way they reach memory does not).
__device__ __forceinline__ void store_bit_row(unsigned long long* out_base, uint64_t row, uint32_t W, unsigned long long w0,
                                              unsigned long long w1, int lane) {
  unsigned long long* out = out_base + row * W;
  if ((uint32_t)lane < W) out[lane] = w0;
  if ((uint32_t)lane + 64u < W) out[lane + 64] = w1;
}

// ------------------------------------------------------------------------------------------ selection
// A round of "the T largest (value, lowest column first)": every lane's best eligible element, the wave maximum of the
// value bits (non-negative binary32 orders as its bit pattern), the lowest column among the lanes that hold it.
// "Eligible" is "comes after the previous winner", so nothing is marked as taken and the data stays read-only.
struct Best {
  int bits;  // value bits of the lane's best eligible element; -1: none
  uint32_t col;
};

// one element offered to a lane's running best, in ascending column order (strict >: the lower column wins in a lane)
template <bool FIRST>
__device__ __forceinline__ void offer(Best& b, int bits, uint32_t col, int pbits, uint32_t pcol) {
  const bool elig = FIRST || bits < pbits || (bits == pbits && col > pcol);
  if (elig && bits > b.bits) {
    b.bits = bits;
    b.col = col;
  }
}

// The winner of a round is wbits = wave_max_i32(b.bits), which a library tests first (nothing left: < 0; the read-out
// also stops below its threshold, before this ballot and reduction are paid for), and then this column.
__device__ __forceinline__ uint32_t winner_col(const Best& b, int wbits) {
  const uint64_t holders = __ballot(b.bits == wbits);
  if (__popcll(holders) == 1) return (uint32_t)__builtin_amdgcn_readlane((int)b.col, (int)__builtin_ctzll(holders));
  // the same value in several lanes: the lowest column (columns are < 2^31, so ~col orders as an int)
  return ~(uint32_t)wave_max_i32((int)~(b.bits == wbits ? b.col : 0x7FFFFFFFu));
}

// ------------------------------------------------------------------------------------------ block-private counters
// n u32 counters in LDS that the block's lanes ds_add into; when the block has run out of work, one 64-bit vector
// atomic per non-zero counter s into out[COL_OF(s)].  Integer adds only: nothing depends on arrival order.
// Two things here are as they are so that every kernel's code stays what it was before these loops had one home: n keeps
// the caller's type (a bound that is the descriptor's 64-bit num_cols is compared as such), and `out` is a reference,
// so that a caller that names a field of its kernel argument has it read after the barrier, where its own loop read it.
// a bound that includes its end: `s < Through{K}` is s <= K, without a K + 1 that could wrap
struct Through {
  uint64_t last;
};
__device__ __forceinline__ bool operator<(uint32_t s, Through t) { return s <= t.last; }

template <int BLOCK, class N>
__device__ __forceinline__ void zero_counters(uint32_t* lds, N n) {
  for (uint32_t s = threadIdx.x; s < n; s += BLOCK) lds[s] = 0;
  __syncthreads();
}

__device__ __forceinline__ uint32_t same_slot(uint32_t s) { return s; }

template <int BLOCK, uint32_t (*COL_OF)(uint32_t) = same_slot, class N>
__device__ __forceinline__ void flush_counters(const uint32_t* lds, N n, unsigned long long* const& out) {
  __syncthreads();
  for (uint32_t s = threadIdx.x; s < n; s += BLOCK) {
    const uint32_t c = lds[s];
    if (c) atomicAdd(&out[COL_OF(s)], (unsigned long long)c);
  }
}

}  // namespace
