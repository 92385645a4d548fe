// libammsb_relate.so (include/ammsb_relate.h): the K x K matrix of the nodes every two detected communities share, and
// per community the partners it overlaps most.
//
//   relate_bits_*   streams a slab of pi into community-major bits.  A wave owns 64 consecutive rows x 64 V columns
//                   (V = 4: one 16-byte load per lane and row; V = 1: one element).  Per row and component a compare and
//                   a __ballot give the 64 columns' bits of that row -- node-major -- which lane (row & 63) keeps.  Then
//                   the V blocks of 64 x 64 bits are transposed: ballot j of bit j of every lane's kept word is the word
//                   of column j over the 64 rows, which lane j keeps and stores whole.  Two ballots per 64 loaded floats;
//                   the read of pi bounds the kernel.  The four waves of a block take four consecutive row groups of the
//                   same columns, so that their 8-byte stores fill 32 consecutive bytes of every community.
//   relate_pairs    ammsb_omega.hip's omega_pairs with the roles swapped: the bit rows belong to communities and run over
//                   the nodes, read as 32-bit words.  A block of 256 lanes owns a tile of 128 x 128 community pairs;
//                   lane (ty, tx) of the 16 x 16 block keeps the 8 x 8 micro-tile of communities {4 ty + i, 64 + 4 ty + i}
//                   x {4 tx + j, 64 + 4 tx + j} in registers.  Chunks of 16 words of both community sets go through LDS
//                   word-major ([word][community], pitch 132): a lane's four communities are one 16-byte read, the 16
//                   lanes of a read group cover one 256-byte bank row, the stores are at most 2-way.  The next chunk is
//                   loaded into registers while this one is worked on.  The work items are (tile, depth slice): the node
//                   words are cut so that about PAIR_ITEMS items exist whatever K is; an item's partial tile is added to
//                   overlap with 32-bit vector atomics, zeros skipped.
//   relate_top      a wave per community, `top` rounds of "the best candidate that comes after the previous winner" over
//                   its row of overlap: nothing is marked as taken, the matrix stays read-only.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_relate.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int R_WAVES = 4;  // waves per block
constexpr int R_BLOCK = 64 * R_WAVES;

// ------------------------------------------------------------------------------------------ the bits pass
struct BitsArgs {
  ammsb_rpm pi;
  float thr;
  uint32_t row0, rows;  // the slab
  uint32_t W;           // ceil(rows / 64): words per community
  uint32_t chunks;      // column chunks of 64 V
  u64 items;            // ceil(W / R_WAVES) * chunks
  u64* bits;            // [K, W]
};

// kept[c] of lane r: bit j <-> (row r, column c0 + V j + c).  Word (column, g) is the ballot of that bit over the lanes.
// All 64 lanes are here (the control flow around is wave-uniform).
template <int V>
__device__ __forceinline__ void transpose_store(const BitsArgs& a, const u64 (&kept)[V], uint32_t c0, uint32_t g, int lane) {
  const uint32_t K = (uint32_t)a.pi.num_cols;
#pragma unroll
  for (int c = 0; c < V; ++c) {
    u64 mine = 0;
#pragma unroll 8
    for (int j = 0; j < 64; ++j) {
      const u64 word = __ballot((kept[c] >> j) & 1ull);
      if (lane == j) mine = word;
    }
    const uint32_t col = c0 + (uint32_t)V * (uint32_t)lane + (uint32_t)c;
    if (col < K) a.bits[(u64)col * a.W + g] = mine;
  }
}

// item -> (the wave's row group, the first column); false: the group is past the slab (wave-uniform)
__device__ __forceinline__ bool bits_item(const BitsArgs& a, u64 item, int V, uint32_t* g, uint32_t* c0, uint32_t* n) {
  *g = (uint32_t)(item / a.chunks) * R_WAVES + (threadIdx.x >> 6);
  *c0 = (uint32_t)(item % a.chunks) * 64u * (uint32_t)V;
  if (*g >= a.W) return false;
  const uint32_t left = a.rows - 64u * *g;  // (> 0: g < W)
  *n = left < 64u ? left : 64u;
  return true;
}

__global__ __launch_bounds__(R_BLOCK) void relate_bits_fast(BitsArgs a) {
  const int lane = threadIdx.x & 63;
  for (u64 item = blockIdx.x; item < a.items; item += gridDim.x) {
    uint32_t g, c0, n;
    if (!bits_item(a, item, 4, &g, &c0, &n)) continue;
    const uint32_t first = a.row0 + 64u * g;
    u64 kept[4] = {0, 0, 0, 0};
    // (64 trips whatever n is, so that the loop unrolls and its loads overlap: a trip past the slab reads the slab's
    // last row again and keeps nothing)
#pragma unroll 8
    for (uint32_t r = 0; r < 64; ++r) {
      const float4 x = reinterpret_cast<const float4*>(postfit_row(a.pi, first + (r < n ? r : n - 1)) + c0)[lane];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const u64 b = __ballot(comp(x, c) >= a.thr);
        if (lane == (int)r && r < n) kept[c] = b;
      }
    }
    transpose_store<4>(a, kept, c0, g, lane);
  }
}

__global__ __launch_bounds__(R_BLOCK) void relate_bits_generic(BitsArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols;
  for (u64 item = blockIdx.x; item < a.items; item += gridDim.x) {
    uint32_t g, c0, n;
    if (!bits_item(a, item, 1, &g, &c0, &n)) continue;
    const uint32_t first = a.row0 + 64u * g, col = c0 + (uint32_t)lane;
    u64 kept[1] = {0};
#pragma unroll 8
    for (uint32_t r = 0; r < 64; ++r) {  // (64 trips: as in the fast form)
      const float v = col < K ? postfit_row(a.pi, first + (r < n ? r : n - 1))[col] : -1.0f;  // (below every threshold)
      const u64 b = __ballot(v >= a.thr);
      if (lane == (int)r && r < n) kept[0] = b;
    }
    transpose_store<1>(a, kept, c0, g, lane);
  }
}

// ------------------------------------------------------------------------------------------ the pair pass
constexpr uint32_t TILE = AMMSB_RELATE_TILE;  // communities a side
constexpr uint32_t HALF = TILE / 2;
constexpr int MT = 8;                 // a lane's micro-tile is MT x MT
constexpr uint32_t CHUNK = 16;        // 32-bit words of a community that go through LDS at a time: 512 nodes
constexpr uint32_t PITCH = TILE + 4;  // of a word's row of communities in LDS: 16-byte aligned, 4 banks on per word
constexpr int STAGE = (int)(TILE * CHUNK) / R_BLOCK;  // words of each community set a lane loads per chunk
constexpr unsigned PAIR_GRID = 512;   // 256 CUs x 2 blocks: what the registers of a lane admit; more would only queue
constexpr u64 PAIR_ITEMS = 1024;      // (tile, slice) items aimed at: two rounds of the grid, to even out the tail
static_assert(TILE == 128 && R_BLOCK == 256 && STAGE == 8, "the micro-tile addressing below assumes a 16 x 16 block");

struct PairArgs {
  const uint32_t* bits;  // [K, W] 32-bit words
  uint32_t K, W;
  uint32_t slice_words;  // a multiple of CHUNK
  uint32_t slices;       // ceil(W / slice_words)
  u64 R;                 // tile rows
  u64 items;             // R (R + 1) / 2 * slices
  uint32_t* overlap;     // [K, K]
};

// the words (c0 + r, w0 + w) of a chunk that this lane stages: r = idx / CHUNK, w = idx % CHUNK, idx = tid + 256 i
__device__ __forceinline__ void stage_load(const PairArgs& a, uint32_t c0, uint32_t w0, uint32_t wend, uint32_t (&v)[STAGE]) {
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const uint32_t idx = threadIdx.x + (uint32_t)R_BLOCK * i, c = c0 + idx / CHUNK, w = w0 + idx % CHUNK;
    v[i] = (c < a.K && w < wend) ? a.bits[(u64)c * a.W + w] : 0u;
  }
}

__device__ __forceinline__ void stage_store(uint32_t* lds, const uint32_t (&v)[STAGE]) {
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const uint32_t idx = threadIdx.x + (uint32_t)R_BLOCK * i;
    lds[(idx % CHUNK) * PITCH + idx / CHUNK] = v[i];
  }
}

// tile number t of the upper triangle of R x R tiles, row by row -> (row, column)
__device__ __forceinline__ void tile_of(u64 t, u64 R, uint32_t* bi, uint32_t* bj) {
  u64 r = 0, start = 0;  // (R <= 64: a walk over the rows)
  while (r + 1 < R && start + (R - r) <= t) {
    start += R - r;
    ++r;
  }
  *bi = (uint32_t)r;
  *bj = (uint32_t)(r + (t - start));
}

__global__ __launch_bounds__(R_BLOCK) void relate_pairs(PairArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t sA[CHUNK * PITCH];
  __shared__ __attribute__((aligned(16))) uint32_t sB[CHUNK * PITCH];
  const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15u, K = a.K;

  for (u64 item = blockIdx.x; item < a.items; item += gridDim.x) {
    uint32_t bi, bj;
    tile_of(item / a.slices, a.R, &bi, &bj);
    const uint32_t ca0 = bi * TILE, cb0 = bj * TILE;
    const uint32_t wbeg = (uint32_t)(item % a.slices) * a.slice_words;
    const uint32_t wend = a.W - wbeg < a.slice_words ? a.W : wbeg + a.slice_words;

    uint32_t acc[MT][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = 0;

    uint32_t va[STAGE], vb[STAGE];
    stage_load(a, ca0, wbeg, wend, va);
    stage_load(a, cb0, wbeg, wend, vb);
#pragma unroll 1
    for (uint32_t w0 = wbeg; w0 < wend; w0 += CHUNK) {
      __syncthreads();  // the previous chunk (or item) has been read
      stage_store(sA, va);
      stage_store(sB, vb);
      __syncthreads();
      if (w0 + CHUNK < wend) {
        stage_load(a, ca0, w0 + CHUNK, wend, va);
        stage_load(a, cb0, w0 + CHUNK, wend, vb);
      }
      const uint32_t nw = wend - w0 < CHUNK ? wend - w0 : CHUNK;
      // (left alone the loop vectoriser interleaves two words with a second set of 64 counters: see ammsb_omega.hip)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
      for (uint32_t w = 0; w < nw; ++w) {
        const uint4 a0 = *reinterpret_cast<const uint4*>(sA + w * PITCH + 4u * ty);
        const uint4 a1 = *reinterpret_cast<const uint4*>(sA + w * PITCH + HALF + 4u * ty);
        const uint4 b0 = *reinterpret_cast<const uint4*>(sB + w * PITCH + 4u * tx);
        const uint4 b1 = *reinterpret_cast<const uint4*>(sB + w * PITCH + HALF + 4u * tx);
        const uint32_t x[MT] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
        const uint32_t y[MT] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
          for (int j = 0; j < MT; ++j) acc[i][j] += (uint32_t)__popc(x[i] & y[j]);
      }
    }

    // integer adds: the sum does not depend on who arrives first.  A diagonal tile holds (k, l) and (l, k) itself.
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const uint32_t k = ca0 + (i < 4 ? 4u * ty + i : HALF + 4u * ty + (i - 4));
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const uint32_t l = cb0 + (j < 4 ? 4u * tx + j : HALF + 4u * tx + (j - 4));
        const uint32_t v = acc[i][j];
        if (k < K && l < K && v) {
          atomicAdd(&a.overlap[(u64)k * K + l], v);
          if (bi != bj) atomicAdd(&a.overlap[(u64)l * K + k], v);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------ the partners
struct TopArgs {
  const uint32_t* overlap;  // [K, K]
  uint32_t K, measure, top, min_overlap;  // min_overlap >= 1
  int32_t* partner;  // [K, top]
  uint32_t* shared;  // [K, top]
};

// A candidate partner is (o, den, l): o shared nodes out of den (the measure is o / den); o == 0: none.
// Does x come before y in the ranking?  o_x / den_x > o_y / den_y as o_x den_y > o_y den_x in 128 bits, then the lower l.
__device__ __forceinline__ bool before(uint32_t xo, u64 xden, uint32_t xl, uint32_t yo, u64 yden, uint32_t yl) {
  const u64 lh = __umul64hi((u64)xo, yden), ll = (u64)xo * yden;
  const u64 rh = __umul64hi((u64)yo, xden), rl = (u64)yo * xden;
  if (lh != rh) return lh > rh;
  if (ll != rl) return ll > rl;
  return xl < yl;
}

// (bo, bden, bl) = whichever of it and (o, den, l) comes first
__device__ __forceinline__ void offer_cand(uint32_t& bo, u64& bden, uint32_t& bl, uint32_t o, u64 den, uint32_t l) {
  const bool take = o != 0 && (bo == 0 || before(o, den, l, bo, bden, bl));
  bo = take ? o : bo;
  bden = take ? den : bden;
  bl = take ? l : bl;
}

__global__ __launch_bounds__(R_BLOCK) void relate_top(TopArgs a) {
  __shared__ uint32_t diag[AMMSB_RELATE_MAX_COLS];
  const uint32_t K = a.K, lane = threadIdx.x & 63u;
  for (uint32_t l = threadIdx.x; l < K; l += R_BLOCK) diag[l] = a.overlap[(u64)l * K + l];
  __syncthreads();
  const uint32_t k = blockIdx.x * R_WAVES + (threadIdx.x >> 6);
  if (k >= K) return;  // (wave-uniform, after the only barrier)
  const uint32_t* row = a.overlap + (u64)k * K;
  const u64 dk = diag[k];
  uint32_t po = 0, pl = 0;  // the previous round's winner
  u64 pden = 1;
  for (uint32_t t = 0; t < a.top; ++t) {
    uint32_t bo = 0, bl = 0;
    u64 bden = 1;
    for (uint32_t l = lane; l < K; l += 64) {
      const uint32_t o = row[l];
      if (l == k || o < a.min_overlap) continue;
      u64 den = 1;
      if (a.measure == AMMSB_RELATE_JACCARD) den = dk + diag[l] - o;
      else if (a.measure == AMMSB_RELATE_CONTAINED) den = diag[l];
      if (t > 0 && !before(po, pden, pl, o, den, l)) continue;  // taken in an earlier round
      offer_cand(bo, bden, bl, o, den, l);
    }
    // every lane ends with the wave's first: the order is total, so the butterfly's partners agree
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const uint32_t oo = (uint32_t)__shfl_xor((int)bo, s, 64), ol = (uint32_t)__shfl_xor((int)bl, s, 64);
      const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)bden, s, 64);
      const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(bden >> 32), s, 64);
      offer_cand(bo, bden, bl, oo, ((u64)hi << 32) | lo, ol);
    }
    if (bo == 0) {  // nothing left: the empty slots
      for (uint32_t s = t + lane; s < a.top; s += 64) {
        a.partner[(u64)k * a.top + s] = -1;
        a.shared[(u64)k * a.top + s] = 0;
      }
      break;
    }
    if (lane == 0) {
      a.partner[(u64)k * a.top + t] = (int32_t)bl;
      a.shared[(u64)k * a.top + t] = bo;
    }
    po = bo;
    pden = bden;
    pl = bl;
  }
}

const char* check_cols(uint32_t K) { return (K == 0 || K > AMMSB_RELATE_MAX_COLS) ? "num_cols outside 1..8192" : nullptr; }

}  // namespace

extern "C" const char* ammsb_relate_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_relate_last_error(void) { return g_last_error; }

extern "C" uint64_t ammsb_relate_bits_bytes(uint64_t rows, uint32_t num_cols) {
  if (check_cols(num_cols) || (rows >> 32)) return 0;
  return (uint64_t)num_cols * ((rows + 63) / 64) * sizeof(uint64_t);
}

extern "C" int ammsb_relate_bits(const ammsb_rpm* pi, float thr, uint64_t row0, uint64_t rows, uint64_t* bits, void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!bits) return fail(AMMSB_EINVAL, "bits is NULL");
  if (!(thr >= 0.0f && thr < INFINITY)) return fail(AMMSB_EINVAL, "thr negative, NaN or infinite");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_RELATE_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (row0 % 64) return fail(AMMSB_EINVAL, "row0 is not a multiple of 64");
  if (rows > pi->num_rows || row0 > pi->num_rows - rows) return fail(AMMSB_EINVAL, "the row range ends past num_rows");
  if (rows == 0) return AMMSB_OK;

  const bool fast = pi->num_cols % 256 == 0 && aligned;
  BitsArgs a;
  a.pi = *pi;
  a.thr = thr;
  a.row0 = (uint32_t)row0;
  a.rows = (uint32_t)rows;
  a.W = (uint32_t)((rows + 63) / 64);
  a.chunks = fast ? (uint32_t)(pi->num_cols / 256) : (uint32_t)((pi->num_cols + 63) / 64);
  a.items = (uint64_t)((a.W + R_WAVES - 1) / R_WAVES) * a.chunks;
  a.bits = reinterpret_cast<u64*>(bits);
  const dim3 grid(persistent_grid(a.items, 1)), block(R_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (fast) {
    hipLaunchKernelGGL(relate_bits_fast, grid, block, 0, s, a);
    return launched("relate_bits_fast");
  }
  hipLaunchKernelGGL(relate_bits_generic, grid, block, 0, s, a);
  return launched("relate_bits_generic");
}

extern "C" int ammsb_relate_pairs(const uint64_t* bits, uint32_t num_cols, uint64_t rows, uint32_t* overlap, void* stream) {
  if (!bits) return fail(AMMSB_EINVAL, "bits is NULL");
  if (!overlap) return fail(AMMSB_EINVAL, "overlap is NULL");
  if (const char* bad = check_cols(num_cols)) return fail(AMMSB_EINVAL, bad);
  if (rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (rows == 0) return AMMSB_OK;

  PairArgs a;
  a.bits = reinterpret_cast<const uint32_t*>(bits);
  a.K = num_cols;
  a.W = 2u * (uint32_t)((rows + 63) / 64);  // (< 2^27)
  a.R = (num_cols + TILE - 1) / TILE;
  const uint64_t tiles = a.R * (a.R + 1) / 2, chunks = (a.W + CHUNK - 1) / CHUNK;
  // depth slices: as many as bring the items to PAIR_ITEMS, whole chunks each
  uint64_t depth = (PAIR_ITEMS + tiles - 1) / tiles;
  if (depth > chunks) depth = chunks;
  const uint64_t slice_chunks = (chunks + depth - 1) / depth;
  a.slice_words = (uint32_t)(slice_chunks * CHUNK);
  a.slices = (uint32_t)((chunks + slice_chunks - 1) / slice_chunks);
  a.items = tiles * a.slices;
  a.overlap = overlap;
  const dim3 grid((unsigned)(a.items < PAIR_GRID ? a.items : PAIR_GRID)), block(R_BLOCK);
  hipLaunchKernelGGL(relate_pairs, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launched("relate_pairs");
}

extern "C" int ammsb_relate_top(const uint32_t* overlap, uint32_t num_cols, uint32_t measure, uint32_t top,
                                uint32_t min_overlap, int32_t* partner, uint32_t* shared, void* stream) {
  if (!overlap) return fail(AMMSB_EINVAL, "overlap is NULL");
  if (!partner) return fail(AMMSB_EINVAL, "partner is NULL");
  if (!shared) return fail(AMMSB_EINVAL, "shared is NULL");
  if (const char* bad = check_cols(num_cols)) return fail(AMMSB_EINVAL, bad);
  if (measure != AMMSB_RELATE_OVERLAP && measure != AMMSB_RELATE_JACCARD && measure != AMMSB_RELATE_CONTAINED)
    return fail(AMMSB_EINVAL, "measure is none of overlap, jaccard, contained");
  if (top == 0 || top > AMMSB_RELATE_MAX_TOP) return fail(AMMSB_EINVAL, "top outside 1..64");

  TopArgs a;
  a.overlap = overlap;
  a.K = num_cols;
  a.measure = measure;
  a.top = top;
  a.min_overlap = min_overlap ? min_overlap : 1u;
  a.partner = partner;
  a.shared = shared;
  const dim3 grid((num_cols + R_WAVES - 1) / R_WAVES), block(R_BLOCK);
  hipLaunchKernelGGL(relate_top, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launched("relate_top");
}
