// libammsb_omega.so (include/ammsb_omega.h): the Omega index's counts -- for every pair of positions of a universe the
// number of communities the two nodes share in the detected cover (sD) and in the ground truth (sT), as three histograms.
//
//   omega_bits_*         streams the rows of pi that the universe names, a wave per row: a compare and a __ballot give 64
//                        membership bits per register slot; the row's population count falls out of the ballots.
//   omega_truth_scatter  a wave per ground-truth community walks its members: position[] says where a member sits in the
//                        universe, one vector atomic OR sets its bit.
//   omega_truth_count    a wave per finished row: its population count.
//   omega_pairs          in shape a GEMM over bit rows.  A block of 256 lanes owns a tile of 128 x 128 positions; lane
//                        (ty, tx) of the 16 x 16 block keeps the 8 x 8 micro-tile of rows {4 ty + i, 64 + 4 ty + i} x
//                        {4 tx + j, 64 + 4 tx + j} in registers.  Chunks of 16 words of both row sets go through LDS,
//                        word-major ([word][row], pitch 132), so that a lane's four rows are one 16-byte read, the 16
//                        lanes of a read group cover one 256-byte bank row, and the stores are at most 2-way.  Per word:
//                        four 16-byte reads and 64 x (AND, population count + add).  The detected rows are accumulated
//                        first and packed two counters to a register (sD <= 8192), then the truth rows, then the
//                        compare: (0, 0) into a register, every other pair into 3 L counters in LDS.  The next chunk is
//                        loaded into registers while this one is worked on.
//
// The detected bits' layout (a function of K alone).  A row is W = ceil(K / 32) u32 words, filled as 64-bit ballots, low
// half first.  With F = 4 (K / 256), the ballots of the whole chunks of 256 columns:
//   ballot t < F,  bit j  <->  column 256 (t >> 2) + 4 j + (t & 3)     what lane j holds in component t & 3 of its 16-byte
//                                                                      load number t >> 2
//   ballot t >= F, bit j  <->  column 64 t + j                         the ragged tail, in column order
// Both forms write exactly these words.  The truth bits are in community order: word g >> 5, bit g & 31.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_omega.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int O_WAVES = 4;  // waves per block
constexpr int O_BLOCK = 64 * O_WAVES;

// ------------------------------------------------------------------------------------------ the detected bits
struct BitsArgs {
  ammsb_rpm pi;
  float thr;
  const uint32_t* nodes;  // [n] or NULL
  u64 n;
  uint32_t* bits;    // [n, W]
  uint32_t* counts;  // [n]
};

// lane l holds ballots l and l + 64: words 2 l, 2 l + 1 and 128 + 2 l, 128 + 2 l + 1 of the row
__device__ __forceinline__ void store_row(const BitsArgs& a, u64 p, uint32_t W, u64 w0, u64 w1, uint32_t cnt, int lane) {
  uint32_t* out = a.bits + p * W;
  const uint32_t s = 2u * (uint32_t)lane;
  if (s < W) out[s] = (uint32_t)w0;
  if (s + 1u < W) out[s + 1u] = (uint32_t)(w0 >> 32);
  if (s + 128u < W) out[s + 128u] = (uint32_t)w1;
  if (s + 129u < W) out[s + 129u] = (uint32_t)(w1 >> 32);
  if (lane == 0) a.counts[p] = cnt;
}

__device__ __forceinline__ bool row_of(const BitsArgs& a, u64 p, uint32_t* row) {
  const uint32_t r = a.nodes ? a.nodes[p] : (uint32_t)p;
  *row = r;
  return r < a.pi.num_rows;
}

__global__ __launch_bounds__(O_BLOCK) void omega_bits_fast(BitsArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = K >> 5;
  const int nv = (int)(K >> 8);  // 16-byte loads per lane and row
  const u64 stride = (u64)gridDim.x * O_WAVES;
  for (u64 p = (u64)blockIdx.x * O_WAVES + (threadIdx.x >> 6); p < a.n; p += stride) {
    uint32_t row;
    const bool ok = row_of(a, p, &row);  // (wave-uniform)
    u64 w0 = 0, w1 = 0;
    uint32_t cnt = 0;
    if (ok) {
      const float4* src = reinterpret_cast<const float4*>(postfit_row(a.pi, row)) + lane;
      for (int i = 0; i < nv; ++i) {
        const float4 x = src[i * 64];
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const u64 b = __ballot(comp(x, c) >= a.thr);
          cnt += (uint32_t)__popcll(b);
          place(w0, w1, 4u * i + c, b, lane);
        }
      }
    }
    store_row(a, p, W, w0, w1, cnt, lane);
  }
}

__global__ __launch_bounds__(O_BLOCK) void omega_bits_generic(BitsArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = (K + 31u) >> 5, B = (K + 63u) >> 6, F = 4u * (K >> 8);
  const u64 stride = (u64)gridDim.x * O_WAVES;
  for (u64 p = (u64)blockIdx.x * O_WAVES + (threadIdx.x >> 6); p < a.n; p += stride) {
    uint32_t row;
    const bool ok = row_of(a, p, &row);  // (wave-uniform)
    u64 w0 = 0, w1 = 0;
    uint32_t cnt = 0;
    if (ok) {
      const float* src = postfit_row(a.pi, row);
      for (uint32_t t = 0; t < B; ++t) {
        const uint32_t col = slot_col(t < F, t, (uint32_t)lane);
        const float v = col < K ? src[col] : -1.0f;  // (below every threshold the entry point lets through)
        const u64 b = __ballot(v >= a.thr);
        cnt += (uint32_t)__popcll(b);
        place(w0, w1, t, b, lane);
      }
    }
    store_row(a, p, W, w0, w1, cnt, lane);
  }
}

// ------------------------------------------------------------------------------------------ the truth bits
struct TruthArgs {
  const u64* offsets;  // [G + 1]
  uint32_t G;
  const uint32_t* members;  // [M]
  u64 M, N;
  const int32_t* position;  // [N]
  u64 n;
  uint32_t W;        // ceil(G / 32)
  uint32_t* bits;    // [n, W]
  uint32_t* counts;  // [n]
  u64 *skipped, *outside;
};

__global__ __launch_bounds__(O_BLOCK) void omega_truth_scatter(TruthArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const u64 stride = (u64)gridDim.x * O_WAVES;
  u64 skipped = 0, outside = 0;
  for (u64 g = (u64)blockIdx.x * O_WAVES + (threadIdx.x >> 6); g < a.G; g += stride) {
    const u64 b0 = a.offsets[g], e0 = a.offsets[g + 1];
    const u64 begin = b0 < a.M ? b0 : a.M, end = e0 < a.M ? e0 : a.M;  // whatever offsets holds, the walk stays in members
    for (u64 i = begin + lane; i < end; i += 64) {
      const uint32_t m = a.members[i];
      if (m >= a.N) {
        ++skipped;
        continue;
      }
      const int32_t p = a.position[m];
      if (p < 0 || (u64)p >= a.n) {
        ++outside;
        continue;
      }
      atomicOr(&a.bits[(u64)p * a.W + (uint32_t)(g >> 5)], 1u << (uint32_t)(g & 31u));
    }
  }
  // (all 64 lanes are here)
  skipped = wave_sum_u64(skipped);
  outside = wave_sum_u64(outside);
  if (lane == 0) {
    if (skipped) atomicAdd(a.skipped, skipped);
    if (outside) atomicAdd(a.outside, outside);
  }
}

__global__ __launch_bounds__(O_BLOCK) void omega_truth_count(TruthArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const u64 stride = (u64)gridDim.x * O_WAVES;
  for (u64 p = (u64)blockIdx.x * O_WAVES + (threadIdx.x >> 6); p < a.n; p += stride) {
    const uint32_t* row = a.bits + p * a.W;
    u64 cnt = 0;
    for (uint32_t w = lane; w < a.W; w += 64) cnt += (u64)__popc(row[w]);
    cnt = wave_sum_u64(cnt);
    if (lane == 0) a.counts[p] = (uint32_t)cnt;
  }
}

// ------------------------------------------------------------------------------------------ the pair pass
constexpr uint32_t TILE = AMMSB_OMEGA_TILE;  // positions a side
constexpr uint32_t HALF = TILE / 2;
constexpr int MT = 8;                // a lane's micro-tile is MT x MT
constexpr uint32_t CHUNK = 16;       // words of a row that go through LDS at a time
constexpr uint32_t PITCH = TILE + 4;  // of a word's row of positions in LDS: 16-byte aligned, 4 banks on per word
constexpr int STAGE = (int)(TILE * CHUNK) / O_BLOCK;  // words of each row set a lane loads per chunk
constexpr unsigned PAIR_GRID = 512;  // 256 CUs x 2: what 226 registers a lane admit; past residency a block would only queue
static_assert(TILE == 128 && O_BLOCK == 256 && STAGE == 8, "the micro-tile addressing below assumes a 16 x 16 block");

struct PairArgs {
  const uint32_t* dbits;  // [n, WD]
  const uint32_t* tbits;  // [n, WT]
  uint32_t WD, WT, n, L;
  u64 R;  // tile rows
  u64 tile_begin, tile_count;
  u64* hist;  // [3 L + 1]
};

// the words (pos0 + r, w0 + w) of a chunk that this lane stages: r = idx / CHUNK, w = idx % CHUNK, idx = tid + 256 i
__device__ __forceinline__ void stage_load(const uint32_t* bits, uint32_t W, uint32_t n, uint32_t pos0, uint32_t w0,
                                           uint32_t (&v)[STAGE]) {
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const uint32_t idx = threadIdx.x + (uint32_t)O_BLOCK * i, r = idx / CHUNK, w = w0 + idx % CHUNK;
    const u64 pos = (u64)pos0 + r;
    v[i] = (pos < n && w < W) ? bits[pos * W + w] : 0u;
  }
}

__device__ __forceinline__ void stage_store(uint32_t* lds, const uint32_t (&v)[STAGE]) {
#pragma unroll
  for (int i = 0; i < STAGE; ++i) {
    const uint32_t idx = threadIdx.x + (uint32_t)O_BLOCK * i;
    lds[(idx % CHUNK) * PITCH + idx / CHUNK] = v[i];
  }
}

// acc[i][j] += |row_a(i) & row_b(j)| over all W words of the two row sets of a tile
__device__ __forceinline__ void accumulate(const uint32_t* bits, uint32_t W, uint32_t n, uint32_t pa0, uint32_t pb0,
                                           uint32_t* sA, uint32_t* sB, uint32_t ty, uint32_t tx,
                                           uint32_t (&acc)[MT][MT]) {
  uint32_t va[STAGE], vb[STAGE];
  stage_load(bits, W, n, pa0, 0, va);
  stage_load(bits, W, n, pb0, 0, vb);
#pragma unroll 1
  for (uint32_t w0 = 0; w0 < W; w0 += CHUNK) {
    __syncthreads();  // the previous chunk (or phase, or tile) has been read
    stage_store(sA, va);
    stage_store(sB, vb);
    __syncthreads();
    if (w0 + CHUNK < W) {
      stage_load(bits, W, n, pa0, w0 + CHUNK, va);
      stage_load(bits, W, n, pb0, w0 + CHUNK, vb);
    }
    const uint32_t nw = W - w0 < CHUNK ? W - w0 : CHUNK;
    // (left alone the loop vectoriser interleaves two words with a second set of 64 counters: 298 registers)
#pragma clang loop vectorize(disable) interleave(disable) unroll(disable)
    for (uint32_t w = 0; w < nw; ++w) {
      const uint4 a0 = *reinterpret_cast<const uint4*>(sA + w * PITCH + 4u * ty);
      const uint4 a1 = *reinterpret_cast<const uint4*>(sA + w * PITCH + HALF + 4u * ty);
      const uint4 b0 = *reinterpret_cast<const uint4*>(sB + w * PITCH + 4u * tx);
      const uint4 b1 = *reinterpret_cast<const uint4*>(sB + w * PITCH + HALF + 4u * tx);
      const uint32_t a[MT] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
      const uint32_t b[MT] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < MT; ++j) acc[i][j] += (uint32_t)__popc(a[i] & b[j]);
    }
  }
}

// tile number t of the upper triangle of R x R tiles, row by row -> (row, column)
__device__ __forceinline__ void tile_of(u64 t, u64 R, uint32_t* bi, uint32_t* bj) {
  // row r starts at r R - r (r - 1) / 2: the root of that, then a correction for the rounding of the double
  const double s = 2.0 * (double)R + 1.0;
  double root = (s - sqrt(s * s - 8.0 * (double)t)) * 0.5;
  if (!(root >= 0.0)) root = 0.0;
  u64 r = (u64)root;
  if (r >= R) r = R - 1;
  auto start = [R](u64 x) { return x * R - x * (x - 1) / 2; };  // (x == 0: 0 * (-1) / 2 == 0 in wrapping arithmetic)
  while (r > 0 && start(r) > t) --r;
  while (r + 1 < R && start(r + 1) <= t) ++r;
  *bi = (uint32_t)r;
  *bj = (uint32_t)(r + (t - start(r)));
}

__global__ __launch_bounds__(O_BLOCK) void omega_pairs(PairArgs a) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];  // the two row sets' chunk, then the counters
  uint32_t *sA = lds, *sB = lds + CHUNK * PITCH;
  uint32_t* counters = lds + 2u * CHUNK * PITCH;  // agree[L], detected[L], truth[L]
  const uint32_t L = a.L, n = a.n;
  const uint32_t ty = threadIdx.x >> 4, tx = threadIdx.x & 15u, lane = threadIdx.x & 63u;
  zero_counters<O_BLOCK>(counters, 3u * L);
  u64 zeros = 0, clipped = 0;  // pairs at (0, 0) and pairs at or past level L, of this lane

  for (u64 t = blockIdx.x; t < a.tile_count; t += gridDim.x) {
    uint32_t bi, bj;
    tile_of(a.tile_begin + t, a.R, &bi, &bj);
    const uint32_t pa0 = bi * TILE, pb0 = bj * TILE;

    uint32_t acc[MT][MT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < MT; ++j) acc[i][j] = 0;
    accumulate(a.dbits, a.WD, n, pa0, pb0, sA, sB, ty, tx, acc);
    uint32_t sd[MT][MT / 2];  // sD <= 8192: two to a register
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
      for (int j = 0; j < MT / 2; ++j) {
        sd[i][j] = acc[i][2 * j] | (acc[i][2 * j + 1] << 16);
        acc[i][2 * j] = 0;
        acc[i][2 * j + 1] = 0;
      }
    if (a.WT) accumulate(a.tbits, a.WT, n, pa0, pb0, sA, sB, ty, tx, acc);

    uint32_t z = 0, c = 0;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
      const u64 pa = (u64)pa0 + (i < 4 ? 4u * ty + i : HALF + 4u * ty + (i - 4));
#pragma unroll
      for (int j = 0; j < MT; ++j) {
        const u64 pb = (u64)pb0 + (j < 4 ? 4u * tx + j : HALF + 4u * tx + (j - 4));
        if (pa < pb && pb < n) {  // (pa < pb < n; off the diagonal every pa is below every pb)
          const uint32_t sD = (sd[i][j >> 1] >> (16 * (j & 1))) & 0xFFFFu, sT = acc[i][j];
          if ((sD | sT) == 0) {
            ++z;
          } else if (sD >= L || sT >= L) {
            ++c;
          } else {
            atomicAdd(&counters[L + sD], 1u);
            atomicAdd(&counters[2u * L + sT], 1u);
            if (sD == sT) atomicAdd(&counters[sD], 1u);
          }
        }
      }
    }
    zeros += z;
    clipped += c;
  }

  flush_counters<O_BLOCK>(counters, 3u * L, a.hist);
  // (all 256 lanes are here) the two register counts: a wave sum, then one 64-bit atomic per wave and histogram
  zeros = wave_sum_u64(zeros);
  clipped = wave_sum_u64(clipped);
  if (lane == 0) {
    if (zeros) {
      atomicAdd(&a.hist[0], zeros);
      atomicAdd(&a.hist[L], zeros);
      atomicAdd(&a.hist[2u * L], zeros);
    }
    if (clipped) atomicAdd(&a.hist[3u * L], clipped);
  }
}

size_t lds_bytes(uint32_t L) { return (size_t)(2u * CHUNK * PITCH + 3u * L) * sizeof(uint32_t); }

const char* check_n(uint64_t n) { return (n >> 31) ? "n is 2^31 or more" : nullptr; }

}  // namespace

extern "C" const char* ammsb_omega_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_omega_last_error(void) { return g_last_error; }

extern "C" int ammsb_omega_detected_bits(const ammsb_rpm* pi, float thr, const uint32_t* nodes, uint64_t n, uint32_t* bits,
                                         uint32_t* counts, void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!bits) return fail(AMMSB_EINVAL, "bits is NULL");
  if (!counts) return fail(AMMSB_EINVAL, "counts is NULL");
  if (!(thr >= 0.0f && thr < INFINITY)) return fail(AMMSB_EINVAL, "thr negative, NaN or infinite");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_OMEGA_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (const char* bad = check_n(n)) return fail(AMMSB_EINVAL, bad);
  if (!nodes && n > pi->num_rows) return fail(AMMSB_EINVAL, "no nodes and n past num_rows");
  if (n == 0) return AMMSB_OK;

  BitsArgs a;
  a.pi = *pi;
  a.thr = thr;
  a.nodes = nodes;
  a.n = n;
  a.bits = bits;
  a.counts = counts;
  const dim3 grid(persistent_grid(n, O_WAVES)), block(O_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (pi->num_cols % 256 == 0 && aligned) {
    hipLaunchKernelGGL(omega_bits_fast, grid, block, 0, s, a);
    return launched("omega_bits_fast");
  }
  hipLaunchKernelGGL(omega_bits_generic, grid, block, 0, s, a);
  return launched("omega_bits_generic");
}

extern "C" int ammsb_omega_truth_bits(const uint64_t* offsets, uint64_t num_truth, const uint32_t* members,
                                      uint64_t num_members, uint64_t num_nodes, const int32_t* position, uint64_t n,
                                      uint32_t* bits, uint32_t* counts, uint64_t* skipped, uint64_t* outside,
                                      void* stream) {
  if (num_truth > AMMSB_OMEGA_MAX_TRUTH)
    return fail(AMMSB_EINVAL, "more than 65536 ground-truth communities: a bit row per node would not be a sparse cover's size");
  if (num_nodes >> 32) return fail(AMMSB_EINVAL, "2^32 nodes or more");
  if (num_members >> 32) return fail(AMMSB_EINVAL, "2^32 members or more");
  if (const char* bad = check_n(n)) return fail(AMMSB_EINVAL, bad);
  if (n > 0 && num_truth > 0 && (!offsets || !position || !bits || !counts || !skipped || !outside))
    return fail(AMMSB_EINVAL, "offsets, position, bits, counts, skipped or outside is NULL");
  if (num_members > 0 && !members) return fail(AMMSB_EINVAL, "members is NULL");
  if (n == 0 || num_truth == 0) return AMMSB_OK;

  TruthArgs a;
  a.offsets = reinterpret_cast<const u64*>(offsets);
  a.G = (uint32_t)num_truth;
  a.members = members;
  a.M = num_members;
  a.N = num_nodes;
  a.position = position;
  a.n = n;
  a.W = ((uint32_t)num_truth + 31u) >> 5;
  a.bits = bits;
  a.counts = counts;
  a.skipped = reinterpret_cast<u64*>(skipped);
  a.outside = reinterpret_cast<u64*>(outside);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (num_members > 0) {
    hipLaunchKernelGGL(omega_truth_scatter, dim3(persistent_grid(num_truth, O_WAVES)), dim3(O_BLOCK), 0, s, a);
    if (const int rc = launched("omega_truth_scatter")) return rc;
  }
  hipLaunchKernelGGL(omega_truth_count, dim3(persistent_grid(n, O_WAVES)), dim3(O_BLOCK), 0, s, a);
  return launched("omega_truth_count");
}

extern "C" int ammsb_omega_pairs(const uint32_t* detected_bits, uint32_t num_cols, const uint32_t* truth_bits,
                                 uint64_t num_truth, uint64_t n, uint32_t num_levels, uint64_t tile_begin,
                                 uint64_t tile_count, uint64_t* hist, void* stream) {
  if (!hist) return fail(AMMSB_EINVAL, "hist is NULL");
  if (num_cols == 0 || num_cols > AMMSB_OMEGA_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (num_truth > AMMSB_OMEGA_MAX_TRUTH) return fail(AMMSB_EINVAL, "more than 65536 ground-truth communities");
  if (num_levels == 0 || num_levels > AMMSB_OMEGA_MAX_LEVELS)
    return fail(AMMSB_EINVAL, "num_levels outside 1..4096: 3 L block-private 32-bit counters have to fit the LDS beside the tile");
  if (const char* bad = check_n(n)) return fail(AMMSB_EINVAL, bad);
  const uint64_t R = (n + TILE - 1) / TILE, tiles = R * (R + 1) / 2;  // (R < 2^24)
  if (tile_begin > tiles || tile_count > tiles - tile_begin) return fail(AMMSB_EINVAL, "the tile range ends past the triangle");
  if (tile_count > AMMSB_OMEGA_MAX_LAUNCH_TILES)
    return fail(AMMSB_EINVAL, "more than 2^26 tiles in one launch: the block-private counters are 32-bit");
  if (n == 0 || tile_count == 0) return AMMSB_OK;
  if (!detected_bits) return fail(AMMSB_EINVAL, "detected_bits is NULL");
  if (num_truth > 0 && !truth_bits) return fail(AMMSB_EINVAL, "truth_bits is NULL");

  PairArgs a;
  a.dbits = detected_bits;
  a.tbits = truth_bits;
  a.WD = (num_cols + 31u) >> 5;
  a.WT = ((uint32_t)num_truth + 31u) >> 5;
  a.n = (uint32_t)n;
  a.L = num_levels;
  a.R = R;
  a.tile_begin = tile_begin;
  a.tile_count = tile_count;
  a.hist = reinterpret_cast<u64*>(hist);
  // the chunk's 2 x 8.25 KiB and 3 L counters are just over the default 64 KiB of dynamic LDS at L = 4096: once per process
  static const hipError_t big =
      hipFuncSetAttribute(reinterpret_cast<const void*>(&omega_pairs), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)lds_bytes(AMMSB_OMEGA_MAX_LEVELS));
  if (big != hipSuccess) return hip_fail("omega_pairs", big);
  // a block of a grid of g blocks meets at most ceil(2^26 / g) tiles of 2^14 pairs: 2^31 for g = PAIR_GRID, and a
  // smaller grid has a tile per block
  const dim3 grid((unsigned)(tile_count < PAIR_GRID ? tile_count : PAIR_GRID)), block(O_BLOCK);
  hipLaunchKernelGGL(omega_pairs, grid, block, lds_bytes(num_levels), static_cast<hipStream_t>(stream), a);
  return launched("omega_pairs");
}
