// libammsb_connect.so (include/ammsb_connect.h): the K x K matrix of the links of an edge list that run between every two
// detected communities, and per community the partners it is linked to most.
//
//   connect_mask_*        streams pi once, a wave per row, into node-major bits in community order: bit k & 63 of word
//                         k >> 6 of the row.  The generic form reads 64 consecutive columns per ballot, which is the word.
//                         The fast form loads 16 bytes per lane, so a ballot holds every fourth column of 256; a lane then
//                         takes the 16-bit slice of its word's 64 columns out of the four ballots of a load and spreads
//                         each to every fourth bit.  The read of pi bounds both.
//   connect_edges_direct  a wave per edge.  b's set bits are compacted into a wave-private list in LDS (2-byte entries,
//                         the words of b in halves of 64, so a wave's list is 8 KiB); a's set bits are walked
//                         wave-uniformly and for each the lanes stride over the list, one 64-bit vector atomic per cell
//                         of directed[k, l].  Sum over the edges of |S_a| |S_b| atomics to L2, which bound it.
//   connect_edges_runs    a wave per chunk of RUN_CHUNK consecutive edges, a group of lanes (the smallest power of two
//                         >= W) per edge.  Over a run of equal high ends it adds b's bits into wave-private counters h
//                         in LDS and keeps the OR of b's words; at the run's end h[l] goes to directed[k, l] for every k
//                         of a and every l of the OR, and those counters are cleared.  The atomics per run are |S_a| times
//                         the distinct communities of the run's neighbours.
//   connect_finish        links = directed + directed^T.
//   connect_top           ammsb_relate.hip's relate_top over 64-bit link counts and the pair counts d_k d_l - overlap.
//
// The mask's layout, and the rule that its readers (the edge kernels here among them) clear the bits past K, are stated
// once, in ammsb_postfit.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/ammsb_connect.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int C_WAVES = 4;  // waves per block
constexpr int C_BLOCK = 64 * C_WAVES;

// LDS traffic between the lanes of one wave: the wave's DS operations execute in order; this keeps the compiler from
// moving them across
__device__ __forceinline__ void wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
  __builtin_amdgcn_wave_barrier();
}

// lane src's value in every lane; src is wave-uniform
__device__ __forceinline__ u64 read_lane64(u64 v, int src) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, src);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), src);
  return ((u64)hi << 32) | lo;
}

__device__ __forceinline__ u64 shfl_xor64(u64 v, int s) {
  const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, s, 64);
  const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), s, 64);
  return ((u64)hi << 32) | lo;
}

// ------------------------------------------------------------------------------------------ the mask pass
struct MaskArgs {
  ammsb_rpm pi;
  float thr;
  u64* mask;
};

// bit j of the low 16 -> bit 4 j
__device__ __forceinline__ u64 spread4(u64 x) {
  x = (x | (x << 24)) & 0x000000FF000000FFull;
  x = (x | (x << 12)) & 0x000F000F000F000Full;
  x = (x | (x << 6)) & 0x0303030303030303ull;
  x = (x | (x << 3)) & 0x1111111111111111ull;
  return x;
}

// A chunk is 1024 columns: up to 4 loads of 16 bytes per lane, load i of lane j being columns 1024 ch + 256 i + 4 j + c.
// Its 16 words, 16 ch + 4 i + q, are the columns 64 q .. 64 q + 63 of load i: component c of lanes 16 q .. 16 q + 15 at
// bits 4 (j - 16 q) + c.  Word t is kept by lane t & 63, so chunk ch lands in the 16 lanes (ch & 3) 16 .., lane j of
// them with i = (j >> 2) & 3 and q = j & 3.
__global__ __launch_bounds__(C_BLOCK) void connect_mask_fast(MaskArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = K >> 6;
  const int nvK = (int)(K >> 8), nch = (nvK + 3) >> 2;
  const int mi = (lane >> 2) & 3, mq = lane & 3;
  const uint64_t rows = a.pi.num_rows, stride = (uint64_t)gridDim.x * C_WAVES;
  for (uint64_t r = (uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const float4* p = reinterpret_cast<const float4*>(postfit_row(a.pi, (uint32_t)r)) + lane;
    u64 w0 = 0, w1 = 0;
    for (int ch = 0; ch < nch; ++ch) {
      const int nv = min(nvK - 4 * ch, 4);
      const float4 none = {-1.f, -1.f, -1.f, -1.f};  // below every threshold the entry point lets through
      float4 x[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        x[i] = none;
        if (i < nv) x[i] = p[(ch * 4 + i) * 64];
      }
      u64 word = 0;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        u64 b[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) b[i] = __ballot(comp(x[i], c) >= a.thr);
        const u64 mine = mi == 0 ? b[0] : mi == 1 ? b[1] : mi == 2 ? b[2] : b[3];
        word |= spread4((mine >> (16 * mq)) & 0xFFFFull) << c;
      }
      if ((lane >> 4) == (ch & 3)) {
        if (ch < 4) w0 = word;
        else w1 = word;
      }
    }
    store_bit_row(a.mask, r, W, w0, w1, lane);
  }
}

__global__ __launch_bounds__(C_BLOCK) void connect_mask_generic(MaskArgs a) {
  const int lane = threadIdx.x & 63;
  const uint32_t K = (uint32_t)a.pi.num_cols, W = (K + 63u) >> 6;
  const uint64_t rows = a.pi.num_rows, stride = (uint64_t)gridDim.x * C_WAVES;
  for (uint64_t r = (uint64_t)blockIdx.x * C_WAVES + (threadIdx.x >> 6); r < rows; r += stride) {
    const float* p = postfit_row(a.pi, (uint32_t)r);
    u64 w0 = 0, w1 = 0;
    for (uint32_t t = 0; t < W; ++t) {
      const uint32_t col = 64u * t + (uint32_t)lane;
      const float v = col < K ? p[col] : -1.0f;  // (below every threshold)
      place(w0, w1, t, __ballot(v >= a.thr), lane);
    }
    store_bit_row(a.mask, r, W, w0, w1, lane);
  }
}

// ------------------------------------------------------------------------------------------ the edge pass
constexpr uint32_t LIST_CAP = 64 * 64;    // the set bits of 64 words at most
constexpr uint32_t DIRECT_TRIPS = 1;      // edges a wave of connect_edges_direct takes before another block is worth it
constexpr uint32_t RUN_CHUNK = 128;       // consecutive edges a wave of connect_edges_runs owns at a time
constexpr uint32_t RUNS_GRID = 1024;      // blocks of connect_edges_runs at most: its counters leave room for 2..8 per CU

struct EdgeArgs {
  const u64* mask;
  uint32_t rows, K, W;
  uint32_t gshift;  // runs: log2 of the lanes that own an edge, the smallest power of two >= W
  const u64* edges;
  uint64_t n;
  u64* directed;
  u64* counts;
};

// every lane's exclusive prefix sum of v over the wave, and the sum
__device__ __forceinline__ uint32_t wave_prefix(uint32_t v, int lane, uint32_t* total) {
  uint32_t s = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t t = (uint32_t)__shfl_up((int)s, o, 64);
    if (lane >= o) s += t;
  }
  *total = (uint32_t)__builtin_amdgcn_readlane((int)s, 63);
  return s - v;
}

__device__ __forceinline__ void add_counts(const EdgeArgs& a, int lane, u64 valid, u64 skipped) {
  if (lane == 0) {
    if (valid) atomicAdd(&a.counts[0], valid);
    if (skipped) atomicAdd(&a.counts[1], skipped);
  }
}

__global__ __launch_bounds__(C_BLOCK) void connect_edges_direct(EdgeArgs a) {
  __shared__ uint16_t lists[C_WAVES][LIST_CAP];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint16_t* list = lists[wave];
  const uint32_t K = a.K, W = a.W;
  const uint64_t stride = (uint64_t)gridDim.x * C_WAVES;
  u64 valid = 0, skipped = 0;  // of this wave's edges: wave-uniform
  for (uint64_t p = (uint64_t)blockIdx.x * C_WAVES + wave; p < a.n; p += stride) {
    const u64 key = a.edges[p];
    const uint32_t u = (uint32_t)(key >> 32), v = (uint32_t)key;
    if (u >= a.rows || v >= a.rows) {
      ++skipped;
      continue;
    }
    ++valid;
    u64 x[2], y[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      x[i] = mask_word(a, u, (uint32_t)lane + 64u * i);
      y[i] = mask_word(a, v, (uint32_t)lane + 64u * i);
    }
    const u64 holds[2] = {__ballot(x[0] != 0), __ballot(x[1] != 0)};  // the lanes with a word of a that has a bit
    if (!(holds[0] | holds[1])) continue;
#pragma unroll
    for (int h = 0; h < 2; ++h) {  // b's words 64 h .. 64 h + 63: communities 4096 h ..
      if (64u * h >= W) break;
      uint32_t total;
      uint32_t at = wave_prefix((uint32_t)__popcll(y[h]), lane, &total);  // (total <= LIST_CAP)
      if (total == 0) continue;
      wave_sync();  // the list's last readers are through
      for (u64 bits = y[h]; bits; bits &= bits - 1) list[at++] = (uint16_t)(64u * lane + (uint32_t)__builtin_ctzll(bits));
      wave_sync();
#pragma unroll
      for (int g = 0; g < 2; ++g) {
        for (u64 nz = holds[g]; nz; nz &= nz - 1) {
          const int src = __builtin_ctzll(nz);
          for (u64 word = read_lane64(x[g], src); word; word &= word - 1) {
            const uint32_t k = 64u * (64u * g + (uint32_t)src) + (uint32_t)__builtin_ctzll(word);  // (< K: live_bits)
            u64* row = a.directed + (uint64_t)k * K + 4096u * h;
            for (uint32_t j = lane; j < total; j += 64) atomicAdd(&row[list[j]], 1ull);
          }
        }
      }
    }
  }
  add_counts(a, lane, valid, skipped);
}

// the end of a run of connect_edges_runs: h[l] to directed[k, l] for every k of xa (a's words, word w in lane w) and every
// l of acc (the OR of the run's words of b, word gl in every lane of a group), and h clear again
__device__ __forceinline__ void flush_run(const EdgeArgs& a, uint32_t* h, u64 xa, u64& acc, uint32_t G, int lane) {
  for (uint32_t o = G; o < 64u; o <<= 1) acc |= shfl_xor64(acc, (int)o);  // over the groups: word gl of every edge
  const u64 mine = (uint32_t)lane < a.W ? acc : 0ull;  // (lane < W <= G: gl == lane)
  wave_sync();  // the run's adds to h are through
  for (u64 nz = __ballot(xa != 0); nz; nz &= nz - 1) {
    const int src = __builtin_ctzll(nz);
    for (u64 word = read_lane64(xa, src); word; word &= word - 1) {
      u64* row = a.directed + (uint64_t)(64u * (uint32_t)src + (uint32_t)__builtin_ctzll(word)) * a.K;
      for (u64 bits = mine; bits; bits &= bits - 1) {
        const uint32_t l = 64u * (uint32_t)lane + (uint32_t)__builtin_ctzll(bits);  // (< K: live_bits)
        atomicAdd(&row[l], (u64)h[l]);
      }
    }
  }
  for (u64 bits = mine; bits; bits &= bits - 1) h[64u * (uint32_t)lane + (uint32_t)__builtin_ctzll(bits)] = 0;
  acc = 0;
  wave_sync();
}

__global__ __launch_bounds__(C_BLOCK) void connect_edges_runs(EdgeArgs a) {
  extern __shared__ uint32_t lds[];  // [C_WAVES][64 W]
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t W = a.W, G = 1u << a.gshift, gl = (uint32_t)lane & (G - 1u), slot = (uint32_t)lane >> a.gshift;
  const uint32_t epw = 64u >> a.gshift;  // edges per step of the wave
  uint32_t* h = lds + (uint32_t)wave * 64u * W;
  for (uint32_t l = lane; l < 64u * W; l += 64) h[l] = 0;
  wave_sync();
  const uint64_t chunks = (a.n + RUN_CHUNK - 1) / RUN_CHUNK, stride = (uint64_t)gridDim.x * C_WAVES;
  u64 valid = 0, skipped = 0;
  for (uint64_t c = (uint64_t)blockIdx.x * C_WAVES + wave; c < chunks; c += stride) {
    const uint64_t e0 = c * RUN_CHUNK, e1 = a.n - e0 < RUN_CHUNK ? a.n : e0 + RUN_CHUNK;
    bool have = false;  // a run is open: cur is its high end, xa its words, any: it holds a community at all
    bool any = false;
    uint32_t cur = 0;
    u64 xa = 0, acc = 0;
    for (uint64_t pb = e0; pb < e1; pb += epw) {  // (RUN_CHUNK is a multiple of epw)
      const uint64_t p = pb + slot;
      const bool exists = p < e1;
      uint32_t u = 0, v = 0;
      bool ok = false;
      if (exists) {
        const u64 key = a.edges[p];
        u = (uint32_t)(key >> 32);
        v = (uint32_t)key;
        ok = u < a.rows && v < a.rows;
      }
      const u64 y = ok ? mask_word(a, v, gl) : 0ull;
      valid += (u64)__popcll(__ballot(ok && gl == 0));
      skipped += (u64)__popcll(__ballot(exists && !ok && gl == 0));
      // the step's edges in rounds of equal high ends; which edges share a round does not matter to the sums
      for (u64 pending = __ballot(ok); pending;) {
        const uint32_t a0 = (uint32_t)__builtin_amdgcn_readlane((int)u, __builtin_ctzll(pending));
        if (!have || a0 != cur) {
          if (have && any) flush_run(a, h, xa, acc, G, lane);
          have = true;
          cur = a0;
          xa = mask_word(a, a0, (uint32_t)lane);
          any = __ballot(xa != 0) != 0;
        }
        const bool mine = ok && u == a0;  // (every lane of a group alike)
        if (mine && any) {
          for (u64 bits = y; bits; bits &= bits - 1) atomicAdd(&h[64u * gl + (uint32_t)__builtin_ctzll(bits)], 1u);
          acc |= y;
        }
        pending &= ~__ballot(mine);
      }
    }
    if (have && any) flush_run(a, h, xa, acc, G, lane);
  }
  add_counts(a, lane, valid, skipped);
}

// ------------------------------------------------------------------------------------------ links = directed + directed^T
__global__ __launch_bounds__(C_BLOCK) void connect_finish(const u64* directed, uint32_t K, u64* links) {
  const uint64_t cells = (uint64_t)K * K, stride = (uint64_t)gridDim.x * C_BLOCK;
  for (uint64_t i = (uint64_t)blockIdx.x * C_BLOCK + threadIdx.x; i < cells; i += stride) {
    const uint64_t k = i / K, l = i % K;
    links[i] = directed[i] + directed[l * K + k];
  }
}

// ------------------------------------------------------------------------------------------ the partners
struct TopArgs {
  const u64* links;         // [K, K]
  const uint32_t* overlap;  // [K, K]
  uint32_t K, measure, top;
  u64 min_links;  // >= 1
  int32_t* partner;   // [K, top]
  u64* plinks;        // [K, top]
  uint32_t* pshared;  // [K, top]
};

// A candidate partner is (w, den, l): w links over den pairs (the measure is w / den); w == 0: none.
// Does x come before y in the ranking?  w_x / den_x > w_y / den_y as w_x den_y > w_y den_x in 128 bits, then the lower l.
__device__ __forceinline__ bool before(u64 xw, u64 xden, uint32_t xl, u64 yw, u64 yden, uint32_t yl) {
  const u64 lh = __umul64hi(xw, yden), ll = xw * yden;
  const u64 rh = __umul64hi(yw, xden), rl = yw * xden;
  if (lh != rh) return lh > rh;
  if (ll != rl) return ll > rl;
  return xl < yl;
}

// (bw, bden, bl) = whichever of it and (w, den, l) comes first
__device__ __forceinline__ void offer_cand(u64& bw, u64& bden, uint32_t& bl, u64 w, u64 den, uint32_t l) {
  const bool take = w != 0 && (bw == 0 || before(w, den, l, bw, bden, bl));
  bw = take ? w : bw;
  bden = take ? den : bden;
  bl = take ? l : bl;
}

__global__ __launch_bounds__(C_BLOCK) void connect_top(TopArgs a) {
  __shared__ uint32_t diag[AMMSB_CONNECT_MAX_COLS];
  const uint32_t K = a.K, lane = threadIdx.x & 63u;
  for (uint32_t l = threadIdx.x; l < K; l += C_BLOCK) diag[l] = a.overlap[(u64)l * K + l];
  __syncthreads();
  const uint32_t k = blockIdx.x * C_WAVES + (threadIdx.x >> 6);
  if (k >= K) return;  // (wave-uniform, after the only barrier)
  const u64* row = a.links + (u64)k * K;
  const uint32_t* orow = a.overlap + (u64)k * K;
  const u64 dk = diag[k];
  u64 pw = 0, pden = 1;  // the previous round's winner
  uint32_t pl = 0;
  for (uint32_t t = 0; t < a.top; ++t) {
    u64 bw = 0, bden = 1;
    uint32_t bl = 0;
    for (uint32_t l = lane; l < K; l += 64) {
      const u64 w = row[l];
      if (l == k || w < a.min_links) continue;
      u64 den = 1;
      if (a.measure == AMMSB_CONNECT_DENSITY) {
        den = dk * (u64)diag[l] - (u64)orow[l];
        if (den == 0) continue;  // no pair of distinct nodes: no density
      }
      if (t > 0 && !before(pw, pden, pl, w, den, l)) continue;  // taken in an earlier round
      offer_cand(bw, bden, bl, w, den, l);
    }
    // every lane ends with the wave's first: the order is total, so the butterfly's partners agree
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {
      const u64 ow = shfl_xor64(bw, s), oden = shfl_xor64(bden, s);
      const uint32_t ol = (uint32_t)__shfl_xor((int)bl, s, 64);
      offer_cand(bw, bden, bl, ow, oden, ol);
    }
    if (bw == 0) {  // nothing left: the empty slots
      for (uint32_t s = t + lane; s < a.top; s += 64) {
        a.partner[(u64)k * a.top + s] = -1;
        a.plinks[(u64)k * a.top + s] = 0;
        a.pshared[(u64)k * a.top + s] = 0;
      }
      break;
    }
    if (lane == 0) {
      a.partner[(u64)k * a.top + t] = (int32_t)bl;
      a.plinks[(u64)k * a.top + t] = bw;
      a.pshared[(u64)k * a.top + t] = orow[bl];
    }
    pw = bw;
    pden = bden;
    pl = bl;
  }
}

const char* check_cols(uint32_t K) { return (K == 0 || K > AMMSB_CONNECT_MAX_COLS) ? "num_cols outside 1..8192" : nullptr; }

}  // namespace

extern "C" const char* ammsb_connect_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_connect_last_error(void) { return g_last_error; }

extern "C" uint64_t ammsb_connect_mask_bytes(uint64_t num_rows, uint32_t num_cols) {
  if (check_cols(num_cols) || (num_rows >> 32)) return 0;
  return num_rows * ((num_cols + 63u) / 64u) * sizeof(uint64_t);
}

extern "C" int ammsb_connect_mask(const ammsb_rpm* pi, float thr, uint64_t* mask, void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (!(thr >= 0.0f && thr < INFINITY)) return fail(AMMSB_EINVAL, "thr negative, NaN or infinite");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_CONNECT_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (reinterpret_cast<uintptr_t>(mask) & 7) return fail(AMMSB_EINVAL, "mask is not 8-byte aligned");
  if (pi->num_rows == 0) return AMMSB_OK;

  MaskArgs a;
  a.pi = *pi;
  a.thr = thr;
  a.mask = reinterpret_cast<u64*>(mask);
  const dim3 grid(persistent_grid(pi->num_rows, C_WAVES)), block(C_BLOCK);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (pi->num_cols % 256 == 0 && aligned) {
    hipLaunchKernelGGL(connect_mask_fast, grid, block, 0, s, a);
    return launched("connect_mask_fast");
  }
  hipLaunchKernelGGL(connect_mask_generic, grid, block, 0, s, a);
  return launched("connect_mask_generic");
}

extern "C" int ammsb_connect_edges(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* edges,
                                   uint64_t n, uint64_t* directed, uint64_t* counts, void* stream) {
  if (n > 0 && !mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (n > 0 && !edges) return fail(AMMSB_EINVAL, "edges is NULL");
  if (!directed) return fail(AMMSB_EINVAL, "directed is NULL");
  if (!counts) return fail(AMMSB_EINVAL, "counts is NULL");
  if (const char* bad = check_cols(num_cols)) return fail(AMMSB_EINVAL, bad);
  if (num_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  // AMMSB_CONNECT_FORM: d or r, read at every call so that one process can take both
  const char* form = getenv("AMMSB_CONNECT_FORM");
  if (form && !((form[0] == 'd' || form[0] == 'r') && form[1] == 0))
    return fail(AMMSB_EINVAL, "AMMSB_CONNECT_FORM is neither d nor r");
  if (n == 0) return AMMSB_OK;

  EdgeArgs a;
  a.mask = reinterpret_cast<const u64*>(mask);
  a.rows = (uint32_t)num_rows;
  a.K = num_cols;
  a.W = (num_cols + 63u) / 64u;
  a.gshift = 0;
  while ((1u << a.gshift) < a.W && a.gshift < 6) ++a.gshift;
  a.edges = reinterpret_cast<const u64*>(edges);
  a.n = n;
  a.directed = reinterpret_cast<u64*>(directed);
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the runs form wherever it exists: on a sorted assortative list at N = 1e6, K = 1024 it took 4.75 ms against the direct
  // form's 8.59 ms (tools/connect_ab.py, profiles/connect_ab.json)
  const bool runs = !(form && form[0] == 'd') && num_cols <= AMMSB_CONNECT_RUNS_MAX_COLS;
  if (runs) {
    const uint64_t chunks = (n + RUN_CHUNK - 1) / RUN_CHUNK, want = (chunks + C_WAVES - 1) / C_WAVES;
    const dim3 grid((unsigned)(want < RUNS_GRID ? want : RUNS_GRID)), block(C_BLOCK);
    const size_t lds = (size_t)C_WAVES * 64u * a.W * sizeof(uint32_t);  // (<= 64 KiB: W <= 64)
    hipLaunchKernelGGL(connect_edges_runs, grid, block, lds, s, a);
    return launched("connect_edges_runs");
  }
  const dim3 grid(persistent_grid(n, (uint64_t)C_WAVES * DIRECT_TRIPS)), block(C_BLOCK);
  hipLaunchKernelGGL(connect_edges_direct, grid, block, 0, s, a);
  return launched("connect_edges_direct");
}

extern "C" int ammsb_connect_finish(const uint64_t* directed, uint32_t num_cols, uint64_t* links, void* stream) {
  if (!directed) return fail(AMMSB_EINVAL, "directed is NULL");
  if (!links) return fail(AMMSB_EINVAL, "links is NULL");
  if (links == directed) return fail(AMMSB_EINVAL, "links and directed are the same buffer");
  if (const char* bad = check_cols(num_cols)) return fail(AMMSB_EINVAL, bad);
  const dim3 grid(persistent_grid((uint64_t)num_cols * num_cols, C_BLOCK)), block(C_BLOCK);
  hipLaunchKernelGGL(connect_finish, grid, block, 0, static_cast<hipStream_t>(stream),
                     reinterpret_cast<const u64*>(directed), num_cols, reinterpret_cast<u64*>(links));
  return launched("connect_finish");
}

extern "C" int ammsb_connect_top(const uint64_t* links, const uint32_t* overlap, uint32_t num_cols, uint32_t measure,
                                 uint32_t top, uint64_t min_links, int32_t* partner, uint64_t* plinks, uint32_t* pshared,
                                 void* stream) {
  if (!links) return fail(AMMSB_EINVAL, "links is NULL");
  if (!overlap) return fail(AMMSB_EINVAL, "overlap is NULL");
  if (!partner) return fail(AMMSB_EINVAL, "partner is NULL");
  if (!plinks) return fail(AMMSB_EINVAL, "plinks is NULL");
  if (!pshared) return fail(AMMSB_EINVAL, "pshared is NULL");
  if (const char* bad = check_cols(num_cols)) return fail(AMMSB_EINVAL, bad);
  if (measure != AMMSB_CONNECT_LINKS && measure != AMMSB_CONNECT_DENSITY)
    return fail(AMMSB_EINVAL, "measure is neither links nor density");
  if (top == 0 || top > AMMSB_CONNECT_MAX_TOP) return fail(AMMSB_EINVAL, "top outside 1..64");

  TopArgs a;
  a.links = reinterpret_cast<const u64*>(links);
  a.overlap = overlap;
  a.K = num_cols;
  a.measure = measure;
  a.top = top;
  a.min_links = min_links ? min_links : 1u;
  a.partner = partner;
  a.plinks = reinterpret_cast<u64*>(plinks);
  a.pshared = pshared;
  const dim3 grid((num_cols + C_WAVES - 1) / C_WAVES), block(C_BLOCK);
  hipLaunchKernelGGL(connect_top, grid, block, 0, static_cast<hipStream_t>(stream), a);
  return launched("connect_top");
}
