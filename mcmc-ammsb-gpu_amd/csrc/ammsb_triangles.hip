// libammsb_triangles.so (include/ammsb_triangles.h): per node of a simple CSR adjacency its triangles, those whose three
// corners share a community of the detected cover, and per community the triangles inside it (three times) and the
// members that take part in one.
//
//   triangles_nodes_w1 / _w2   a wave owns a node a.  Lane l holds word l (and l + 64 in the two-word form above K = 4096)
//                          of a row of membership bits.  The row of a goes into the wave's LDS where it has at most ROW_LDS
//                          targets; a longer one stays in global memory and is read through the same accessor (a runtime
//                          branch, not a third form).  For each neighbour b the triangles {b, c} with c > b are the
//                          intersection of two sorted lists, the row of a after b and the row of b above b: the shorter
//                          one gives the candidates, 64 at a time, one per lane, and each is binary-searched in the other
//                          inside that list's bounds; a ballot collects the hits.  Where S_a & S_b is empty wave-wide
//                          (one ballot) the hits are only counted.  Otherwise the rows of bits of TRI_FLIGHT hits are
//                          requested together (each W words, coalesced), m = S_a & S_b & S_c, one ballot gives tri_in,
//                          and each lane walks the set bits of its word of m and increments counters it alone owns in the
//                          wave's private u32 h[64 W].  Counter (w, t) lives at t W + w, not at 64 w + t: the lanes of one
//                          request differ in w, so they fall on different banks whatever their bits t are.  No LDS
//                          atomics.  A lane ORs the words it has touched; at the row's end it walks only those bits for
//                          ktri3, kpart and tri_comms and sets the counters back to zero, so h is clean for the next row.
//                          Bounded by the dependent loads of the searches (log2 of the other list's length per batch).
//
// Rows go to the waves of a persistent grid in turn (wave g takes rows g, g + G, ...).  A hub row is walked by its one
// wave.
//
// The mask is read through mask_word() of ammsb_postfit.h alone (bits past K cleared).  Every index into the mask (a W)
// and into targets is 64-bit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_triangles.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int TRI_FLIGHT = 4;  // hits whose rows of bits are requested before the first is counted
constexpr int TRI_TRIPS = 2;   // rows a wave takes before another block is worth it
constexpr int W1_WAVES = 2;    // h is at most 16 KiB per wave (K <= 4096) and the row 4 KiB: 40 KiB per block
constexpr int W2_WAVES = 1;    // at most 32 KiB per wave (K <= 8192) and the row 4 KiB: 36 KiB per block
constexpr uint32_t ROW_LDS = AMMSB_TRIANGLES_ROW_LDS;

struct Args {
  const u64* mask;
  uint32_t rows, K, W;
  const u64* offsets;
  const uint32_t* targets;
  uint64_t first, n;  // the node range
  uint32_t *tri, *tri_in, *tri_comms;
  u64 *ktri3, *kpart, *counts;
};

// every lane ends with the sum
__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// lane j's value (j wave-uniform) in every lane
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, uint32_t j) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, (int)(j & 63u));
}

__device__ __forceinline__ u64 lane_u64(u64 v, uint32_t j) {
  return ((u64)lane_u32((uint32_t)(v >> 32), j) << 32) | lane_u32((uint32_t)v, j);
}

// A sorted row: `len` targets at positions 0 .. len - 1, in the wave's LDS or at targets[beg ..] (a 64-bit index).
struct Row {
  const uint32_t* lds;  // the copy, where in_lds
  const uint32_t* at;   // targets + beg
  bool in_lds;
};

__device__ __forceinline__ uint32_t elem(const Row& r, uint64_t i) { return r.in_lds ? r.lds[(uint32_t)i] : r.at[i]; }

// the first position in [lo, hi) whose target is >= v, or hi: every read is at a position inside [lo, hi)
__device__ __forceinline__ uint64_t lower_bound(const Row& r, uint64_t lo, uint64_t hi, uint32_t v) {
  uint64_t n = hi - lo;
  while (n) {
    const uint64_t half = n >> 1;
    if (elem(r, lo + half) < v) {
      lo += half + 1;
      n -= half + 1;
    } else {
      n = half;
    }
  }
  return lo;
}

// what one lane wrote to the wave's LDS is what the others read after this
__device__ __forceinline__ void wave_lds_fence() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <int WPL, int WAVES>
__device__ __forceinline__ void nodes_body(const Args& a) {
  extern __shared__ uint32_t lds[];  // WAVES x 64 W counters, all zero between two rows; then WAVES x ROW_LDS targets
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = a.W;
  uint32_t* h = lds + (size_t)wave * 64u * W;
  uint32_t* copy = lds + (size_t)WAVES * 64u * W + (size_t)wave * ROW_LDS;
  for (uint32_t s = lane; s < 64u * W; s += 64u) h[s] = 0;  // (the wave's own part: no barrier)
  const uint64_t stride = (uint64_t)gridDim.x * WAVES;
  u64 total = 0, skipped = 0;  // of this wave's rows: wave-uniform
  for (uint64_t r = (uint64_t)blockIdx.x * WAVES + wave; r < a.n; r += stride) {
    const uint32_t node = (uint32_t)(a.first + r);  // (< rows: the entry point checked the range)
    const uint64_t beg = a.offsets[node], end = a.offsets[node + 1];
    const uint64_t da = end > beg ? end - beg : 0;
    if (da == 0) {  // (wave-uniform) no neighbour: no row of bits is read
      if (lane == 0) a.tri[node] = a.tri_in[node] = a.tri_comms[node] = 0;
      continue;
    }
    u64 xa[WPL], seen[WPL];
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      xa[i] = mask_word(a, node, lane + 64u * i);
      seen[i] = 0;
    }
    Row ra = {copy, a.targets + beg, da <= ROW_LDS};
    wave_lds_fence();  // (the previous row's reads of the copy are over)
    if (ra.in_lds) {
      for (uint64_t s = lane; s < da; s += 64) copy[s] = a.targets[beg + s];
      wave_lds_fence();
    }
    uint32_t tri = 0, tri_in = 0;  // wave-uniform
    for (uint64_t p = 0; p < da; p += 64) {
      const uint64_t left = da - p;
      const uint32_t cnt = left < 64 ? (uint32_t)left : 64u;
      // 64 neighbours and the bounds of their rows in one request each
      const uint32_t mine = lane < cnt ? elem(ra, p + lane) : 0xFFFFFFFFu;
      const bool inside = mine < a.rows;
      const u64 obeg = inside ? a.offsets[mine] : 0ull, oend = inside ? a.offsets[(uint64_t)mine + 1] : 0ull;
      skipped += (u64)__popcll(__ballot(lane < cnt && !inside));
      for (uint32_t j = 0; j < cnt; ++j) {  // (wave-uniform)
        const uint32_t b = lane_u32(mine, j);
        const uint64_t after = p + j + 1;  // the row of a after b: positions after .. da - 1
        if (b >= a.rows || after >= da) continue;
        const uint64_t bb = lane_u64(obeg, j), be = lane_u64(oend, j);
        const uint64_t db = be > bb ? be - bb : 0;
        if (db == 0) continue;
        u64 sab[WPL], any = 0;
#pragma unroll
        for (int i = 0; i < WPL; ++i) {  // (on its way during the search below)
          sab[i] = xa[i] & mask_word(a, b, lane + 64u * i);
          any |= sab[i];
        }
        const Row rb = {copy, a.targets + bb, false};
        const uint64_t above = lower_bound(rb, 0, db, b + 1u);  // the row of b above b: positions above .. db - 1
        if (above >= db) continue;
        // candidates from the shorter list, searched in the other
        const bool from_a = da - after <= db - above;
        const Row& rc = from_a ? ra : rb;
        const Row& ro = from_a ? rb : ra;
        const uint64_t cbeg = from_a ? after : above, cend = from_a ? da : db;
        const uint64_t sbeg = from_a ? above : after, send = from_a ? db : da;
        const bool share = __ballot(any != 0) != 0;  // S_a & S_b is not empty
        for (uint64_t q = cbeg; q < cend; q += 64) {
          const bool has = q + lane < cend;
          const uint32_t cand = has ? elem(rc, q + lane) : 0xFFFFFFFFu;
          bool found = false;
          if (has && cand < a.rows) {
            const uint64_t at = lower_bound(ro, sbeg, send, cand);
            found = at < send && elem(ro, at) == cand;
          }
          u64 hits = __ballot(found);
          tri += (uint32_t)__popcll(hits);
          if (!share) continue;  // no row of bits of c is read
          while (hits) {
            u64 y[TRI_FLIGHT][WPL];
            bool ok[TRI_FLIGHT];
#pragma unroll
            for (int f = 0; f < TRI_FLIGHT; ++f) {  // the trip's rows of bits are on their way together
              ok[f] = hits != 0;
              const uint32_t from = ok[f] ? (uint32_t)__builtin_ctzll(hits) : 0u;
              hits &= hits - 1;  // (0 stays 0)
              const uint32_t c = lane_u32(cand, from);  // (< rows where ok: found)
#pragma unroll
              for (int i = 0; i < WPL; ++i) y[f][i] = ok[f] ? mask_word(a, c, lane + 64u * i) : 0ull;
            }
#pragma unroll
            for (int f = 0; f < TRI_FLIGHT; ++f) {
              if (!ok[f]) continue;  // (wave-uniform)
              u64 in = 0;
#pragma unroll
              for (int i = 0; i < WPL; ++i) {
                const u64 m = sab[i] & y[f][i];
                in |= m;
                seen[i] |= m;
                const uint32_t w = lane + 64u * i;
                for (u64 bits = m; bits; bits &= bits - 1) ++h[(uint32_t)__builtin_ctzll(bits) * W + w];  // (bits != 0: w < W)
              }
              tri_in += (uint32_t)(__ballot(in != 0) != 0);
            }
          }
        }
      }
    }
    total += tri;

    // the row's end: only the counters that were touched
    uint32_t comms = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const uint32_t w = lane + 64u * i;
      comms += (uint32_t)__popcll(seen[i]);
      for (u64 bits = seen[i]; bits; bits &= bits - 1) {
        const uint32_t t = (uint32_t)__builtin_ctzll(bits);
        atomicAdd(&a.ktri3[64u * w + t], (u64)h[t * W + w]);  // (k = 64 w + t < K: live_bits)
        atomicAdd(&a.kpart[64u * w + t], 1ull);
        h[t * W + w] = 0;
      }
    }
    comms = wave_sum_u32(comms);
    if (lane == 0) {
      a.tri[node] = tri;
      a.tri_in[node] = tri_in;
      a.tri_comms[node] = comms;
    }
  }
  if (lane == 0) {
    if (total) atomicAdd(&a.counts[0], total);
    if (skipped) atomicAdd(&a.counts[1], skipped);
  }
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(64 * W1_WAVES) void triangles_nodes_w1(Args a) { nodes_body<1, W1_WAVES>(a); }
__global__ __launch_bounds__(64 * W2_WAVES) void triangles_nodes_w2(Args a) { nodes_body<2, W2_WAVES>(a); }


}  // namespace

extern "C" const char* ammsb_triangles_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_triangles_last_error(void) { return g_last_error; }

extern "C" int ammsb_triangles_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* offsets,
                                     const uint32_t* targets, uint64_t first_row, uint64_t n_rows, uint32_t* tri,
                                     uint32_t* tri_in, uint32_t* tri_comms, uint64_t* ktri3, uint64_t* kpart, uint64_t* counts,
                                     void* stream) {
  if (!mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (!offsets) return fail(AMMSB_EINVAL, "offsets is NULL");
  if (!targets) return fail(AMMSB_EINVAL, "targets is NULL");
  if (!tri || !tri_in || !tri_comms) return fail(AMMSB_EINVAL, "tri, tri_in or tri_comms is NULL");
  if (!ktri3 || !kpart) return fail(AMMSB_EINVAL, "ktri3 or kpart is NULL");
  if (!counts) return fail(AMMSB_EINVAL, "counts is NULL");
  if (num_cols == 0 || num_cols > AMMSB_TRIANGLES_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (num_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (first_row > num_rows || n_rows > num_rows - first_row) return fail(AMMSB_EINVAL, "first_row + n_rows is past num_rows");
  if (misaligned(mask, 8) || misaligned(offsets, 8)) return fail(AMMSB_EINVAL, "mask or offsets is not 8-byte aligned");
  if (misaligned(targets, 4)) return fail(AMMSB_EINVAL, "targets is not 4-byte aligned");
  if (misaligned(tri, 4) || misaligned(tri_in, 4) || misaligned(tri_comms, 4))
    return fail(AMMSB_EINVAL, "tri, tri_in or tri_comms is not 4-byte aligned");
  if (misaligned(ktri3, 8) || misaligned(kpart, 8) || misaligned(counts, 8))
    return fail(AMMSB_EINVAL, "ktri3, kpart or counts is not 8-byte aligned");
  if (n_rows == 0) return AMMSB_OK;

  Args a;
  a.mask = reinterpret_cast<const u64*>(mask);
  a.rows = (uint32_t)num_rows;
  a.K = num_cols;
  a.W = (num_cols + 63u) / 64u;
  a.offsets = reinterpret_cast<const u64*>(offsets);
  a.targets = targets;
  a.first = first_row;
  a.n = n_rows;
  a.tri = tri;
  a.tri_in = tri_in;
  a.tri_comms = tri_comms;
  a.ktri3 = reinterpret_cast<u64*>(ktri3);
  a.kpart = reinterpret_cast<u64*>(kpart);
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  // per wave: h, at most 16 KiB (w1) or 32 KiB (w2), and the copy of a row, 4 KiB
  const size_t per_wave = ((size_t)64 * a.W + ROW_LDS) * sizeof(uint32_t);
  if (num_cols <= AMMSB_TRIANGLES_W1_MAX_COLS) {
    const dim3 grid(persistent_grid(n_rows, (uint64_t)W1_WAVES * TRI_TRIPS));
    hipLaunchKernelGGL(triangles_nodes_w1, grid, dim3(64 * W1_WAVES), W1_WAVES * per_wave, s, a);
    return launched("triangles_nodes_w1");
  }
  const dim3 grid(persistent_grid(n_rows, (uint64_t)W2_WAVES * TRI_TRIPS));
  hipLaunchKernelGGL(triangles_nodes_w2, grid, dim3(64 * W2_WAVES), W2_WAVES * per_wave, s, a);
  return launched("triangles_nodes_w2");
}
