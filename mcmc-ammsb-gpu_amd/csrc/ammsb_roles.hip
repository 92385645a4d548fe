// libammsb_roles.so (include/ammsb_roles.h): per node of a CSR adjacency, how many of its neighbours are in each community
// of the detected cover, reduced per node (degree, embedded, reached, votes, squares, the `top` communities its
// neighbourhood votes for) and per community (ksum, ksq, kmembers).
//
//   roles_nodes_w1 / _w2   a wave owns a node.  Lane l holds word l (and l + 64 in the two-word form above K = 4096) of a row
//                          of membership bits and alone owns that word's 64 counters of the wave's private u32 h[64 W] in
//                          LDS: counting needs no LDS atomics and no lane meets another's counter.  Counter (w, t) lives at
//                          t W + w, not at 64 w + t: the lanes of one request differ in w, so they fall on different banks
//                          whatever their bits t are (64 w + t would put every lane on bank t).  Neighbours are taken in
//                          trips of ROLES_FLIGHT: their rows of bits are requested together (each W words, coalesced), then
//                          each lane walks the set bits of its words and increments.  A lane ORs the words it has seen; at
//                          the row's end it walks only those bits for squares, reached, ksum and ksq, the selection, and to
//                          set the counters back to zero, so h is clean for the wave's next row.  Bounded by the dependent
//                          load per trip on short rows and by the LDS increments (one per membership of a neighbour) on
//                          long ones.
//
// The selection is `top` rounds of a wave-wide arg-max of (c, lowest k first) over the candidates that come after the
// previous winner (ammsb_postfit.h), so nothing is marked as taken.
//
// Rows go to the waves of a persistent grid in turn (wave g takes rows g, g + G, ...), so neighbouring rows, which a hub
// seldom follows, go to different waves.  A hub row is walked by its one wave.
//
// The mask is read through mask_word() of ammsb_postfit.h alone (bits past K cleared).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ammsb_roles.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int ROLES_FLIGHT = 4;  // neighbours whose rows of bits are requested before the first is counted
constexpr int ROLES_TRIPS = 2;   // rows a wave takes before another block is worth it
constexpr int W1_WAVES = 4;      // h is at most 16 KiB per wave (K <= 4096): 64 KiB per block
constexpr int W2_WAVES = 2;      // at most 32 KiB per wave (K <= 8192): 64 KiB per block

struct Args {
  const u64* mask;
  uint32_t rows, K, W;
  const u64* offsets;
  const uint32_t* targets;
  uint64_t first, n;  // the node range
  uint32_t among, top, min_count;
  uint32_t *degree, *own, *embedded, *reached;
  u64 *votes, *squares;
  int32_t* home;
  uint32_t *hcount, *hflags;
  u64 *ksum, *ksq, *kmembers, *counts;
};

template <int WPL, int WAVES>
__device__ __forceinline__ void nodes_body(const Args& a) {
  extern __shared__ uint32_t lds[];  // WAVES x 64 W counters, all zero between two rows
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6, W = a.W;
  uint32_t* h = lds + (size_t)wave * 64u * W;
  for (uint32_t s = lane; s < 64u * W; s += 64u) h[s] = 0;  // (the wave's own part: no barrier)
  const uint32_t floor_all = a.min_count > 1u ? a.min_count : 1u;
  const bool own_only = a.among == AMMSB_ROLES_OWN;
  const uint64_t stride = (uint64_t)gridDim.x * WAVES;
  u64 valid = 0, skipped = 0;  // of this wave's rows: wave-uniform
  for (uint64_t r = (uint64_t)blockIdx.x * WAVES + wave; r < a.n; r += stride) {
    const uint32_t node = (uint32_t)(a.first + r);  // (< rows: the entry point checked the range)
    u64 xa[WPL], seen[WPL];
    uint32_t own = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      xa[i] = mask_word(a, node, lane + 64u * i);
      seen[i] = 0;
      own += (uint32_t)__popcll(xa[i]);
    }
    const uint64_t beg = a.offsets[node], end = a.offsets[node + 1];
    uint32_t degree = 0, embedded = 0;  // wave-uniform
    u64 votes = 0;                      // the lane's share
    for (uint64_t p = beg; p < end; p += 64) {
      const uint64_t left = end - p;
      const uint32_t cnt = left < 64 ? (uint32_t)left : 64u;
      const uint32_t mine = lane < cnt ? a.targets[p + lane] : 0xFFFFFFFFu;  // 64 targets in one request
      for (uint32_t j0 = 0; j0 < cnt; j0 += ROLES_FLIGHT) {
        u64 y[ROLES_FLIGHT][WPL];
        bool ok[ROLES_FLIGHT];
#pragma unroll
        for (int f = 0; f < ROLES_FLIGHT; ++f) {  // the trip's rows of bits are on their way together
          const uint32_t j = j0 + f;              // (wave-uniform)
          const uint32_t b = (uint32_t)__builtin_amdgcn_readlane((int)mine, (int)(j & 63u));
          const bool exists = j < cnt;
          ok[f] = exists && b < a.rows;
          skipped += (u64)(exists && !ok[f]);
#pragma unroll
          for (int i = 0; i < WPL; ++i) y[f][i] = ok[f] ? mask_word(a, b, lane + 64u * i) : 0ull;
        }
#pragma unroll
        for (int f = 0; f < ROLES_FLIGHT; ++f) {
          if (!ok[f]) continue;  // (wave-uniform)
          ++degree;
          u64 shared = 0;
#pragma unroll
          for (int i = 0; i < WPL; ++i) {
            shared |= xa[i] & y[f][i];
            seen[i] |= y[f][i];
            votes += (u64)__popcll(y[f][i]);
            const uint32_t w = lane + 64u * i;
            for (u64 bits = y[f][i]; bits; bits &= bits - 1) ++h[(uint32_t)__builtin_ctzll(bits) * W + w];  // (bits != 0: w < W)
          }
          embedded += (uint32_t)(__ballot(shared != 0) != 0);
        }
      }
    }
    valid += degree;

    // the row's end: only the counters that were touched
    u64 squares = 0;
    uint32_t reached = 0;
#pragma unroll
    for (int i = 0; i < WPL; ++i) {
      const uint32_t w = lane + 64u * i;
      reached += (uint32_t)__popcll(seen[i]);
      for (u64 bits = seen[i]; bits; bits &= bits - 1) {
        const uint32_t t = (uint32_t)__builtin_ctzll(bits);
        const u64 c = h[t * W + w];
        squares += c * c;
        if ((xa[i] >> t) & 1ull) {  // a is in k = 64 w + t (< K: live_bits)
          atomicAdd(&a.ksum[64u * w + t], c);
          atomicAdd(&a.ksq[64u * w + t], c * c);
        }
      }
      for (u64 bits = xa[i]; bits; bits &= bits - 1) atomicAdd(&a.kmembers[64u * w + (uint32_t)__builtin_ctzll(bits)], 1ull);
    }
    own = (uint32_t)wave_sum_u64(own);
    reached = (uint32_t)wave_sum_u64(reached);
    votes = wave_sum_u64(votes);
    squares = wave_sum_u64(squares);
    if (lane == 0) {
      a.degree[node] = degree;
      a.own[node] = own;
      a.embedded[node] = embedded;
      a.reached[node] = reached;
      a.votes[node] = votes;
      a.squares[node] = squares;
    }

    if (a.top) {
      const uint32_t floor = own_only ? a.min_count : floor_all;
      int pbits = 0x7FFFFFFF;  // the previous winner: (count, community); every count (<= degree < 2^31) comes after this
      uint32_t pcol = 0, flags = 0, filled = 0;
      for (; filled < a.top; ++filled) {
        Best best = {-1, 0};
#pragma unroll
        for (int i = 0; i < WPL; ++i) {  // ascending k inside a lane: word l before word l + 64
          const uint32_t w = lane + 64u * i;
          for (u64 bits = own_only ? xa[i] : seen[i]; bits; bits &= bits - 1) {
            const uint32_t t = (uint32_t)__builtin_ctzll(bits);
            const uint32_t c = h[t * W + w];
            if (c >= floor) offer<false>(best, (int)c, 64u * w + t, pbits, pcol);
          }
        }
        const int wbits = wave_max_i32(best.bits);
        if (wbits < 0) break;  // no candidate is left (wave-uniform)
        const uint32_t k = winner_col(best, wbits);
        // is a in k?  the lane that holds word k >> 6 knows
        const uint32_t kw = k >> 6;
        const u64 word = WPL == 2 && kw >= 64u ? xa[WPL - 1] : xa[0];
        const bool member = lane == (kw & 63u) && ((word >> (k & 63u)) & 1ull);
        if (__ballot(member)) flags |= 1u << filled;
        if (lane == 0) {
          a.home[(uint64_t)node * a.top + filled] = (int32_t)k;
          a.hcount[(uint64_t)node * a.top + filled] = (uint32_t)wbits;
        }
        pbits = wbits;
        pcol = k;
      }
      if (lane == 0) {
        for (uint32_t j = filled; j < a.top; ++j) {
          a.home[(uint64_t)node * a.top + j] = -1;
          a.hcount[(uint64_t)node * a.top + j] = 0;
        }
        a.hflags[node] = flags;
      }
    }

#pragma unroll
    for (int i = 0; i < WPL; ++i)
      for (u64 bits = seen[i]; bits; bits &= bits - 1) h[(uint32_t)__builtin_ctzll(bits) * W + lane + 64u * i] = 0;
  }
  if (lane == 0) {
    if (valid) atomicAdd(&a.counts[0], valid);
    if (skipped) atomicAdd(&a.counts[1], skipped);
  }
}

// WPL words per lane: 1 while a row's words fit a wave (K <= 4096), 2 above
__global__ __launch_bounds__(64 * W1_WAVES) void roles_nodes_w1(Args a) { nodes_body<1, W1_WAVES>(a); }
__global__ __launch_bounds__(64 * W2_WAVES) void roles_nodes_w2(Args a) { nodes_body<2, W2_WAVES>(a); }


}  // namespace

extern "C" const char* ammsb_roles_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_roles_last_error(void) { return g_last_error; }

extern "C" int ammsb_roles_nodes(const uint64_t* mask, uint64_t num_rows, uint32_t num_cols, const uint64_t* offsets,
                                 const uint32_t* targets, uint64_t first_row, uint64_t n_rows, uint32_t among, uint32_t top,
                                 uint32_t min_count, uint32_t* degree, uint32_t* own, uint32_t* embedded, uint32_t* reached,
                                 uint64_t* votes, uint64_t* squares, int32_t* home, uint32_t* hcount, uint32_t* hflags,
                                 uint64_t* ksum, uint64_t* ksq, uint64_t* kmembers, uint64_t* counts, void* stream) {
  if (!mask) return fail(AMMSB_EINVAL, "mask is NULL");
  if (!offsets) return fail(AMMSB_EINVAL, "offsets is NULL");
  if (!targets) return fail(AMMSB_EINVAL, "targets is NULL");
  if (!degree || !own || !embedded || !reached) return fail(AMMSB_EINVAL, "degree, own, embedded or reached is NULL");
  if (!votes || !squares) return fail(AMMSB_EINVAL, "votes or squares is NULL");
  if (!ksum || !ksq || !kmembers) return fail(AMMSB_EINVAL, "ksum, ksq or kmembers is NULL");
  if (!counts) return fail(AMMSB_EINVAL, "counts is NULL");
  if (num_cols == 0 || num_cols > AMMSB_ROLES_MAX_COLS) return fail(AMMSB_EINVAL, "num_cols outside 1..8192");
  if (num_rows >> 32) return fail(AMMSB_EINVAL, "2^32 rows or more");
  if (first_row > num_rows || n_rows > num_rows - first_row) return fail(AMMSB_EINVAL, "first_row + n_rows is past num_rows");
  if (among != AMMSB_ROLES_ALL && among != AMMSB_ROLES_OWN) return fail(AMMSB_EINVAL, "among is neither ALL nor OWN");
  if (top > AMMSB_ROLES_MAX_TOP) return fail(AMMSB_EINVAL, "top above 16");
  if (top > 0 && (!home || !hcount || !hflags)) return fail(AMMSB_EINVAL, "top > 0 and home, hcount or hflags is NULL");
  if (misaligned(mask, 8) || misaligned(offsets, 8)) return fail(AMMSB_EINVAL, "mask or offsets is not 8-byte aligned");
  if (misaligned(targets, 4)) return fail(AMMSB_EINVAL, "targets is not 4-byte aligned");
  if (misaligned(degree, 4) || misaligned(own, 4) || misaligned(embedded, 4) || misaligned(reached, 4))
    return fail(AMMSB_EINVAL, "degree, own, embedded or reached is not 4-byte aligned");
  if (misaligned(votes, 8) || misaligned(squares, 8)) return fail(AMMSB_EINVAL, "votes or squares is not 8-byte aligned");
  if (misaligned(home, 4) || misaligned(hcount, 4) || misaligned(hflags, 4))
    return fail(AMMSB_EINVAL, "home, hcount or hflags is not 4-byte aligned");
  if (misaligned(ksum, 8) || misaligned(ksq, 8) || misaligned(kmembers, 8) || misaligned(counts, 8))
    return fail(AMMSB_EINVAL, "ksum, ksq, kmembers or counts is not 8-byte aligned");
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
  a.among = among;
  a.top = top;
  a.min_count = min_count;
  a.degree = degree;
  a.own = own;
  a.embedded = embedded;
  a.reached = reached;
  a.votes = reinterpret_cast<u64*>(votes);
  a.squares = reinterpret_cast<u64*>(squares);
  a.home = home;
  a.hcount = hcount;
  a.hflags = hflags;
  a.ksum = reinterpret_cast<u64*>(ksum);
  a.ksq = reinterpret_cast<u64*>(ksq);
  a.kmembers = reinterpret_cast<u64*>(kmembers);
  a.counts = reinterpret_cast<u64*>(counts);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t per_wave = (size_t)64 * a.W * sizeof(uint32_t);  // h: at most 16 KiB (w1) or 32 KiB (w2)
  if (num_cols <= AMMSB_ROLES_W1_MAX_COLS) {
    const dim3 grid(persistent_grid(n_rows, (uint64_t)W1_WAVES * ROLES_TRIPS));
    hipLaunchKernelGGL(roles_nodes_w1, grid, dim3(64 * W1_WAVES), W1_WAVES * per_wave, s, a);
    return launched("roles_nodes_w1");
  }
  const dim3 grid(persistent_grid(n_rows, (uint64_t)W2_WAVES * ROLES_TRIPS));
  hipLaunchKernelGGL(roles_nodes_w2, grid, dim3(64 * W2_WAVES), W2_WAVES * per_wave, s, a);
  return launched("roles_nodes_w2");
}
