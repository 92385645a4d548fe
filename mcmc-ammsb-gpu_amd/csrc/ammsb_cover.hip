// libammsb_cover.so (include/ammsb_cover.h): the best match of every ground-truth community among the detected ones and
// of every detected community among the ground-truth ones, membership being pi[a, k] >= thr.
//
// A segmented reduction over the concatenated member list, so that every wave reads the same number of rows of pi
// whatever the sizes of the communities, and no G x K matrix exists:
//   cover_fast / cover_generic   a wave of a persistent grid takes a unit of AMMSB_COVER_UNIT consecutive entries of
//                    `members`, finds the communities the unit spans from `offsets` and counts, per run of entries of
//                    one community, the hits of every column in W = ceil(K / 64) LDS words per lane that only that
//                    lane touches (slot j of lane l is word 64 j + l of the wave's region: no bank conflicts and
//                    nothing to synchronise).  At the end of a run a community that lies inside the unit is finished in
//                    place; one that crosses a unit boundary adds its non-zero counts and its valid entries into the
//                    workspace row of the unit it starts in.  At most one community starts in a unit and leaves it.
//   cover_finish     a wave per workspace row: the community that holds the unit's last entry, if it starts in the unit
//                    and ends past it, is finished from the row.
//   cover_unpack     the running best of every detected community into the two output arrays.
// Finishing a community g with t valid entries: every lane walks its slots; a non-zero overlap o with column k is
// offered to the lane's best by the rational compare o1 (t + d2) > o2 (t + d1) (columns ascend with the slot, so the
// lower column stays on equality) and to the running best of k, a packed (overlap << 32) | g word, by a compare-and-swap
// loop; a butterfly of the same compare over the wave gives the best match of g.  The compare of the reverse direction
// needs t of the community that holds the word: truth_size[g] is stored, and fenced, before g's first swap, and read
// with a device-scope load after the word that names g.  A maximum under a total order does not depend on arrival.
//
// Which column a slot stands for: cover_fast loads 16 bytes per lane, so slot j = 4 i + c of lane l is column
// 256 i + 4 l + c; cover_generic loads column 64 j + l.  The workspace rows use the layout of the form that wrote them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/ammsb_cover.h"
#include "ammsb_postfit.h"

namespace {

typedef unsigned long long u64;

constexpr int C_WAVES = 4;  // waves per block, a unit each
constexpr int C_BLOCK = 64 * C_WAVES;
constexpr uint32_t UNIT = AMMSB_COVER_UNIT;
constexpr int IDS = UNIT / 64;  // member ids a lane holds of its wave's unit
constexpr uint32_t NONE = 0xFFFFFFFFu;
constexpr uint32_t BLOCKS_PER_CU = 8;        // what MAX_GRID (ammsb_postfit.h) counts per CU
constexpr uint32_t LDS_PER_CU = 160u << 10;  // gfx950
static_assert(UNIT % 64 == 0, "a unit is whole registers of member ids");

struct CoverArgs {
  ammsb_rpm pi;
  float thr;
  uint32_t G, units, W;
  const u64* offsets;
  const uint32_t* members;
  u64 M;
  const u64* dsize;
  int32_t* tbest;
  uint32_t *tover, *tsize;
  u64* skipped;
  uint32_t* dense;
  u64* best;          // [K] (overlap << 32) | g, 0: none yet
  uint32_t* tcount;   // [units] valid entries of the community that starts in the unit and leaves it
  uint32_t* scratch;  // [units][64 W] its counts, in the slot layout of the counting form
  int fast;
};

// o1 / s1 > o2 / s2 for s1, s2 > 0, as o1 s2 > o2 s1 in 128 bits
__device__ __forceinline__ bool ratio_gt(uint32_t o1, u64 s1, uint32_t o2, u64 s2) {
  const u64 lh = __umul64hi((u64)o1, s2), ll = (u64)o1 * s2;
  const u64 rh = __umul64hi((u64)o2, s1), rl = (u64)o2 * s1;
  return lh > rh || (lh == rh && ll > rl);
}

// the community that holds entry p < M: the largest g with offsets[g] <= p
__device__ __forceinline__ uint32_t community_of(const CoverArgs& a, u64 p) {
  uint32_t lo = 0, hi = a.G;
  while (hi - lo > 1) {
    const uint32_t mid = lo + ((hi - lo) >> 1);
    if (a.offsets[mid] <= p) lo = mid;
    else hi = mid;
  }
  return lo;
}

// overlap o of community g (t valid entries) with column col of size d, offered to the running best of col
__device__ __forceinline__ void offer_detected(const CoverArgs& a, uint32_t col, uint32_t o, uint32_t g, uint32_t t, u64 d) {
  const u64 mine = ((u64)o << 32) | g;
  u64 cur = __hip_atomic_load(&a.best[col], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (;;) {
    const uint32_t co = (uint32_t)(cur >> 32), cg = (uint32_t)cur;
    if (co) {
      const u64 tc = __hip_atomic_load(&a.tsize[cg], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool better = ratio_gt(o, t + d, co, tc + d) || (!ratio_gt(co, tc + d, o, t + d) && g < cg);
      if (!better) return;
    }
    const u64 prev = atomicCAS(&a.best[col], cur, mine);
    if (prev == cur) return;
    cur = prev;
  }
}

// GET(j): the lane's count of slot j.  All 64 lanes are here.
template <class GET>
__device__ __forceinline__ void finish_community(const CoverArgs& a, uint32_t g, uint32_t t, bool fast, uint32_t lane,
                                                 GET get) {
  // t_g is visible before g can be found in a running best
  if (lane == 0) __hip_atomic_store(&a.tsize[g], t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __threadfence();
  const uint32_t K = (uint32_t)a.pi.num_cols;
  uint32_t bo = 0, bcol = NONE;
  u64 bs = 1;
  for (uint32_t j = 0; j < a.W; ++j) {
    const uint32_t o = get(j);
    if (o) {
      const uint32_t col = slot_col(fast, j, lane);
      if (col < K) {  // (a count can only be of a column)
        const u64 d = a.dsize[col], s = (u64)t + d;
        if (a.dense) a.dense[(u64)g * K + col] = o;
        if (ratio_gt(o, s, bo, bs)) {
          bo = o;
          bs = s;
          bcol = col;
        }
        offer_detected(a, col, o, g, t, d);
      }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const uint32_t oo = __shfl_xor(bo, off, 64), oc = __shfl_xor(bcol, off, 64);
    const u64 os = __shfl_xor(bs, off, 64);
    if (ratio_gt(oo, os, bo, bs) || (!ratio_gt(bo, bs, oo, os) && oc < bcol)) {
      bo = oo;
      bs = os;
      bcol = oc;
    }
  }
  if (lane == 0) {
    a.tbest[g] = bo ? (int32_t)bcol : -1;
    a.tover[g] = bo;
  }
}

// 16 slots of a row: slots 16 ch .. 16 ch + 15 of the lane; a slot past the row holds -1, below every threshold
template <bool FAST>
__device__ __forceinline__ void load_chunk(const float* p, uint32_t ch, uint32_t K, uint32_t lane, float (&x)[16]) {
  if (FAST) {
    const float4* q = reinterpret_cast<const float4*>(p) + ch * 256u + lane;
    const int nv = (int)(K >> 8) - 4 * (int)ch;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      float4 v = {-1.f, -1.f, -1.f, -1.f};
      if (i < nv) v = q[i * 64];
      x[4 * i] = v.x;
      x[4 * i + 1] = v.y;
      x[4 * i + 2] = v.z;
      x[4 * i + 3] = v.w;
    }
  } else {
#pragma unroll
    for (int t = 0; t < 16; ++t) {
      const uint32_t col = 64u * (16u * ch + t) + lane;
      x[t] = col < K ? p[col] : -1.0f;
    }
  }
}

template <bool FAST>
__device__ __forceinline__ void count_body(const CoverArgs& a, uint32_t* lds) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const uint32_t K = (uint32_t)a.pi.num_cols, W = a.W, nch = (W + 15u) >> 4;
  const uint32_t rows = (uint32_t)a.pi.num_rows;  // (0 rows: every member is invalid)
  uint32_t* cnt = lds + (size_t)wave * 64u * W + lane;
  for (uint32_t j = 0; j < W; ++j) cnt[j * 64u] = 0;
  u64 nskip = 0;
  for (uint32_t unit = blockIdx.x * C_WAVES + wave; unit < a.units; unit += gridDim.x * C_WAVES) {
    const u64 ustart = (u64)unit * UNIT;
    const uint32_t n = (uint32_t)(a.M - ustart < (u64)UNIT ? a.M - ustart : (u64)UNIT);
    uint32_t id[IDS];
#pragma unroll
    for (int r = 0; r < IDS; ++r) {
      const uint32_t at = 64u * r + lane;
      id[r] = at < n ? a.members[ustart + at] : NONE;
    }
    auto member = [&](uint32_t e) -> uint32_t {
      uint32_t v = NONE;
#pragma unroll
      for (int r = 0; r < IDS; ++r)
        if ((int)(e >> 6) == r) v = (uint32_t)__shfl((int)id[r], (int)(e & 63u), 64);
      return (uint32_t)__builtin_amdgcn_readfirstlane((int)v);
    };
    auto next_valid = [&](uint32_t e) -> uint32_t {
      while (e < n && member(e) >= rows) ++e;
      return e;
    };
    uint32_t g = community_of(a, ustart), e = 0, nv = next_valid(0);
    float x[16];
    if (nv < n) load_chunk<FAST>(postfit_row(a.pi, member(nv)), 0, K, lane, x);
    while (e < n) {
      const u64 gstart = a.offsets[g], gend = a.offsets[g + 1];
      uint32_t rend = gend < ustart + n ? (gend > ustart ? (uint32_t)(gend - ustart) : 0u) : n;
      if (rend <= e) rend = e + 1;  // (offsets that do not ascend: still one entry per trip, and never past the unit)
      uint32_t valid = 0;
      for (; e < rend; ++e) {
        if (e != nv) {  // an invalid member: nv is the next valid entry at or after e
          ++nskip;
          continue;
        }
        ++valid;
        const float* p = postfit_row(a.pi, member(e));
        nv = next_valid(e + 1);
        for (uint32_t ch = 0; ch < nch; ++ch) {
          uint32_t h[16];
#pragma unroll
          for (int t = 0; t < 16; ++t) h[t] = x[t] >= a.thr ? 1u : 0u;
          // the registers are free: the next chunk, or the next valid row's first, before these hits are added
          if (ch + 1 < nch) load_chunk<FAST>(p, ch + 1, K, lane, x);
          else if (nv < n) load_chunk<FAST>(postfit_row(a.pi, member(nv)), 0, K, lane, x);
#pragma unroll
          for (int t = 0; t < 16; ++t) {
            const uint32_t j = 16u * ch + t;
            if (j < W) atomicAdd(&cnt[j * 64u], h[t]);
          }
        }
      }
      auto take = [&](uint32_t j) -> uint32_t {
        const uint32_t o = cnt[j * 64u];
        cnt[j * 64u] = 0;
        return o;
      };
      if (gstart >= ustart && gend <= ustart + n) {
        finish_community(a, g, valid, FAST, lane, take);
      } else {
        const u64 sr = gstart / UNIT;  // the unit the community starts in
        if (sr < a.units) {
          uint32_t* row = a.scratch + sr * 64u * W + lane;
          for (uint32_t j = 0; j < W; ++j) {
            const uint32_t o = take(j);
            if (o) atomicAdd(&row[j * 64u], o);
          }
          if (lane == 0 && valid) atomicAdd(&a.tcount[sr], valid);
        } else {
          for (uint32_t j = 0; j < W; ++j) take(j);
        }
      }
      if (e < n) {  // the next community with an entry at or after e
        const u64 pos = ustart + e;
        do ++g;
        while (g + 1 < a.G && a.offsets[g + 1] <= pos);
        if (g >= a.G) g = a.G - 1;
      }
    }
  }
  if (lane == 0 && nskip) atomicAdd(a.skipped, nskip);
}

__global__ __launch_bounds__(C_BLOCK) void cover_fast(CoverArgs a) {
  extern __shared__ uint32_t lds[];
  count_body<true>(a, lds);
}

__global__ __launch_bounds__(C_BLOCK) void cover_generic(CoverArgs a) {
  extern __shared__ uint32_t lds[];
  count_body<false>(a, lds);
}

__global__ __launch_bounds__(C_BLOCK) void cover_finish(CoverArgs a) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  // the last unit has no boundary after it
  for (uint32_t u = blockIdx.x * C_WAVES + wave; u + 1 < a.units; u += gridDim.x * C_WAVES) {
    const u64 ustart = (u64)u * UNIT, uend = ustart + UNIT;
    const uint32_t g = community_of(a, uend - 1);
    if (a.offsets[g] < ustart || a.offsets[g + 1] <= uend) continue;
    const uint32_t* row = a.scratch + (u64)u * 64u * a.W + lane;
    finish_community(a, g, a.tcount[u], a.fast != 0, lane, [&](uint32_t j) -> uint32_t { return row[j * 64u]; });
  }
}

__global__ __launch_bounds__(C_BLOCK) void cover_unpack(const u64* best, uint32_t K, int32_t* dbest, uint32_t* dover) {
  const uint32_t k = blockIdx.x * C_BLOCK + threadIdx.x;
  if (k >= K) return;
  const u64 w = best[k];
  dbest[k] = (w >> 32) ? (int32_t)(uint32_t)w : -1;
  dover[k] = (uint32_t)(w >> 32);
}

bool shape_ok(uint64_t num_members, uint64_t num_cols) {
  return num_cols >= 1 && num_cols <= AMMSB_COVER_MAX_COLS && !(num_members >> 32);
}

uint64_t units_of(uint64_t num_members) { return (num_members + UNIT - 1) / UNIT; }
uint64_t words_of(uint64_t num_cols) { return (num_cols + 63) / 64; }

}  // namespace

extern "C" const char* ammsb_cover_last_kernel_name(void) { return g_last_kernel; }
extern "C" const char* ammsb_cover_last_error(void) { return g_last_error; }

extern "C" uint64_t ammsb_cover_workspace_bytes(uint64_t num_members, uint32_t num_cols) {
  if (!shape_ok(num_members, num_cols) || num_members == 0) return 0;
  const uint64_t U = units_of(num_members);
  return 8ull * num_cols + 8ull * ((U + 1) / 2) + 256ull * U * words_of(num_cols);
}

extern "C" int ammsb_cover_match(const ammsb_rpm* pi, float thr, const uint64_t* offsets, uint64_t num_truth,
                                 const uint32_t* members, uint64_t num_members, const uint64_t* detected_size,
                                 int32_t* truth_best, uint32_t* truth_overlap, uint32_t* truth_size,
                                 int32_t* detected_best, uint32_t* detected_overlap, uint64_t* skipped,
                                 uint32_t* overlap, void* workspace, uint64_t workspace_bytes, void* stream) {
  if (!pi) return fail(AMMSB_EINVAL, "pi is NULL");
  if (!detected_size) return fail(AMMSB_EINVAL, "detected_size is NULL");
  if (!detected_best || !detected_overlap || !skipped) return fail(AMMSB_EINVAL, "an output is NULL");
  if (num_truth > 0 && !offsets) return fail(AMMSB_EINVAL, "offsets is NULL");
  if (num_truth > 0 && (!truth_best || !truth_overlap || !truth_size)) return fail(AMMSB_EINVAL, "an output is NULL");
  if (num_members > 0 && !members) return fail(AMMSB_EINVAL, "members is NULL");
  if (!(thr >= 0.0f && thr < INFINITY)) return fail(AMMSB_EINVAL, "thr negative, NaN or infinite");
  bool aligned;
  if (const char* bad = check_rpm(pi, AMMSB_COVER_MAX_COLS, &aligned)) return fail(AMMSB_EINVAL, bad);
  if (num_truth >> 31) return fail(AMMSB_EINVAL, "2^31 communities or more");
  if (num_members >> 32) return fail(AMMSB_EINVAL, "2^32 members or more");
  if (num_truth == 0 || num_members == 0) return AMMSB_OK;
  const uint32_t K = (uint32_t)pi->num_cols;
  const uint64_t need = ammsb_cover_workspace_bytes(num_members, K);
  if (!workspace || workspace_bytes < need) return fail(AMMSB_EINVAL, "the workspace is NULL or too small");
  if (reinterpret_cast<uintptr_t>(workspace) & 7) return fail(AMMSB_EINVAL, "the workspace is not 8-byte aligned");

  const uint64_t U = units_of(num_members), W = words_of(K);
  CoverArgs a;
  a.pi = *pi;
  a.thr = thr;
  a.G = (uint32_t)num_truth;
  a.units = (uint32_t)U;
  a.W = (uint32_t)W;
  a.offsets = reinterpret_cast<const u64*>(offsets);
  a.members = members;
  a.M = num_members;
  a.dsize = reinterpret_cast<const u64*>(detected_size);
  a.tbest = truth_best;
  a.tover = truth_overlap;
  a.tsize = truth_size;
  a.skipped = reinterpret_cast<u64*>(skipped);
  a.dense = overlap;
  a.best = static_cast<u64*>(workspace);
  a.tcount = reinterpret_cast<uint32_t*>(a.best + K);
  a.scratch = a.tcount + 2 * ((U + 1) / 2);
  a.fast = (K % 256 == 0 && aligned) ? 1 : 0;

  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if ((e = hipMemsetAsync(workspace, 0, need, s)) != hipSuccess) return hip_fail("cover: memset", e);
  if ((e = hipMemsetAsync(truth_best, 0xFF, 4 * num_truth, s)) != hipSuccess) return hip_fail("cover: memset", e);
  if ((e = hipMemsetAsync(truth_overlap, 0, 4 * num_truth, s)) != hipSuccess) return hip_fail("cover: memset", e);
  if ((e = hipMemsetAsync(truth_size, 0, 4 * num_truth, s)) != hipSuccess) return hip_fail("cover: memset", e);
  if ((e = hipMemsetAsync(skipped, 0, 8, s)) != hipSuccess) return hip_fail("cover: memset", e);
  if (overlap && (e = hipMemsetAsync(overlap, 0, 4 * num_truth * K, s)) != hipSuccess)
    return hip_fail("cover: memset", e);

  // a block's LDS is one region of 64 W words per wave; past residency a block would only queue
  const size_t lds = (size_t)C_WAVES * 64 * W * sizeof(uint32_t);
  uint32_t per_cu = LDS_PER_CU / (uint32_t)lds;
  per_cu = per_cu > BLOCKS_PER_CU ? BLOCKS_PER_CU : per_cu;
  per_cu = per_cu < 1 ? 1 : per_cu;
  const unsigned cap = MAX_GRID / BLOCKS_PER_CU * per_cu, want = persistent_grid(U, C_WAVES);
  const dim3 grid(want < cap ? want : cap), block(C_BLOCK);
  const char* name;
  if (a.fast) {
    name = "cover_fast";
    // per call, not once per process: the attribute belongs to the current device
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cover_fast), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds)) != hipSuccess)
      return hip_fail(name, e);
    hipLaunchKernelGGL(cover_fast, grid, block, lds, s, a);
  } else {
    name = "cover_generic";
    // per call, not once per process: the attribute belongs to the current device
    if ((e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cover_generic), hipFuncAttributeMaxDynamicSharedMemorySize,
                                 (int)lds)) != hipSuccess)
      return hip_fail(name, e);
    hipLaunchKernelGGL(cover_generic, grid, block, lds, s, a);
  }
  if (const int rc = launched(name)) return rc;
  if (U > 1) {
    hipLaunchKernelGGL(cover_finish, dim3(persistent_grid(U - 1, C_WAVES)), block, 0, s, a);
    if (const int rc = launched("cover_finish")) return rc;
  }
  hipLaunchKernelGGL(cover_unpack, dim3((K + C_BLOCK - 1) / C_BLOCK), block, 0, s, a.best, K, detected_best,
                     detected_overlap);
  if (const int rc = launched("cover_unpack")) return rc;
  g_last_kernel = name;
  return AMMSB_OK;
}
