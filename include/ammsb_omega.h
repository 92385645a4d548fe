/* libammsb_omega.so: the Omega index (Collins & Dent) of the detected cover against a known one -- the agreement of the
 * two covers on how many communities every pair of nodes shares, corrected for chance.  It is a pass over node pairs
 * and not over (community, community) pairs, so it takes a universe of nodes from the start.
 *
 * Definitions (the contract):
 *   universe         U: n distinct node ids < N, ascending.  Positions i < j of U form the P = n (n - 1) / 2 unordered
 *                    pairs.  Every array below with n rows is indexed by position.
 *   detected cover   D(a) = {k : pi[a, k] >= thr}: a binary32 compare of the stored value, so a NaN is never a member
 *                    (ammsb_quality.h's definition).
 *   ground truth     T(a) = {g : a in members_g}, from the CSR the cover match takes: offsets[G + 1] u64 (non-decreasing,
 *                    offsets[0] == 0, offsets[G] == M), members[M] u32 node ids.  A member >= N is counted in `skipped`,
 *                    a valid member that is not in U in `outside`; neither sets a bit.  A node listed twice inside one
 *                    community sets its bit once here; the Python and C++ layers refuse such a ground truth, as they do
 *                    for the NMI.  offsets lives on the device: for offsets that do not ascend from 0 to M every walk is
 *                    still bounded by M and G, but the results are unspecified.
 *   per pair         sD = |D(a) & D(b)|,  sT = |T(a) & T(b)|.
 *   per level        for j = 0 .. L - 1:  detected[j] = the pairs with sD == j,  truth[j] = the pairs with sT == j,
 *                    agree[j] = the pairs with sD == sT == j.  A pair with sD >= L or sT >= L is counted only in
 *                    `clipped`.  The layers above choose L = 1 + max(max |D(a)|, max |T(a)|) over U, which makes clipped
 *                    0, and raise if it is not.  L <= AMMSB_OMEGA_MAX_LEVELS.
 *   hist             [3 L + 1] u64: agree[0 .. L), detected[L .. 2 L), truth[2 L .. 3 L), clipped.
 *   the score        Sa = sum agree[j],  Se = sum detected[j] truth[j]:
 *                        omega = (Sa P - Se) / (P^2 - Se)      [ = (w_u - w_e) / (1 - w_e), w_u = Sa / P, w_e = Se / P^2 ]
 *                    Numerator and denominator are exact integers (Python int, signed __int128 in C++) and their
 *                    quotient is rounded to binary64 once, to nearest even (Python's int / int; an integer long division
 *                    in C++): it is the value of the exact fraction, and _omega.py and mcmc::Learner::CoverOmega print
 *                    the same bytes.  (Converting each to binary64 first and dividing then rounds three times and misses
 *                    that value by a unit in the last place in ordinary cases.)  omega = NaN when n < 2 or P^2 == Se.
 *                    NaN and not the -1 that the other scores of this project use for "undefined":
 *                    the Omega index can itself be negative.
 *                    omega_unadjusted = Sa / P (NaN when n < 2).
 * In numpy: MD = pi[U] >= np.float32(thr); SD = MD.astype(np.int32) @ MD.T.astype(np.int32), ST likewise from the truth;
 * iu = np.triu_indices(n, 1); the bincounts of SD[iu], ST[iu] and SD[iu][SD[iu] == ST[iu]].  Integer adds only: every
 * count is exact, the same from run to run, and does not depend on how the tile range is cut into launches.
 *
 * Bit rows.  Both covers become one bit per (position, community): rows of ceil(K / 32) and ceil(G / 32) u32 words.  Which
 * bit of a row stands for which community is a function of the row length (K or G) alone and otherwise private to this
 * library -- the pair pass only ANDs two rows of one matrix and counts -- and a bit that stands for no community is 0.
 *
 * The pair pass.  The n x n position square is cut into tiles of AMMSB_OMEGA_TILE x AMMSB_OMEGA_TILE; with
 * R = ceil(n / AMMSB_OMEGA_TILE) the R (R + 1) / 2 tiles of the upper triangle, diagonal included, are numbered row by
 * row: tile row r holds numbers r R - r (r - 1) / 2 .. + (R - r - 1).  ammsb_omega_pairs takes a range of them, so that
 * one long pass can be several short launches.
 *
 * A library, a header and a signature table of their own: include/ammsb.h and libammsb_hip.so are unchanged; ammsb_rpm
 * is taken by pointer (copied before return) and no ammsb_ctx is needed.  A call only enqueues kernels on `stream` (a
 * hipStream_t as void*, NULL = the null stream): no allocation, no synchronisation.  Return values are the codes of
 * ammsb.h.  AMMSB_EINVAL, before anything is launched and before any device pointer is used, is listed per call. */
#ifndef AMMSB_OMEGA_H_
#define AMMSB_OMEGA_H_

#include <stdint.h>

#include "ammsb.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AMMSB_OMEGA_MAX_COLS 8192u
#define AMMSB_OMEGA_MAX_TRUTH 65536u
#define AMMSB_OMEGA_MAX_LEVELS 4096u
#define AMMSB_OMEGA_TILE 128u
/* most tiles of one launch: the block-private counters are 32-bit */
#define AMMSB_OMEGA_MAX_LAUNCH_TILES (1ull << 26)

/* bits[n, ceil(K / 32)] and counts[n] = |D(U[i])| from pi.  nodes[n] u32 on the device; NULL means the identity, rows
 * 0 .. n - 1 of pi.  A node id >= num_rows reads nothing and gives an empty row.  n == 0 launches nothing.
 * EINVAL: a NULL pi, bits or counts; thr negative, NaN or infinite; num_cols == 0 or > 8192; num_rows >= 2^32; a
 * descriptor whose blocks do not cover num_rows; n >= 2^31; nodes == NULL and n > num_rows. */
int ammsb_omega_detected_bits(const ammsb_rpm* pi, float thr, const uint32_t* nodes, uint64_t n, uint32_t* bits,
                              uint32_t* counts, void* stream);

/* bits[n, ceil(G / 32)] (zeroed by the caller; ORed into) and counts[n] = |T(U[i])| (written, from a second pass over
 * the finished rows: a duplicate member cannot inflate them); *skipped and *outside are added to.  position[N] i32 on the
 * device: the position of a node in U, or -1.  n == 0 or G == 0 launches nothing.
 * EINVAL: G > 65536; N >= 2^32; n >= 2^31; M >= 2^32; with n > 0 and G > 0 a NULL offsets, position, bits, counts,
 * skipped or outside; with M > 0 a NULL members. */
int ammsb_omega_truth_bits(const uint64_t* offsets, uint64_t num_truth, const uint32_t* members, uint64_t num_members,
                           uint64_t num_nodes, const int32_t* position, uint64_t n, uint32_t* bits, uint32_t* counts,
                           uint64_t* skipped, uint64_t* outside, void* stream);

/* Adds the pairs of tiles tile_begin .. tile_begin + tile_count - 1 to hist[3 L + 1].  detected_bits[n, ceil(K / 32)]
 * and truth_bits[n, ceil(G / 32)] as the two calls above write them (truth_bits is not read when G == 0).  n == 0 or
 * tile_count == 0 launches nothing.
 * EINVAL: a NULL hist; with n > 0 and tile_count > 0 a NULL detected_bits, or a NULL truth_bits with G > 0; num_cols == 0
 * or > 8192; G > 65536; L == 0 or > 4096 (3 L block-private 32-bit counters have to fit the LDS of a compute unit
 * beside the tile); n >= 2^31; a tile range that ends past the triangle; tile_count > AMMSB_OMEGA_MAX_LAUNCH_TILES. */
int ammsb_omega_pairs(const uint32_t* detected_bits, uint32_t num_cols, const uint32_t* truth_bits, uint64_t num_truth,
                      uint64_t n, uint32_t num_levels, uint64_t tile_begin, uint64_t tile_count, uint64_t* hist,
                      void* stream);

/* Name of the kernel form the calling thread's last successful call took ("" before the first):
 *   omega_bits_fast      K a multiple of 256 and 16-byte aligned blocks: a wave per row of U, 16-byte loads, a compare
 *                        and a ballot per register slot.
 *   omega_bits_generic   every other 1 <= K <= 8192, and misaligned blocks: scalar loads; the same words.
 *   omega_truth_scatter  a wave per ground-truth community: one vector atomic OR per member that is in U.
 *   omega_truth_count    a wave per row: the population count of the finished row (what ammsb_omega_truth_bits reports:
 *                        it runs last).
 *   omega_pairs          a persistent grid over the tile range; a block of 256 lanes owns a tile, streams 16-word
 *                        chunks of both row sets through LDS and every lane keeps an 8 x 8 micro-tile of counters in
 *                        registers: AND + population count over the detected rows, then over the truth rows, then the
 *                        compare.  The pair (0, 0) is counted in a register; every other pair goes into 3 L
 *                        block-private LDS counters that are flushed with 64-bit vector atomics. */
const char* ammsb_omega_last_kernel_name(void);
/* Text of the calling thread's last failure ("" if none). */
const char* ammsb_omega_last_error(void);

#ifdef __cplusplus
}
#endif
#endif  /* AMMSB_OMEGA_H_ */
