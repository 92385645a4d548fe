"""Child process of test_gpu_relate.py (one per group): the community relations (include/ammsb_relate.h,
ops.CommunityRelations, Learner.CommunityOverlap / RelatedCommunities) against the numpy statement of the header's
definitions:

    M = pi >= np.float32(thr);  overlap = M.T.astype(np.float64) @ M.astype(np.float64)      (exact: every count < 2^32)
    bits of rows [lo, hi) = np.packbits(M[lo:hi].T, axis=1, bitorder="little") as little-endian 64-bit words
    partners of k = the l != k with overlap[k, l] >= max(1, min_overlap), sorted by (-Fraction(o, den), l)

Only integer adds and integer compares are involved on both sides, so everything must be equal: there is no tolerance
anywhere below."""
import io
import os
import sys
from fractions import Fraction

import numpy as np

import postfit_support as ps

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SEEN = set()
F32 = np.float32
MEASURES = ("overlap", "jaccard", "contained")


def members(pi, thr):
    return pi >= F32(thr)


def overlap_of(M):
    return (M.T.astype(np.float64) @ M.astype(np.float64)).astype(np.int64)


def words_of(M, lo, hi):
    """-> [K, ceil((hi - lo) / 64)] uint64: the statement's bits of rows lo .. hi - 1"""
    n, K = hi - lo, M.shape[1]
    W = (n + 63) // 64
    padded = np.zeros((K, W * 64), dtype=bool)
    padded[:, :n] = M[lo:hi].T
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(K, W)


def ranking(ov, by):
    """-> per community (l [c], o [c]): the l != k with o = overlap[k, l] >= 1 in the order of the measure.  The order of
    the values is that of their fractions.Fraction (one per distinct (o, den) of the row; equal fractions share a rank),
    equal values go to the lower l"""
    K, d = ov.shape[0], np.diagonal(ov)
    assert int(ov.max(initial=0)) < 2 ** 29
    out = []
    for k in range(K):
        ls = np.flatnonzero(ov[k] > 0)
        ls = ls[ls != k]
        o = ov[k, ls]
        den = np.ones_like(o) if by == "overlap" else d[k] + d[ls] - o if by == "jaccard" else d[ls]
        keys, inverse = np.unique(o * (1 << 33) + den, return_inverse=True)
        fracs = [Fraction(int(key) >> 33, int(key) & ((1 << 33) - 1)) for key in keys.tolist()]
        rank_of = {f: i for i, f in enumerate(sorted(set(fracs), reverse=True))}
        rank = np.array([rank_of[f] for f in fracs], dtype=np.int64)[inverse.reshape(-1)] if ls.size else np.zeros(0, np.int64)
        order = np.lexsort((ls, rank))
        out.append((ls[order], o[order]))
    return out


def selection(rank, top, min_overlap):
    """-> (partner [K, top] int32, shared [K, top] uint32) from ranking(): a filter keeps the order"""
    K = len(rank)
    partner, shared = np.full((K, top), -1, dtype=np.int32), np.zeros((K, top), dtype=np.uint32)
    for k, (ls, o) in enumerate(rank):
        keep = np.flatnonzero(o >= max(1, min_overlap))[:top]
        partner[k, :keep.size], shared[k, :keep.size] = ls[keep], o[keep]
    return partner, shared


def cuttings(N):
    c1, c2 = (N // 3) // 64 * 64, (2 * N // 3) // 64 * 64
    ragged = [(a, b) for a, b in ((0, c1), (c1, c2), (c2, N)) if b > a]
    return {"whole": [(0, N)], "slabs of 64": [(lo, min(lo + 64, N)) for lo in range(0, N, 64)], "ragged": ragged}


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _relate
        super().__init__()
        self.rl = _relate
        self.lib = _relate.load()
        self.api = self.ops.CommunityRelations(self.ctx)
        self.readout = self.ops.CommunityReadout(self.ctx)

    def overlap(self, pi, M, thr, cuts, what):
        """the bits and pair calls over guarded buffers of this test's own, slab by slab; every slab's words are
        compared with the statement's -> overlap [K, K] int64"""
        import ctypes as C
        T = self.torch
        K = int(pi.cols)
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        ov = self.guarded(K * K, T.int32, FILL32, zero=True)
        for lo, hi in cuts:
            W = (hi - lo + 63) // 64
            assert int(self.lib.ammsb_relate_bits_bytes(hi - lo, K)) == K * W * 8
            bits = self.guarded(K * W, T.int64, FILL64)
            self.rl.check(self.lib.ammsb_relate_bits(C.byref(pi.desc), float(F32(thr)), lo, hi - lo, ptr(bits), None))
            SEEN.add(self.rl.last_kernel_name())
            self.rl.check(self.lib.ammsb_relate_pairs(ptr(bits), K, hi - lo, ptr(ov), None))
            SEEN.add(self.rl.last_kernel_name())
            got = bits.cpu().numpy().view(np.uint64)
            assert (got[K * W:] == FILL64).all(), "%s: the words past bits were written" % what
            want = words_of(M, lo, hi)
            assert np.array_equal(got[:K * W].reshape(K, W), want), "%s: the bit words of rows %d..%d differ" % (what, lo, hi)
        got = ov.cpu().numpy().view(np.uint32)
        assert (got[K * K:] == FILL32).all(), "%s: the words past overlap were written" % what
        return got[:K * K].reshape(K, K).astype(np.int64)

    def top(self, d_ov, by, top, min_overlap, what):
        """the selection call over guarded outputs, d_ov [K, K] on the device -> (partner [K, top] int32, shared [K, top]
        uint32)"""
        import ctypes as C
        T = self.torch
        K = int(d_ov.shape[0])
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        partner, shared = self.guarded(K * top, T.int32, FILL32), self.guarded(K * top, T.int32, FILL32)
        self.rl.check(self.lib.ammsb_relate_top(ptr(d_ov), K, self.rl.MEASURES[by], top, min_overlap, ptr(partner),
                                                ptr(shared), None))
        SEEN.add(self.rl.last_kernel_name())
        p, s = partner.cpu().numpy(), shared.cpu().numpy().view(np.uint32)
        assert (p[K * top:].view(np.uint32) == FILL32).all() and (s[K * top:] == FILL32).all(), \
            "%s: the words past partner or shared were written" % what
        return p[:K * top].reshape(K, top).copy(), s[:K * top].reshape(K, top).copy()

    def everything(self, host, thr, what, select=True):
        """every cutting against the statement, bit-equal to each other and to a second call; the diagonal against the
        read-out's sizes; the partners against the host selection"""
        pi = self.matrix(host)
        M = members(host, thr)
        want = overlap_of(M)
        first = None
        for name, cuts in cuttings(host.shape[0]).items():
            got = self.overlap(pi, M, thr, cuts, "%s cut=%s" % (what, name))
            assert np.array_equal(got, want), "%s cut=%s: overlap differs from M.T @ M" % (what, name)
            if first is None:
                first = got
                assert np.array_equal(first, self.overlap(pi, M, thr, cuts, what)), what + ": two calls differ"
            else:
                assert np.array_equal(first, got), "%s: cut=%s differs from one slab" % (what, name)
        assert np.array_equal(first, first.T), what + ": not symmetric"
        sizes = self.readout.sizes(pi, float(F32(thr))).cpu().numpy()
        assert np.array_equal(np.diagonal(first), sizes), what + ": the diagonal is not CommunitySizes"
        if select:
            d_ov = self.ctx.from_numpy(first.astype(np.uint32))
            for by in MEASURES:
                rank = ranking(want, by)
                for top in (1, 4, 64):
                    for min_overlap in (1, 3):
                        p, s = self.top(d_ov, by, top, min_overlap, what)
                        wp, ws = selection(rank, top, min_overlap)
                        tag = "%s by=%s top=%d min_overlap=%d" % (what, by, top, min_overlap)
                        assert np.array_equal(p, wp), tag + ": partners differ"
                        assert np.array_equal(s, ws), tag + ": shared differs"
                        if (top, min_overlap) == (4, 1):
                            again = self.top(d_ov, by, top, min_overlap, what)
                            assert np.array_equal(p, again[0]) and np.array_equal(s, again[1]), tag + ": two calls differ"
        return first


def random_pi(rng, N, K, thr, plant=True):
    """about K^-1/2 of the entries at or above thr; NaNs and values equal to thr planted; column 0 holds every node and
    column K - 1 none (K >= 3)"""
    host = (rng.random((N, K)) * 0.9 * thr).astype(F32)
    above = rng.random((N, K)) < K ** -0.5
    host[above] = (thr + rng.random(int(above.sum())) * (1 - thr)).astype(F32)
    flat = host.reshape(-1)
    spots = rng.choice(flat.size, min(flat.size, max(2, flat.size // 50)), replace=False)
    flat[spots[::2]] = np.nan
    flat[spots[1::2]] = F32(thr)
    if plant and K >= 3:
        host[:, 0] = F32(0.5)
        host[:, K - 1] = F32(0.5) * F32(thr)
    return host


# (N, K): every N of {1, 63, 64, 65, 127, 129, 1000, 4100}, every K of {1, 2, 31, 33, 64, 65, 127, 129, 260, 1024}, and
# K = 8192 at N = 300
EXACT = ((1, 1), (63, 2), (64, 31), (65, 33), (127, 64), (129, 1024), (1000, 65), (4100, 260), (1000, 127), (4100, 129),
         (300, 8192))


def exact_group(which):
    b = Bench()
    rng = np.random.default_rng(11)
    for i, (N, K) in enumerate(EXACT):
        if which and i not in which:
            continue
        thr = 0.05
        host = random_pi(rng, N, K, thr)
        got = b.everything(host, thr, "N=%d K=%d" % (N, K))
        print("exact N=%d K=%d: %d pairs of communities overlap, largest community %d" % (
            N, K, int(((got > 0).sum() - (np.diagonal(got) > 0).sum()) // 2), int(np.diagonal(got).max())), flush=True)
    if not which or 0 in which:
        # thr = 0 (every stored number but a NaN is a member) and thr above every value
        host = random_pi(rng, 130, 65, 0.05)
        got = b.everything(host, 0.0, "thr=0")
        assert got[0, 0] == 130 and got.max() == 130 and (np.diagonal(got) == (~np.isnan(host)).sum(0)).all()
        got = b.everything(host, 2.0, "thr above every value")
        assert not got.any()
        # pi in two and in three blocks whose rows_in_block is no multiple of 64: a 64-row group straddles two blocks
        for K in (1024, 65):
            host = random_pi(rng, 300, K, 0.05)
            M = members(host, 0.05)
            want = overlap_of(M)
            for rib in (151, 101):
                pi = b.matrix(host, rib)
                assert len(pi.blocks) == (2 if rib == 151 else 3)
                for name, cuts in cuttings(300).items():
                    got = b.overlap(pi, M, 0.05, cuts, "K=%d rows_in_block=%d cut=%s" % (K, rib, name))
                    assert np.array_equal(got, want), (K, rib, name)
        print("exact thr=0, thr=2, blocks ok", flush=True)
    print("exact ok", flush=True)


def depth_group():
    """The pair pass cuts the node words into depth slices so that tiles x slices reaches PAIR_ITEMS = 1024, a slice
    being whole chunks of CHUNK = 16 32-bit words (512 nodes), and runs min(items, PAIR_GRID = 512) blocks.
      K = 64, N = 307163: one tile, 600 chunks -> 600 slices of one chunk: 600 items for 512 blocks.
      K = 260, N = 100000: 6 tiles, 196 chunks, depth ceil(1024 / 6) = 171 -> 98 slices of two chunks: 588 items, the
      last slice of every tile ragged (N is no multiple of 64 either)."""
    b = Bench()
    rng = np.random.default_rng(21)
    for N, K in ((307163, 64), (100000, 260)):
        host = rng.random((N, K), dtype=F32)
        host[rng.integers(0, N, 1000), rng.integers(0, K, 1000)] = np.nan
        thr = 0.9
        M = members(host, thr)
        pi = b.matrix(host)
        got = b.overlap(pi, M, thr, [(0, N)], "depth N=%d K=%d" % (N, K))
        assert np.array_equal(got, overlap_of(M)), "depth N=%d K=%d: overlap differs from M.T @ M" % (N, K)
        half = N // 2 // 64 * 64
        assert np.array_equal(got, b.overlap(pi, M, thr, [(0, half), (half, N)], "depth, two slabs"))
        print("depth N=%d K=%d ok" % (N, K), flush=True)
    print("depth ok", flush=True)


def forms_group():
    """every kernel form is named and reached, on both sides of its dispatch boundary, and a misaligned pi takes the
    generic form and writes the same words"""
    b = Bench()
    rng = np.random.default_rng(9)
    T = b.torch
    for K, form in ((256, "relate_bits_fast"), (255, "relate_bits_generic"), (257, "relate_bits_generic"),
                    (512, "relate_bits_fast"), (8192, "relate_bits_fast"), (260, "relate_bits_generic")):
        N = 200
        host = random_pi(rng, N, K, 0.05)
        M = members(host, 0.05)
        pi = b.matrix(host)
        bits = b.api.bits(pi, 0.05)
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == form, (K, b.api.kernel_name())
        assert np.array_equal(bits.cpu().numpy().view(np.uint64), words_of(M, 0, N)), K
        part = b.api.bits(pi, 0.05, rows=(64, 171))
        assert np.array_equal(part.cpu().numpy().view(np.uint64), words_of(M, 64, 171)), K
        ov = b.ctx.zeros((K, K), T.int32)
        b.api.pairs(bits, K, N, ov)
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == "relate_pairs"
        want = overlap_of(M)
        assert np.array_equal(ov.cpu().numpy().view(np.uint32).astype(np.int64), want), K
        partner, shared = b.api.top(ov, "jaccard", 4, 1)
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == "relate_top"
        wp, ws = selection(ranking(want, "jaccard"), 4, 1)
        assert np.array_equal(partner.cpu().numpy(), wp) and np.array_equal(shared.cpu().numpy().view(np.uint32), ws), K
        if K % 256 == 0:
            mis = b.misaligned(host)
            mbits = b.api.bits(mis, 0.05)
            SEEN.add(b.api.kernel_name())
            assert b.api.kernel_name() == "relate_bits_generic"
            assert T.equal(bits, mbits), "K=%d: the two forms write other words" % K
    assert SEEN == set(b.rl.KERNEL_FORMS), SEEN ^ set(b.rl.KERNEL_FORMS)
    print("forms ok", flush=True)


def sparse_overlap(M):
    """-> (cells k K + l ascending, counts): the non-zero entries of M.T @ M, counted row by row from the members of a row"""
    K = M.shape[1]
    sets = [np.flatnonzero(row).astype(np.int64) for row in M]
    flat = np.concatenate([np.add.outer(s * K, s).reshape(-1) for s in sets])
    cells, counts = np.unique(flat, return_counts=True)
    return cells, counts.astype(np.int64)


def dense_of(K, cells, counts):
    out = np.zeros(K * K, np.int64)
    out[cells] = counts
    return out.reshape(K, K)


def big_group():
    """pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, zero but 640 planted rows
    in four windows): the bits of all rows and of the slab that starts 128 rows before element 2^32, in the 16-byte form
    and, from a base 4 bytes past a 16-byte boundary, in the generic form; overlap and partners of the full bits.  The
    statement is evaluated over the 640 rows; every word of the other rows must be 0.  relate_pairs and relate_top read
    no pi: they are checked here on what the bits gave them, not reached past 2^32 themselves."""
    b = Bench()
    T = b.torch
    n, K = ps.BIG_ROWS, ps.BIG_K
    slab = ((1 << 19) - 128, n)
    pi, compact, ids = b.big_pi(61)
    thr = ps.big_threshold(compact)
    M, Mw = members(compact, thr), members(ps.big_wrapped(compact), thr)
    assert np.array_equal(ids & 63, np.arange(640) & 63)     # a window begins and ends on a word of 64 rows
    cols = np.unique(ids >> 6)
    want, wrapped = words_of(M, 0, 640), words_of(Mw, 0, 640)
    tail = want[:, -4:].copy()                               # the slab's words
    cells, counts = sparse_overlap(M)
    wcells, wcounts = sparse_overlap(Mw)
    ov = dense_of(K, cells, counts)
    wp, ws = selection(ranking(ov, "jaccard"), 4, 1)
    # a kernel that keeps row * K in 32 bits would give the wrapped figures: each of them differs from the true ones
    assert M.sum() >= 40 * 640 and cols.size == 10 == want.shape[1]
    assert not np.array_equal(want, wrapped) and not np.array_equal(tail, wrapped[:, -4:])
    assert not (np.array_equal(cells, wcells) and np.array_equal(counts, wcounts))
    wov = dense_of(K, wcells, wcounts)
    assert not np.array_equal(np.diagonal(ov), np.diagonal(wov))
    wwp, wws = selection(ranking(wov, "jaccard"), 4, 1)
    assert not np.array_equal(wp, wwp) and not np.array_equal(ws, wws)
    del wov
    print("big: the wrapped-offset reference differs in the words, the slab's words, overlap, its diagonal, partners "
          "and shared", flush=True)
    d_cols = b.ctx.from_numpy(cols)

    def bits_of(pi, form):
        full = b.api.bits(pi, thr)
        assert b.api.kernel_name() == form, b.api.kernel_name()
        assert tuple(full.shape) == (K, n // 64)
        got = full[:, d_cols].cpu().numpy().view(np.uint64)
        assert np.array_equal(got, want), "%s: the words of the planted rows differ" % form
        rest = full.clone()
        rest[:, d_cols] = 0
        assert int(T.count_nonzero(rest)) == 0, "%s: a word of an unplanted row is set" % form
        del rest
        part = b.api.bits(pi, thr, rows=slab)
        assert b.api.kernel_name() == form, b.api.kernel_name()
        assert tuple(part.shape) == (K, 4)
        assert np.array_equal(part.cpu().numpy().view(np.uint64), tail), "%s: the words of the slab differ" % form
        return full, part

    full, part = bits_of(pi, "relate_bits_fast")
    d_ov = b.ctx.zeros((K, K), T.int32)
    b.api.pairs(full, K, n, d_ov)
    assert b.api.kernel_name() == "relate_pairs"
    d_want = b.ctx.zeros((K * K,), T.int32)
    d_want[b.ctx.from_numpy(cells)] = b.ctx.from_numpy(counts.astype(np.int32))
    assert T.equal(d_ov.view(-1), d_want), "overlap differs from M.T @ M over the planted rows"
    assert np.array_equal(d_ov.diagonal().cpu().numpy().astype(np.int64), M.sum(0)), "the diagonal is not the column sums"
    partner, shared = b.api.top(d_ov, "jaccard", 4, 1)
    assert b.api.kernel_name() == "relate_top"
    assert np.array_equal(partner.cpu().numpy(), wp), "partners differ"
    assert np.array_equal(shared.cpu().numpy().view(np.uint32), ws), "shared differs"
    del pi, d_ov, d_want
    b.release()
    mis, again, _ = b.big_pi(61, misaligned=True)
    assert np.array_equal(again, compact)
    mfull, mpart = bits_of(mis, "relate_bits_generic")
    assert T.equal(full, mfull) and T.equal(part, mpart), "the two forms write other words"
    print("big ok: %d x %d, thr %.3g, %d memberships, %d overlapping pairs" % (n, K, thr, int(M.sum()), cells.size), flush=True)


def planted_group():
    from mcmc_ammsb_gpu_amd import _relate
    b = Bench()
    rng = np.random.default_rng(5)
    T = b.torch

    def related(host, thr, by, top=4, min_overlap=1):
        pi = b.matrix(host)
        K, N = host.shape[1], host.shape[0]
        ov = b.ctx.zeros((K, K), T.int32)
        b.api.pairs(b.api.bits(pi, thr), K, N, ov)
        partner, shared = b.api.top(ov, by, top, min_overlap)
        m = ov.cpu().numpy().view(np.uint32)
        return _relate.Related(thr, by, min_overlap, np.diagonal(m).astype(np.int64), partner.cpu().numpy(),
                               shared.cpu().numpy().view(np.uint32), m, N=N)

    # columns 0 and 1 identical; column 2 a strict subset of column 3; columns 4 and 5 disjoint from everything
    N = 200
    host = np.zeros((N, 6), F32)
    same = rng.choice(190, 70, replace=False)
    host[same, 0] = host[same, 1] = 0.7
    big = rng.choice(190, 90, replace=False)
    host[big, 3] = 0.3
    host[big[:31], 2] = 0.9
    host[190:195, 4] = 1.0
    host[195:200, 5] = 1.0
    for by in MEASURES:
        r = related(host, 0.25, by)
        ov = r.matrix.astype(np.int64)
        assert r.size.tolist() == [70, 70, 31, 90, 5, 5], r.size
        assert r.partner[0, 0] == 1 and r.partner[1, 0] == 0    # (1 is the largest value of all three, ties by id)
        i01, i10 = r.partner[0].tolist().index(1), r.partner[1].tolist().index(0)
        assert r.jaccard[0, i01] == 1.0 and r.jaccard[1, i10] == 1.0 and r.overlap[0, i01] == 70
        assert (0, 1) in r.duplicates() and (2, 3) not in r.duplicates()
        i23, i32 = r.partner[2].tolist().index(3), r.partner[3].tolist().index(2)
        assert r.inside[2, i23] == 1.0 and r.contained[3, i32] == 1.0 and r.jaccard[2, i23] == 31 / 90
        assert r.inside[3, i32] == 31 / 90 and (3, 2) in r.nested() and (2, 3) not in r.nested()
        assert (r.partner[4:] == -1).all() and (r.overlap[4:] == 0).all() and not ov[4:, :4].any()
        wp, ws = selection(ranking(ov, by), 4, 1)
        assert np.array_equal(r.partner, wp) and np.array_equal(r.overlap, ws), by
    # ties go to the lower id: community 0 shares 3 of its 6 nodes with 1 and the other 3 with 2, which are disjoint
    host = np.zeros((12, 4), F32)
    host[0:6, 0] = host[[0, 1, 2, 6, 7, 8], 1] = host[[3, 4, 5, 9, 10, 11], 2] = 1.0
    for by in MEASURES:
        r = related(host, 0.5, by, top=3)
        assert r.partner.tolist() == [[1, 2, -1], [0, -1, -1], [0, -1, -1], [-1, -1, -1]], (by, r.partner)
        assert r.overlap.tolist() == [[3, 3, 0], [3, 0, 0], [3, 0, 0], [0, 0, 0]], by
        assert r.jaccard[0].tolist() == [3 / 9, 3 / 9, 0.0] and r.contained[0].tolist() == [0.5, 0.5, 0.0]
    # min_overlap above every overlap: no partner at all
    r = related(host, 0.5, "overlap", top=2, min_overlap=4)
    assert (r.partner == -1).all() and (r.overlap == 0).all()
    print("planted ok", flush=True)


def _check_related(r, host, thr, by, top, min_overlap, what):
    want = overlap_of(members(host, thr))
    assert np.array_equal(r.size, np.diagonal(want)), what + ": sizes"
    wp, ws = selection(ranking(want, by), top, min_overlap)
    assert np.array_equal(r.partner, wp), what + ": partners differ"
    assert np.array_equal(r.overlap, ws), what + ": shared differs"
    return want


def learner_group(graph):
    import torch
    from mcmc_ammsb_gpu_amd import _relate
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    for thr in (0.05, 0.01):
        ov = lrn.CommunityOverlap(thr)
        assert ov.dtype == torch.int32 and tuple(ov.shape) == (K, K)
        want = overlap_of(members(host, thr))
        assert np.array_equal(ov.cpu().numpy().view(np.uint32).astype(np.int64), want), "CommunityOverlap thr=%g" % thr
        assert np.array_equal(np.diagonal(want), lrn.CommunitySizes(thr).cpu().numpy())
        # 1000 bytes hold the bits of 192 rows at K = 32: 53 slabs; 1 byte: slabs of 64 rows
        for max_bytes in (1000, 1):
            assert torch.equal(ov, lrn.CommunityOverlap(thr, max_bytes=max_bytes)), (thr, max_bytes)
        for by, top, min_overlap in (("jaccard", 4, 1), ("overlap", 1, 3), ("contained", 31, 1), ("jaccard", 64, 0)):
            r = lrn.RelatedCommunities(thr, top, by, min_overlap, dense=True)
            assert isinstance(r, _relate.Related) and r.top == top and r.N == N
            _check_related(r, host, thr, by, top, min_overlap, "learner thr=%g by=%s top=%d" % (thr, by, top))
            assert np.array_equal(r.matrix.astype(np.int64), want)
            cut = lrn.RelatedCommunities(thr, top, by, min_overlap, max_bytes=1000)
            assert cut.matrix is None and np.array_equal(cut.partner, r.partner) and np.array_equal(cut.overlap, r.overlap)
            assert np.array_equal(cut.size, r.size)
        print("thr=%g: %d of %d community pairs overlap" % (thr, int((np.triu(want, 1) > 0).sum()), K * (K - 1) // 2), flush=True)
    ps.rejects(AmmsbError, (lambda: lrn.CommunityOverlap(-1.0), lambda: lrn.RelatedCommunities(top=65), lambda: lrn.RelatedCommunities(by="cosine"),
                            lambda: lrn.CommunityOverlap(max_bytes=0)))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CommunityOverlap(0.05, max_bytes=1000)
        a.RelatedCommunities()
    ps.unperturbed_run(make, calls, "community relations")
    print("learner ok graph=%s" % graph, flush=True)


def _check_related_file(path, ckpt, K, thr, by, top, what):
    """a related-communities file against the statement over the pi of the checkpoint the same process wrote; the
    Python writer reproduces its bytes"""
    from mcmc_ammsb_gpu_amd import _relate
    fN, r = _relate.read_related(path)
    assert r.size.size == K and F32(r.threshold) == F32(thr) and (r.by, r.top, r.min_overlap) == (by, top, 1), what
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    _check_related(r, pi, thr, by, top, 1, what)
    again = path + ".py"
    _relate.write_related(again, fN, r)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the Python writer's bytes differ" % what
    return fN, r


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("relate_test", d, 240)
        fN, res = _check_related_file(os.path.join(d, "related.txt"), os.path.join(d, "cpp.ckpt"), 64, 0.05, "jaccard", 4,
                                      "relate_test")
        assert fN == 20000
        print("cpp ok: Learner::WriteRelatedCommunities equals the statement over the checkpoint's pi", flush=True)
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck = os.path.join(d, "r.txt"), os.path.join(d, "main.ckpt")
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--checkpoint-out", ck]
        for extra, thr, by, top in (([], 0.05, "jaccard", 4),
                                    (["--related-communities-threshold", "0.02", "--related-communities-top", "64",
                                      "--related-communities-by", "contained"], 0.02, "contained", 64),
                                    (["--related-communities-by", "overlap", "--related-communities-top", "1"], 0.05, "overlap", 1)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--related-communities-out", out] + extra, 240)
            fN, res = _check_related_file(out, ck, 48, thr, by, top, "ammsb_main by=%s" % by)
            assert fN == N
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "depth": lambda a: depth_group(),
    "forms": lambda a: forms_group(),
    "planted": lambda a: planted_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
