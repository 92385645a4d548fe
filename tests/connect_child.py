"""Child process of test_gpu_connect.py (one per group): the community links (include/ammsb_connect.h, ops.CommunityLinks,
Learner.CommunityLinks / LinkedCommunities) against the numpy statement of the header's definitions:

    M = pi >= np.float32(thr);  a, b = keys >> 32, keys & 0xFFFFFFFF over the keys with both ends < N
    C = M[a].T.astype(np.float64) @ M[b].astype(np.float64);  links = C + C.T                  (exact below 2^53)
    mask words of node a = np.packbits(M[a], bitorder="little") as little-endian 64-bit words
    partners of k = the l != k with links[k, l] >= max(1, min_links), sorted by (-Fraction(w, den), l), den = 1 or
                    d_k d_l - overlap[k, l] (a pair with den == 0 left out), overlap = M.T @ M

Only integer adds and integer compares are involved on both sides, so everything must be equal: there is no tolerance
anywhere below.  At a large K the product above is taken edge by edge over the index sets of the two rows (the same sum,
term by term); statement() does both where both are affordable and asserts that they agree."""
import io
import os
import sys
from fractions import Fraction

import numpy as np

import postfit_support as ps

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SEEN = set()
F32 = np.float32
MEASURES = ("links", "density")
# the kernels' constants (csrc/ammsb_connect.hip)
C_WAVES, MAX_GRID, RUN_CHUNK, RUNS_GRID = 4, 2048, 128, 1024


def members(pi, thr):
    return pi >= F32(thr)


def overlap_of(M):
    return (M.T.astype(np.float64) @ M.astype(np.float64)).astype(np.int64)


def words_of(M):
    """-> [N, ceil(K / 64)] uint64: the statement's mask"""
    N, K = M.shape
    W = (K + 63) // 64
    padded = np.zeros((N, W * 64), dtype=bool)
    padded[:, :K] = M
    return np.packbits(padded, axis=1, bitorder="little").view("<u8").reshape(N, W)


def ends_of(keys, N):
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N)
    return a[ok], b[ok], int(ok.sum()), int((~ok).sum())


def statement(M, keys):
    """-> (cells [c] int64 ascending, counts [c] int64, valid, skipped): the non-zero cells k K + l of directed"""
    N, K = M.shape
    a, b, valid, skipped = ends_of(keys, N)
    sets = [np.flatnonzero(row).astype(np.int64) for row in M]
    parts = [np.add.outer(sets[u] * K, sets[v]).reshape(-1) for u, v in zip(a.tolist(), b.tolist())]
    flat = np.concatenate(parts) if parts else np.zeros(0, np.int64)
    cells, counts = np.unique(flat, return_counts=True)
    if K <= 1024 and a.size * K <= 1 << 24:   # the statement as the header writes it
        C = np.zeros((K, K))
        for lo in range(0, a.size, 1 << 15):
            C += M[a[lo:lo + (1 << 15)]].T.astype(np.float64) @ M[b[lo:lo + (1 << 15)]].astype(np.float64)
        dense = np.zeros(K * K, np.int64)
        dense[cells] = counts
        assert np.array_equal(dense.reshape(K, K), C.astype(np.int64)), "the two forms of the statement differ"
    return cells, counts.astype(np.int64), valid, skipped


def ranking(links, ov, by):
    """-> per community (l [c], w [c], o [c]): the l != k with w = links[k, l] >= 1 (and, by density, pairs > 0) in the
    order of the measure.  The order of the values is that of their fractions.Fraction (one per distinct (w, den) of the
    row), equal values go to the lower l"""
    K, d = links.shape[0], np.diagonal(ov)
    assert int(links.max(initial=0)) < 2 ** 30 and int(d.max(initial=0)) < 2 ** 16
    out = []
    for k in range(K):
        ls = np.flatnonzero(links[k] > 0)
        ls = ls[ls != k]
        w, o = links[k, ls], ov[k, ls]
        den = np.ones_like(w) if by == "links" else d[k] * d[ls] - o
        keep = den > 0
        ls, w, o, den = ls[keep], w[keep], o[keep], den[keep]
        keys, inverse = np.unique(w * (1 << 33) + den, return_inverse=True)
        fracs = [Fraction(int(key) >> 33, int(key) & ((1 << 33) - 1)) for key in keys.tolist()]
        rank_of = {f: i for i, f in enumerate(sorted(set(fracs), reverse=True))}
        rank = np.array([rank_of[f] for f in fracs], dtype=np.int64)[inverse.reshape(-1)] if ls.size else np.zeros(0, np.int64)
        order = np.lexsort((ls, rank))
        out.append((ls[order], w[order], o[order]))
    return out


def selection(rank, top, min_links):
    """-> (partner [K, top] int32, links [K, top] uint64, shared [K, top] uint32) from ranking(): a filter keeps the order"""
    K = len(rank)
    partner, plinks = np.full((K, top), -1, dtype=np.int32), np.zeros((K, top), dtype=np.uint64)
    shared = np.zeros((K, top), dtype=np.uint32)
    for k, (ls, w, o) in enumerate(rank):
        keep = np.flatnonzero(w >= max(1, min_links))[:top]
        partner[k, :keep.size], plinks[k, :keep.size], shared[k, :keep.size] = ls[keep], w[keep], o[keep]
    return partner, plinks, shared


def edge_list(rng, N, n):
    """n keys over N nodes, both orders of the ends: about a twentieth each self loops, repeats of earlier keys, and keys
    with an end >= N (N itself, a little past it, 2^32 - 1)"""
    a, b = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    loops = rng.random(n) < 0.05
    b[loops] = a[loops]
    bad = rng.random(n) < 0.05
    past = rng.choice(np.array([N, N + 5, 2 ** 32 - 1], dtype=np.uint64), n)
    side = rng.random(n) < 0.5
    a[bad & side] = past[bad & side]
    b[bad & ~side] = past[bad & ~side]
    keys = (a << np.uint64(32)) | b
    for i in np.flatnonzero(rng.random(n) < 0.05):
        if i:
            keys[i] = keys[rng.integers(0, i)]
    return keys


def force(form):
    if form is None:
        os.environ.pop("AMMSB_CONNECT_FORM", None)
    else:
        os.environ["AMMSB_CONNECT_FORM"] = form


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _connect
        super().__init__()
        self.cn = _connect
        self.lib = _connect.load()
        self.api = self.ops.CommunityLinks(self.ctx)
        self.quality = self.ops.CommunityQuality(self.ctx)

    def mask(self, pi, M, what):
        """the mask call over a guarded buffer, compared with the statement's words -> the [N, W] device tensor"""
        import ctypes as C
        T = self.torch
        N, K = M.shape
        W = (K + 63) // 64
        assert int(self.lib.ammsb_connect_mask_bytes(N, K)) == N * W * 8
        buf = self.guarded(N * W, T.int64, FILL64)
        self.cn.check(self.lib.ammsb_connect_mask(C.byref(pi.desc), float(F32(self.thr)), C.c_void_p(buf.data_ptr()), None))
        SEEN.add(self.cn.last_kernel_name())
        got = buf.cpu().numpy().view(np.uint64)
        assert (got[N * W:] == FILL64).all(), what + ": the words past the mask were written"
        assert np.array_equal(got[:N * W].reshape(N, W), words_of(M)), what + ": the mask words differ"
        return buf[:N * W].reshape(N, W)

    def directed(self, mask, N, K, cuts, what):
        """the edge call over guarded buffers, the list in the pieces `cuts` -> (directed [K * K] int64 on the device,
        counts [2] on the host)"""
        import ctypes as C
        T = self.torch
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        d, cnt = self.guarded(K * K, T.int64, FILL64, zero=True), self.guarded(2, T.int64, FILL64, zero=True)
        for keys in cuts:
            dev = self.ctx.from_numpy(keys) if keys.size else None
            self.cn.check(self.lib.ammsb_connect_edges(ptr(mask), N, K, ptr(dev) if keys.size else None, keys.size, ptr(d),
                                                       ptr(cnt), None))
            if keys.size:
                SEEN.add(self.cn.last_kernel_name())
        assert bool((d[K * K:] == FILL64).all()) and bool((cnt[2:] == FILL64).all()), what + ": the words past directed or counts were written"
        return d[:K * K], cnt[:2].cpu().numpy()

    def finish(self, d, K, what):
        import ctypes as C
        T = self.torch
        links = self.guarded(K * K, T.int64, FILL64)
        self.cn.check(self.lib.ammsb_connect_finish(C.c_void_p(d.data_ptr()), K, C.c_void_p(links.data_ptr()), None))
        SEEN.add(self.cn.last_kernel_name())
        assert bool((links[K * K:] == FILL64).all()), what + ": the words past links were written"
        return links[:K * K]

    def top(self, d_links, d_ov, by, top, min_links, what):
        import ctypes as C
        T = self.torch
        K = int(d_ov.shape[0])
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        partner, shared = self.guarded(K * top, T.int32, FILL32), self.guarded(K * top, T.int32, FILL32)
        plinks = self.guarded(K * top, T.int64, FILL64)
        self.cn.check(self.lib.ammsb_connect_top(ptr(d_links), ptr(d_ov), K, self.cn.MEASURES[by], top, min_links,
                                                 ptr(partner), ptr(plinks), ptr(shared), None))
        SEEN.add(self.cn.last_kernel_name())
        p, w, s = partner.cpu().numpy(), plinks.cpu().numpy().view(np.uint64), shared.cpu().numpy().view(np.uint32)
        assert (p[K * top:].view(np.uint32) == FILL32).all() and (s[K * top:] == FILL32).all() and \
            (w[K * top:] == FILL64).all(), what + ": the words past partner, links or shared were written"
        return tuple(x[:K * top].reshape(K, top).copy() for x in (p, w, s))

    def want_dev(self, K, cells, counts):
        ref = self.ctx.zeros((K * K,), self.torch.int64)
        if cells.size:
            ref[self.ctx.from_numpy(cells)] = self.ctx.from_numpy(counts)
        return ref

    def everything(self, host, thr, what, pi=None, sizes=(0, 1, 257, 3000), select=True, seed=3):
        """mask, edges (every list sorted and shuffled, every form the shape has), finish and top against the statement"""
        T = self.torch
        self.thr = thr
        N, K = host.shape
        pi = self.matrix(host) if pi is None else pi
        M = members(host, thr)
        mask = self.mask(pi, M, what)
        rng = np.random.default_rng(seed)
        forms = ("d", "r") if K <= self.cn.RUNS_MAX_COLS else ("d",)
        last = None
        for n in sizes:
            base = edge_list(rng, N, n)
            for order, keys in (("sorted", np.sort(base)), ("shuffled", rng.permutation(base))):
                tag = "%s n=%d %s" % (what, n, order)
                cells, counts, valid, skipped = statement(M, keys)
                want = self.want_dev(K, cells, counts)
                for form in forms:
                    force(form)
                    d, cnt = self.directed(mask, N, K, [keys], tag)
                    if n:
                        assert self.cn.last_kernel_name() == {"d": "connect_edges_direct", "r": "connect_edges_runs"}[form]
                    assert T.equal(d, want), "%s form=%s: directed differs from M[a].T @ M[b]" % (tag, form)
                    assert cnt.tolist() == [valid, skipped], "%s form=%s: counts %s, not %s" % (tag, form, cnt, (valid, skipped))
                    if n >= 257:
                        again, cnt2 = self.directed(mask, N, K, [keys], tag)
                        assert T.equal(d, again) and cnt2.tolist() == cnt.tolist(), tag + ": two calls differ"
                        c1, c2 = n // 3 - 7, 2 * n // 3 + 5
                        cut, cnt3 = self.directed(mask, N, K, [keys[:c1], keys[c1:c2], keys[c2:]], tag)
                        assert T.equal(d, cut) and cnt3.tolist() == cnt.tolist(), tag + ": three ragged calls differ from one"
                force(None)
                links = self.finish(d, K, tag)
                wl = want.view(K, K) + want.view(K, K).t()
                assert T.equal(links.view(K, K), wl), tag + ": links differs from C + C.T"
                assert T.equal(links.view(K, K), links.view(K, K).t()), tag + ": links is not symmetric"
                q = self.quality.edges(self.quality.mask(pi, float(F32(thr))), N, K, keys) if n else T.zeros(2 * K + 2, dtype=T.int64, device=links.device)
                assert T.equal(links.view(K, K).diagonal(), 2 * q[:K]), tag + ": the diagonal is not 2 internal"
                if n:
                    assert int(q[2 * K + 1]) == skipped
                last = (links, keys)
        if select and last is not None:
            d_links = last[0].contiguous()
            hl = d_links.cpu().numpy().reshape(K, K)
            ov = overlap_of(M)
            d_ov = self.ctx.from_numpy(ov.astype(np.uint32).view(np.int32)).reshape(K, K).contiguous()
            for by in MEASURES:
                rank = ranking(hl, ov, by)
                for top in (1, 4, 64):
                    for min_links in (1, 3):
                        p, w, s = self.top(d_links, d_ov, by, top, min_links, what)
                        wp, ww, ws = selection(rank, top, min_links)
                        tag = "%s by=%s top=%d min_links=%d" % (what, by, top, min_links)
                        assert np.array_equal(p, wp), tag + ": partners differ"
                        assert np.array_equal(w, ww), tag + ": links differ"
                        assert np.array_equal(s, ws), tag + ": shared differs"
                        if (top, min_links) == (4, 1):
                            again = self.top(d_links, d_ov, by, top, min_links, what)
                            assert all(np.array_equal(x, y) for x, y in zip((p, w, s), again)), tag + ": two calls differ"
        return last


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


# (N, K): every N of {1, 2, 65, 1000}, every K of {1, 2, 63, 64, 65, 129, 260, 1024}, and K = 4100, 8192 at N = 300
EXACT = ((1, 1), (2, 2), (65, 63), (1000, 64), (1, 65), (2, 129), (65, 260), (1000, 1024), (65, 1024), (1000, 65), (1000, 129),
         (300, 4100), (300, 8192))


def exact_group(which):
    b = Bench()
    rng = np.random.default_rng(11)
    for i, (N, K) in enumerate(EXACT):
        host = random_pi(rng, N, K, 0.05)
        if which and i not in which:
            continue
        links, _ = b.everything(host, 0.05, "N=%d K=%d" % (N, K), seed=100 + i)
        print("exact N=%d K=%d: %d pairs of communities linked" % (N, K, int((links.view(K, K).triu(1) > 0).sum())), flush=True)
    if not which or 0 in which:
        # thr = 0 (every stored number but a NaN is a member; K <= 65: the cost is quadratic) and thr above every value
        host = random_pi(rng, 130, 65, 0.05)
        links, keys = b.everything(host, 0.0, "thr=0")
        a, bb, valid, _ = ends_of(keys, 130)
        assert int(links.view(65, 65)[0, 0]) == 2 * valid
        links, _ = b.everything(host, 2.0, "thr above every value")
        assert not bool(links.any())
        # pi in two and in three blocks whose rows_in_block is no multiple of 64
        for K in (1024, 65):
            host = random_pi(rng, 300, K, 0.05)
            for rib in (151, 101):
                pi = b.matrix(host, rib)
                assert len(pi.blocks) == (2 if rib == 151 else 3)
                b.everything(host, 0.05, "K=%d rows_in_block=%d" % (K, rib), pi=pi, sizes=(257,), select=False)
        print("exact thr=0, thr=2, blocks ok", flush=True)
    print("exact ok", flush=True)


def forms_group():
    """every kernel form is named and reached, on both sides of its dispatch boundary; direct and runs forced on the same
    inputs give equal matrices; a misaligned pi takes the generic mask form and writes the same words; an unknown
    AMMSB_CONNECT_FORM is refused"""
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    b = Bench()
    rng = np.random.default_rng(9)
    T = b.torch
    for K, mform in ((256, "connect_mask_fast"), (255, "connect_mask_generic"), (257, "connect_mask_generic"),
                     (512, "connect_mask_fast"), (4096, "connect_mask_fast"), (4097, "connect_mask_generic"),
                     (8192, "connect_mask_fast"), (260, "connect_mask_generic")):
        N = 200
        host = random_pi(rng, N, K, 0.05)
        M = members(host, 0.05)
        pi = b.matrix(host)
        force(None)
        mask = b.api.mask(pi, 0.05)
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == mform, (K, b.api.kernel_name())
        assert np.array_equal(mask.cpu().numpy().view(np.uint64), words_of(M)), K
        keys = np.sort(edge_list(rng, N, 500))
        cells, counts, valid, skipped = statement(M, keys)
        want = b.want_dev(K, cells, counts)
        got = {}
        runs = "connect_edges_runs" if K <= 4096 else "connect_edges_direct"   # (the default where it exists)
        for form, name in ((None, runs), ("d", "connect_edges_direct"), ("r", runs)):
            force(form)
            d, cnt = b.api.edges(mask, N, K, keys)
            SEEN.add(b.api.kernel_name())
            assert b.api.kernel_name() == name, (K, form, b.api.kernel_name())
            assert T.equal(d.view(-1), want) and cnt.tolist() == [valid, skipped], (K, form)
            got[form] = d
        assert T.equal(got["d"], got["r"]) and T.equal(got["d"], got[None]), "K=%d: the forms give other matrices" % K
        force("x")
        caught = ps.rejects(AmmsbError, (lambda: b.api.edges(mask, N, K, keys),))
        assert "AMMSB_CONNECT_FORM" in str(caught[0])
        force(None)
        links = b.api.finish(got["d"])
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == "connect_finish"
        ov = overlap_of(M)
        d_ov = b.ctx.from_numpy(ov.astype(np.uint32).view(np.int32)).reshape(K, K).contiguous()
        partner, plinks, pshared = b.api.top(links, d_ov, "density", 4, 1)
        SEEN.add(b.api.kernel_name())
        assert b.api.kernel_name() == "connect_top"
        wp, ww, ws = selection(ranking(links.cpu().numpy(), ov, "density"), 4, 1)
        assert np.array_equal(partner.cpu().numpy(), wp) and np.array_equal(plinks.cpu().numpy().view(np.uint64), ww) and \
            np.array_equal(pshared.cpu().numpy().view(np.uint32), ws), K
        if K % 256 == 0:
            mis = b.misaligned(host)
            mmask = b.api.mask(mis, 0.05)
            SEEN.add(b.api.kernel_name())
            assert b.api.kernel_name() == "connect_mask_generic"
            assert T.equal(mask, mmask), "K=%d: the two mask forms write other words" % K
    assert SEEN == set(b.cn.KERNEL_FORMS), SEEN ^ set(b.cn.KERNEL_FORMS)
    print("forms ok", flush=True)


def depth_group():
    """connect_edges_direct takes a wave per edge over at most MAX_GRID blocks of C_WAVES waves: more than 8192 edges go
    round its loop.  connect_edges_runs takes a wave per chunk of RUN_CHUNK edges over at most RUNS_GRID blocks: more than
    RUNS_GRID C_WAVES RUN_CHUNK = 524288 edges go round its loop.  One run longer than a chunk (a hub with 3 RUN_CHUNK
    + 11 links) and runs that straddle chunk boundaries (every node with 37 links: 128 is no multiple of 37)."""
    b = Bench()
    rng = np.random.default_rng(21)
    T = b.torch
    N, K = 3000, 96
    host = random_pi(rng, N, K, 0.05)
    M = members(host, 0.05)
    b.thr = 0.05
    mask = b.mask(b.matrix(host), M, "depth")
    one_pass = RUNS_GRID * C_WAVES * RUN_CHUNK
    assert one_pass > MAX_GRID * C_WAVES
    n = one_pass + 3 * RUN_CHUNK + 1001
    src = np.repeat(np.arange(N, dtype=np.uint64), 37)
    hub = np.full(3 * RUN_CHUNK + 11, 1234, dtype=np.uint64)
    src = np.sort(np.concatenate([src, hub, rng.integers(0, N, n - src.size - hub.size).astype(np.uint64)]))
    keys = (src << np.uint64(32)) | rng.integers(0, N, n).astype(np.uint64)
    keys[::1000] |= np.uint64(0xFFFFFFFF)    # some keys with an end >= N in between
    a, bb, valid, skipped = ends_of(keys, N)
    C = np.zeros((K, K))
    for lo in range(0, a.size, 1 << 16):
        C += M[a[lo:lo + (1 << 16)]].T.astype(np.float64) @ M[bb[lo:lo + (1 << 16)]].astype(np.float64)
    want = b.ctx.from_numpy(C.astype(np.int64).reshape(-1))
    got = {}
    for form in ("d", "r"):
        force(form)
        d, cnt = b.directed(mask, N, K, [keys], "depth form=%s" % form)
        assert T.equal(d, want) and cnt.tolist() == [valid, skipped], "depth form=%s: directed or counts differ" % form
        cut, cnt = b.directed(mask, N, K, [keys[:100001], keys[100001:]], "depth form=%s, two calls" % form)
        assert T.equal(cut, want) and cnt.tolist() == [valid, skipped]
        got[form] = d
        print("depth form=%s ok: %d edges" % (form, n), flush=True)
    force(None)
    assert T.equal(got["d"], got["r"])
    print("depth ok", flush=True)


def sparse_overlap(M):
    """-> [K, K] int64: M.T @ M counted row by row from the members of a row"""
    K = M.shape[1]
    sets = [np.flatnonzero(row).astype(np.int64) for row in M]
    cells, counts = np.unique(np.concatenate([np.add.outer(s * K, s).reshape(-1) for s in sets]), return_counts=True)
    out = np.zeros(K * K, np.int64)
    out[cells] = counts
    return out.reshape(K, K)


def big_reference(compact, thr, keys):
    """the statement over the planted rows and the zero rows of postfit_support's big fixture, the keys remapped to them
    -> dict(M, words, cells, counts, valid, skipped, links, overlap, top)"""
    M = members(ps.big_extended(compact), thr)
    K = M.shape[1]
    cells, counts, valid, skipped = statement(M, ps.big_remap(keys))
    C = np.zeros(K * K, np.int64)
    C[cells] = counts
    links = C.reshape(K, K) + C.reshape(K, K).T
    ov = sparse_overlap(M)
    return dict(M=M, words=words_of(M), cells=cells, counts=counts, valid=valid, skipped=skipped, links=links, overlap=ov,
                top=selection(ranking(links, ov, "density"), 4, 1))


def big_group():
    """pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, zero but 640 planted rows
    in four windows): the mask of all rows in the 16-byte form and, from a base 4 bytes past a 16-byte boundary, in the
    generic form; then edges, finish and top over keys between every two windows, with loops, repeats, ends >= N and ends
    in zero rows.  The statement is evaluated over the planted rows with the keys remapped; the mask of every other row
    must be 0.  Only connect_edges_direct exists at this K: connect_edges_runs (K <= 4096) reads no pi, it indexes a mask
    whose largest word offset at this N is below 2^27, and is left out."""
    b = Bench()
    T = b.torch
    relate = b.ops.CommunityRelations(b.ctx)
    n, K = ps.BIG_ROWS, ps.BIG_K
    pi, compact, ids = b.big_pi(62)
    thr = ps.big_threshold(compact)
    keys = ps.big_keys(71)
    ref = big_reference(compact, thr, keys)
    # a kernel that keeps row * K in 32 bits would give the wrapped figures: each of them that reads pi differs from the
    # true ones (valid and skipped are counted from the keys alone)
    wrap = big_reference(ps.big_wrapped(compact), thr, keys)
    assert (ref["valid"], ref["skipped"]) == (wrap["valid"], wrap["skipped"]) and ref["skipped"] > 20
    assert not np.array_equal(ref["words"], wrap["words"])
    assert not (np.array_equal(ref["cells"], wrap["cells"]) and np.array_equal(ref["counts"], wrap["counts"]))
    assert not np.array_equal(ref["links"], wrap["links"]) and not np.array_equal(ref["overlap"], wrap["overlap"])
    assert all(not np.array_equal(x, y) for x, y in zip(ref["top"], wrap["top"]))
    del wrap
    print("big: the wrapped-offset reference differs in the mask words, directed, links, overlap, partners, their links "
          "and shared", flush=True)
    rows = np.concatenate([ids, np.asarray(ps.BIG_ZERO_ROWS, dtype=np.int64)])
    d_rows = b.ctx.from_numpy(rows)

    def mask_of(pi, form):
        mask = b.api.mask(pi, thr)
        assert b.api.kernel_name() == form, b.api.kernel_name()
        assert tuple(mask.shape) == (n, K // 64)
        assert np.array_equal(mask[d_rows].cpu().numpy().view(np.uint64), ref["words"]), form + ": the mask words differ"
        rest = mask.clone()
        rest[d_rows] = 0
        assert int(T.count_nonzero(rest)) == 0, form + ": a word of an unplanted row is set"
        return mask

    mask = mask_of(pi, "connect_mask_fast")
    force(None)
    d, cnt = b.api.edges(mask, n, K, keys)
    assert b.api.kernel_name() == "connect_edges_direct", b.api.kernel_name()
    want = b.want_dev(K, ref["cells"], ref["counts"])
    assert T.equal(d.view(-1), want), "directed differs from M[a].T @ M[b]"
    assert cnt.tolist() == [ref["valid"], ref["skipped"]], (cnt.tolist(), ref["valid"], ref["skipped"])
    links = b.api.finish(d)
    assert b.api.kernel_name() == "connect_finish"
    assert T.equal(links, want.view(K, K) + want.view(K, K).t()), "links differs from C + C.T"
    d_ov = b.ctx.zeros((K, K), T.int32)
    relate.pairs(relate.bits(pi, thr), K, n, d_ov)
    assert T.equal(d_ov, b.ctx.from_numpy(ref["overlap"].astype(np.int32))), "relate's overlap differs from M.T @ M"
    got = b.api.top(links, d_ov, "density", 4, 1)
    assert b.api.kernel_name() == "connect_top"
    for name, x, y, view in zip(("partners", "their links", "shared"), got, ref["top"], (np.int32, np.uint64, np.uint32)):
        assert np.array_equal(x.cpu().numpy().view(view), y), name + " differ"
    del pi, d, links, d_ov, want
    b.release()
    mis, again, _ = b.big_pi(62, misaligned=True)
    assert np.array_equal(again, compact)
    assert T.equal(mask, mask_of(mis, "connect_mask_generic")), "the two forms write other words"
    print("big ok: %d x %d, thr %.3g, %d keys (%d valid), %d cells linked" % (n, K, thr, keys.size, ref["valid"],
                                                                             ref["cells"].size), flush=True)


def planted_group():
    from mcmc_ammsb_gpu_amd import _connect
    b = Bench()
    T = b.torch

    def linked(host, thr, keys, by, top=4, min_links=1):
        pi = b.matrix(host)
        N, K = host.shape
        d, cnt = b.api.edges(b.api.mask(pi, thr), N, K, keys)
        links = b.api.finish(d)
        ov = overlap_of(members(host, thr))
        d_ov = b.ctx.from_numpy(ov.astype(np.uint32).view(np.int32)).reshape(K, K).contiguous()
        partner, plinks, pshared = b.api.top(links, d_ov, by, top, min_links)
        m = links.cpu().numpy().view(np.uint64)
        valid, skipped = cnt.tolist()
        return _connect.Linked(thr, by, min_links, np.diagonal(ov), (np.diagonal(m) // np.uint64(2)).astype(np.int64),
                               partner.cpu().numpy(), plinks.cpu().numpy().view(np.uint64),
                               pshared.cpu().numpy().view(np.uint32), valid, skipped, m, N=N)

    def key(a, bb):
        return (np.asarray(a, dtype=np.uint64) << np.uint64(32)) | np.asarray(bb, dtype=np.uint64)

    # columns 0 = {0..9} and 1 = {10..19}: every one of the 100 links between them, and a ring inside each; columns 2 =
    # {20..29} and 3 = {30..39} with their rings and no link between them or to the others
    host = np.zeros((40, 4), F32)
    for c in range(4):
        host[10 * c:10 * c + 10, c] = 0.8
    ring = lambda c: key(np.arange(10) + 10 * c, (np.arange(10) + 1) % 10 + 10 * c)   # noqa: E731
    aa, bb = np.meshgrid(np.arange(10), np.arange(10, 20))
    keys = np.concatenate([key(aa.reshape(-1), bb.reshape(-1))] + [ring(c) for c in range(4)])
    for by in MEASURES:
        r = linked(host, 0.5, keys, by)
        assert r.size.tolist() == [10] * 4 and r.internal.tolist() == [10] * 4 and (r.valid, r.skipped) == (140, 0)
        assert r.partner.tolist() == [[1, -1, -1, -1], [0, -1, -1, -1], [-1] * 4, [-1] * 4], (by, r.partner)
        assert r.links[0, 0] == 100 and r.links[1, 0] == 100 and r.shared[0, 0] == 0
        assert r.density[0, 0] == 1.0 and r.density[1, 0] == 1.0 and r.within.tolist() == [20 / 90] * 4
        assert r.bridged() == [(0, 1)] and r.bridged(4.0) == [(0, 1)] and r.bridged(5.0) == []
        assert (r.links[2:] == 0).all() and (r.shared[2:] == 0).all()
        assert not r.matrix[2:, :2].any() and not r.matrix[2, 3] and not r.matrix[3, 2]
    # ties go to the lower id: community 0 has 3 links to 1 and 3 links to 2, all of one size
    host = np.zeros((12, 4), F32)
    host[0:4, 0] = host[4:8, 1] = host[8:12, 2] = 1.0
    keys = key([0, 1, 2, 0, 1, 2], [4, 5, 6, 8, 9, 10])
    for by in MEASURES:
        r = linked(host, 0.5, keys, by, top=3)
        assert r.partner.tolist() == [[1, 2, -1], [0, -1, -1], [0, -1, -1], [-1, -1, -1]], (by, r.partner)
        assert r.links.tolist() == [[3, 3, 0], [3, 0, 0], [3, 0, 0], [0, 0, 0]], by
        assert r.density[0].tolist() == [3 / 16, 3 / 16, 0.0]
    # a pair with pairs == 0 is no partner by density: communities 0 and 1 are the same single node, with a loop on it
    host = np.zeros((3, 3), F32)
    host[0, 0] = host[0, 1] = host[1, 2] = host[2, 2] = 1.0
    keys = key([0, 0], [0, 1])
    r = linked(host, 0.5, keys, "links", top=2)
    assert r.partner.tolist() == [[1, 2], [0, 2], [0, 1]] and r.links.tolist() == [[2, 1], [2, 1], [1, 1]], (r.partner, r.links)
    assert r.shared.tolist() == [[1, 0], [1, 0], [0, 0]] and r.density[0].tolist() == [0.0, 0.5]
    r = linked(host, 0.5, keys, "density", top=2)
    assert r.partner.tolist() == [[2, -1], [2, -1], [0, 1]] and r.links.tolist() == [[1, 0], [1, 0], [1, 1]], (r.partner, r.links)
    # min_links above every count: no partner at all
    r = linked(host, 0.5, keys, "links", top=2, min_links=3)
    assert (r.partner == -1).all() and (r.links == 0).all() and (r.shared == 0).all()
    print("planted ok", flush=True)


def _check_linked(r, host, thr, keys, by, top, min_links, what):
    M = members(host, thr)
    K = M.shape[1]
    cells, counts, valid, skipped = statement(M, keys)
    C = np.zeros(K * K, np.int64)
    C[cells] = counts
    links = C.reshape(K, K) + C.reshape(K, K).T
    ov = overlap_of(M)
    assert np.array_equal(r.size, np.diagonal(ov)), what + ": sizes"
    assert np.array_equal(2 * r.internal, np.diagonal(links)), what + ": internal"
    assert (r.valid, r.skipped) == (valid, skipped), what + ": valid, skipped"
    wp, ww, ws = selection(ranking(links, ov, by), top, min_links)
    assert np.array_equal(r.partner, wp), what + ": partners differ"
    assert np.array_equal(r.links, ww), what + ": links differ"
    assert np.array_equal(r.shared, ws), what + ": shared differs"
    return links


def learner_group(graph):
    import torch
    from mcmc_ammsb_gpu_amd import _connect
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    keys = lrn.TrainingLinks().cpu().numpy().view(np.uint64)
    off, tgt = ds.training_csr()
    assert keys.size == int(np.diff(off.astype(np.int64)).sum()) // 2 and (np.diff(keys.astype(np.int64)) > 0).all()
    for thr in (0.05, 0.1):
        got = lrn.CommunityLinks(thr)
        assert got.dtype == torch.int64 and tuple(got.shape) == (K, K)
        q = lrn.CommunityQuality(thr)
        assert np.array_equal(np.diagonal(got.cpu().numpy()), 2 * q.internal), "thr=%g: the diagonal is not 2 internal" % thr
        for by, top, min_links in (("density", 4, 1), ("links", 1, 3), ("density", 31, 1), ("links", 64, 0)):
            r = lrn.LinkedCommunities(thr, top, by, min_links, dense=True)
            assert isinstance(r, _connect.Linked) and r.top == top and r.N == N
            want = _check_linked(r, host, thr, keys, by, top, min_links, "learner thr=%g by=%s top=%d" % (thr, by, top))
            assert np.array_equal(r.matrix.astype(np.int64), want) and np.array_equal(got.cpu().numpy(), want)
            cut = lrn.LinkedCommunities(thr, top, by, min_links, max_bytes=1000)
            assert cut.matrix is None and np.array_equal(cut.partner, r.partner) and np.array_equal(cut.links, r.links)
        sub = keys[::7].copy()
        sub[::50] |= np.uint64(0xFFFFFFFF)
        r = lrn.LinkedCommunities(thr, 4, "density", 1, edges=sub)
        _check_linked(r, host, thr, sub, "density", 4, 1, "learner thr=%g, a list of its own" % thr)
        assert r.skipped == sub[::50].size
        print("thr=%g: %d of %d community pairs linked" % (thr, int((np.triu(want, 1) > 0).sum()), K * (K - 1) // 2), flush=True)
    ps.rejects(AmmsbError, (lambda: lrn.CommunityLinks(-1.0), lambda: lrn.LinkedCommunities(top=65), lambda: lrn.LinkedCommunities(by="jaccard"),
                            lambda: lrn.LinkedCommunities(max_bytes=0), lambda: lrn.LinkedCommunities(min_links=-1)))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CommunityLinks(0.05)
        a.LinkedCommunities()
    ps.unperturbed_run(make, calls, "community links")
    print("learner ok graph=%s" % graph, flush=True)


def _check_linked_file(path, ckpt, lc, K, thr, by, top, min_links, what):
    """a linked-communities file against the statement over the pi of the checkpoint and the training links of the
    link-communities file the same process wrote; the Python writer reproduces its bytes"""
    from mcmc_ammsb_gpu_amd import _connect, _linkcomm
    fN, r = _connect.read_linked(path)
    assert r.size.size == K and F32(r.threshold) == F32(thr) and (r.by, r.top, r.min_links) == (by, top, min_links), what
    again = path + ".py"
    _connect.write_linked(again, fN, r)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the Python writer's bytes differ" % what
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    keys = np.ascontiguousarray(_linkcomm.read_link_communities(lc)[4], dtype=np.uint64)
    assert keys.size > 1000 and r.valid == keys.size and r.skipped == 0, what
    _check_linked(r, pi, thr, keys, by, top, min_links, what)
    return fN, r


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("connect_test", d, 300)
        fN, r = _check_linked_file(os.path.join(d, "linked.txt"), os.path.join(d, "cpp.ckpt"), os.path.join(d, "links.txt"), 64,
                                   0.05, "density", 4, 1, "connect_test")
        assert fN == 20000
        print("cpp ok: Learner::WriteLinkedCommunities equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a small generated graph; the links from the link-communities file of the same run
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck, lc = os.path.join(d, "r.txt"), os.path.join(d, "main.ckpt"), os.path.join(d, "lc.txt")
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--checkpoint-out", ck, "--link-communities-out", lc]
        for extra, thr, by, top, ml in (([], 0.05, "density", 4, 1),
                                        (["--linked-communities-threshold", "0.02", "--linked-communities-top", "64",
                                          "--linked-communities-by", "links", "--linked-communities-min-links", "3"], 0.02, "links", 64, 3),
                                        (["--linked-communities-by", "density", "--linked-communities-top", "1"], 0.05, "density", 1, 1)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--linked-communities-out", out] + extra, 240)
            fN, r = _check_linked_file(out, ck, lc, 48, thr, by, top, ml, "ammsb_main by=%s" % by)
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
