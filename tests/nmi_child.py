"""Child process of test_gpu_nmi.py (one per group): the pair pass of the overlapping NMI (include/ammsb_nmi.h,
ops.CoverNMI, Learner.CoverNMI) against the numpy float64 statement of the header's definitions, fed the same integers
and written with the same association:

    h(x) = -(x / N) * log2(x / N), h(0) = 0;  n11 = o, n10 = t - o, n01 = d - o, n00 = N - t - d + o
    H(X_g) = h(t) + h(N - t);  H(Y_k) = h(d) + h(N - d);  J = (h(n11) + h(n00)) + (h(n01) + h(n10))
    qualifies iff n00 >= 0 and h(n11) + h(n00) >= h(n01) + h(n10)
    c_truth[g] = min over the qualifying k of max(0, J - H(Y_k)), c_detected[k] likewise over g; +inf if none

The bound.  Both sides divide identically (IEEE); ROCm documents its double log2 at 1 ulp (e = 1) and numpy's is within
1 ulp as well, so a term differs by at most (2 e + 1) 2^-53 |h| and the adds contribute at most 6 2^-53 S, S being the
sum of the magnitudes of the h-terms that enter the element: 9 2^-53 S at e = 1, 15 2^-53 S at e = 4.  The bound used is
2^-47 S = 64 2^-53 S.  For a minimum S is the largest S among the qualifying pairs of the row or column, because
|min a - min b| <= max |a - b|.  +inf must match exactly, and so must the exact 0 of an identical pair.

The guard.  A pair whose two sides of the qualifying inequality are closer than rounding could qualify on one side only,
so before anything is compared reference() asserts that |lhs - rhs| is exactly 0 or above 1e-9 for every pair."""
import io
import os
import sys

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
FILL = -12345.678
TOL = 2.0 ** -47
INF = float("inf")
SEEN = set()
F32 = np.float32


def h_of(x, N):
    x = np.asarray(x, dtype=np.int64)
    p = np.maximum(x, 1).astype(np.float64) / float(N)
    return np.where(x > 0, -(p * np.log2(p)), 0.0)


def entropy_of(s, N):
    s = np.asarray(s, dtype=np.int64)
    return np.where(s >= N, 0.0, h_of(s, N) + h_of(np.maximum(N - s, 0), N))


def reference(N, t, d, ov):
    """-> dict: HX [G], HY [K], cX [G], cY [K] and the magnitudes sX, sY the bound of each minimum is made of; asserts
    the guard"""
    t, d, o = np.asarray(t, np.int64), np.asarray(d, np.int64), np.asarray(ov, np.int64)
    G, K = o.shape
    HX, HY = entropy_of(t, N), entropy_of(d, N)
    n10, n01, n00 = t[:, None] - o, d[None, :] - o, N - t[:, None] - d[None, :] + o
    valid = (n00 >= 0) & (n10 >= 0) & (n01 >= 0)
    a, b = h_of(o, N), h_of(np.maximum(n00, 0), N)
    c, e = h_of(np.maximum(n01, 0), N), h_of(np.maximum(n10, 0), N)
    lhs, rhs = a + b, c + e
    gaps = np.abs(lhs - rhs)[valid & (lhs != rhs)]
    gap = float(gaps.min()) if gaps.size else INF
    assert gap > 1e-9, "a borderline pair: |lhs - rhs| = %g" % gap
    q = valid & (lhs >= rhs)
    J = lhs + rhs
    S = np.abs(a) + np.abs(b) + np.abs(c) + np.abs(e)
    cX = np.where(q, np.maximum(0.0, J - HY[None, :]), INF).min(1, initial=INF)
    cY = np.where(q, np.maximum(0.0, J - HX[:, None]), INF).min(0, initial=INF)
    sX = np.where(q, S + HY[None, :], 0.0).max(1, initial=0.0)
    sY = np.where(q, S + HX[:, None], 0.0).max(0, initial=0.0)
    return dict(HX=HX, HY=HY, cX=cX, cY=cY, sX=sX, sY=sY, gap=gap, qualifying=int(q.sum()),
                zero_overlap_qualifying=int((q & (o == 0)).sum()))


def check(got, ref, what):
    for name, s in (("HX", None), ("HY", None), ("cX", "sX"), ("cY", "sY")):
        g, r = got[name], ref[name]
        assert g.shape == r.shape, (what, name, g.shape, r.shape)
        assert not np.isnan(g).any() and (g >= 0).all() and not np.signbit(g).any(), "%s: %s holds a NaN or a negative" % (what, name)
        assert np.array_equal(np.isinf(g), np.isinf(r)), "%s: %s: +inf at %s, want %s" % (
            what, name, np.flatnonzero(np.isinf(g))[:8], np.flatnonzero(np.isinf(r))[:8])
        fin = ~np.isinf(r)
        bound = TOL * (np.abs(r) if s is None else ref[s])
        err = np.abs(g[fin] - r[fin])
        bad = np.flatnonzero(err > bound[fin])
        assert not bad.size, "%s: %s off at %s: got %s, want %s, bound %s" % (
            what, name, bad[:5], g[fin][bad[:5]], r[fin][bad[:5]], bound[fin][bad[:5]])


def same_bits(a, b):
    return all(np.array_equal(a[n].view(np.uint64), b[n].view(np.uint64)) for n in ("HX", "HY", "cX", "cY"))


def slabbings(G):
    """the whole matrix, one row at a time, and a ragged three-way split"""
    cuts = sorted({0, G // 5, G // 5 + (G + 1) // 2, G})
    return {"whole": [(0, G)], "rows": [(g, g + 1) for g in range(G)], "ragged": list(zip(cuts[:-1], cuts[1:]))}


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _nmi
        super().__init__()
        self.nm = _nmi
        self.lib = _nmi.load()
        self.api = self.ops.CoverNMI(self.ctx)
        self.cover = self.ops.CoverMatch(self.ctx)
        self.ro = self.ops.CommunityReadout(self.ctx)

    def run(self, N, t, d, ov, slabs, misalign=False):
        """the library calls over buffers of this test's own, each followed by GUARD words that must survive; ov: a host
        uint32 [G, K] matrix or an int32 device tensor; every slab is passed as a pointer into it.  -> numpy arrays"""
        import ctypes as C
        T = self.torch
        G, K = int(ov.shape[0]), int(ov.shape[1])
        d_t = self.ctx.from_numpy(np.ascontiguousarray(t, dtype=np.uint32))
        d_d = d if T.is_tensor(d) else self.ctx.from_numpy(np.ascontiguousarray(d, dtype=np.int64))
        flat = ov.reshape(-1) if T.is_tensor(ov) else self.ctx.from_numpy(np.ascontiguousarray(ov, dtype=np.uint32).reshape(-1))
        store = self.ctx.empty((G * K + 1 + ps.GUARD,), T.int32)
        store.fill_(0x5A5A5A5A)
        lead = 1 if misalign else 0   # 4 bytes past a 16-byte boundary
        store[lead:lead + G * K].copy_(flat)
        base = store.data_ptr() + 4 * lead
        assert base % 16 == (4 if misalign else 0)
        bufs = {n: self.guarded(words, T.float64, FILL) for n, words in (("HX", G), ("HY", K), ("cX", G), ("cY", K))}
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        self.nm.check(self.lib.ammsb_nmi_begin(N, ptr(d_t), G, ptr(d_d), K, ptr(bufs["HX"]), ptr(bufs["HY"]),
                                               ptr(bufs["cX"]), ptr(bufs["cY"]), None))
        SEEN.add(self.nm.last_kernel_name())
        for g0, g1 in slabs:
            self.nm.check(self.lib.ammsb_nmi_accumulate(C.c_void_p(base + 4 * g0 * K), g0, g1 - g0, N, ptr(d_t), G,
                                                        ptr(d_d), K, ptr(bufs["HX"]), ptr(bufs["HY"]), ptr(bufs["cX"]),
                                                        ptr(bufs["cY"]), None))
            if g1 > g0:
                SEEN.add(self.nm.last_kernel_name())
        T.cuda.synchronize()
        out = {}
        for n, buf in bufs.items():
            hst = buf.cpu().numpy()
            words = G if n in ("HX", "cX") else K
            assert (hst[words:] == FILL).all(), "the words past %s were written" % n
            out[n] = hst[:words].copy()
        tail = store.cpu().numpy()
        assert (tail[lead + G * K:] == 0x5A5A5A5A).all() and (tail[:lead] == 0x5A5A5A5A).all()
        return out

    def all_slabbings(self, N, t, d, ov, ref, what):
        """every slabbing against the reference, bit-equal to each other and to a second call"""
        G = int(ov.shape[0])
        first = None
        for name, slabs in slabbings(G).items():
            got = self.run(N, t, d, ov, slabs)
            check(got, ref, "%s slabs=%s" % (what, name))
            if first is None:
                first = got
                assert same_bits(first, self.run(N, t, d, ov, slabs)), what + ": two calls differ"
            else:
                assert same_bits(first, got), "%s: slabs=%s differs from the whole matrix" % (what, name)
        return first


def random_pi(rng, N, K):
    host = rng.random((N, K)) ** 6 + 1e-9
    host /= host.sum(1, keepdims=True)
    return host.astype(F32)


def random_cover(rng, N, G):
    """communities of 0 .. 90 distinct members; a member == N and a member == 2^32 - 1 where the sizes allow it"""
    sizes = rng.integers(0, 91, G)
    if G >= 7:
        sizes[:3] = (0, 1, 90)
    lists = [rng.choice(N, int(sz), replace=False).astype(np.uint32) for sz in sizes]
    big = [i for i, c in enumerate(lists) if c.size >= 5]
    if big:
        lists[big[0]][1] = N
        lists[big[-1]][-1] = NONE
    offsets = np.zeros(G + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([c.size for c in lists])
    return offsets, np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)


def hand_matrix(rng, N, G, K):
    """integers of no particular cover: sparse overlaps, columns that hold more than half the nodes (their zero-overlap
    pairs can qualify), noisy copies of a row's community as a column, identical pairs, empty communities"""
    t = rng.integers(1, max(2, N // 3), G)
    d = rng.integers(1, max(2, N // 3), K)
    heavy = rng.random(K) < 0.15
    d[heavy] = rng.integers(N // 2 + 1, N, int(heavy.sum()))
    t[rng.random(G) < 0.1] = 0
    d[rng.random(K) < 0.05] = 0
    cap = np.minimum(t[:, None], d[None, :])
    ov = np.where(rng.random((G, K)) < 0.06, (rng.random((G, K)) * (cap + 1)).astype(np.int64), 0)
    for g in range(min(G, K)):                      # noisy copies and identical pairs on a diagonal
        k = (7 * g + 1) % K
        if g % 3 == 0 and t[g] > 0:
            d[k] = t[g]
            ov[:, k] = np.minimum(ov[:, k], np.minimum(t, d[k]))
            ov[g, k] = t[g]                         # identical: exactly 0
        elif g % 3 == 1 and t[g] > 4:
            d[k] = t[g] + 2
            ov[:, k] = np.minimum(ov[:, k], np.minimum(t, d[k]))
            ov[g, k] = t[g] - 3
    ov = np.minimum(ov, np.minimum(t[:, None], d[None, :]))
    return t.astype(np.int64), d.astype(np.int64), ov.astype(np.uint32)


def exact_group(ks):
    b = Bench()
    rng = np.random.default_rng(61)
    for K in ks:
        N = {1: 4999, 3: 1237, 64: 3000}.get(K, 600 if K >= 1024 else 911)
        host = random_pi(rng, N, K)
        pi = b.matrix(host)
        for G in (1, 7, 300):
            # (a) the overlap the cover match gives for a random pi and a random cover
            off, mem = random_cover(rng, N, G)
            for thr in (0.5 / K, 2.0 / K):
                what = "K=%d G=%d thr=%g (a)" % (K, G, thr)
                dsize = b.ro.sizes(pi, thr)
                _, _, ts, _, _, sk, ov = b.cover.match(pi, thr, off, mem, dsize, dense=True)
                t = ts.cpu().numpy().view(np.uint32)
                assert int(sk.item()) == int((mem.astype(np.int64) >= N).sum()), what
                ref = reference(N, t, dsize.cpu().numpy(), ov.cpu().numpy().view(np.uint32))
                b.all_slabbings(N, t, dsize, ov, ref, what)
            # (b) integers made by hand
            t, d, ovh = hand_matrix(rng, N, G, K)
            ref = reference(N, t, d, ovh)
            got = b.all_slabbings(N, t, d, ovh, ref, "K=%d G=%d (b)" % (K, G))
            for g in range(min(G, K)):
                if g % 3 == 0 and t[g] > 0:
                    assert got["cX"][g] == 0.0, "an identical pair does not give exactly 0 (g=%d)" % g
            print("K=%d G=%d: %d qualifying pairs, %d of them with overlap 0, smallest gap %.3g" % (
                K, G, ref["qualifying"], ref["zero_overlap_qualifying"], ref["gap"]), flush=True)
        # the layer above: ops.CoverNMI over its own tensors
        st = b.api.begin(N, t, b.ctx.from_numpy(d))
        dev = b.ctx.from_numpy(ovh.reshape(-1)).reshape(ovh.shape)
        for g0, g1 in slabbings(300)["ragged"]:
            b.api.accumulate(st, dev[g0:g1], g0)
        b.api.accumulate(st, dev[0:0], 0)
        b.torch.cuda.synchronize()
        got2 = dict(HX=st.H_truth.cpu().numpy(), HY=st.H_detected.cpu().numpy(), cX=st.c_truth.cpu().numpy(),
                    cY=st.c_detected.cpu().numpy())
        assert same_bits(got, got2), "ops.CoverNMI differs from the library calls at K=%d" % K
        print("exact K=%d ok (%s)" % (K, b.nm.last_kernel_name()), flush=True)
    print("exact ok", flush=True)


def planted_group():
    from mcmc_ammsb_gpu_amd import hostlib
    b = Bench()
    rng = np.random.default_rng(66)
    # truth == the detected cover under a column permutation
    N, G = 3000, 24
    off, mem = hostlib.generate_cover(N, G, seed=17)
    perm = rng.permutation(G)
    host = np.zeros((N, G), dtype=F32)
    for g in range(G):
        host[mem[int(off[g]):int(off[g + 1])], perm[g]] = 1
    host /= host.sum(1, keepdims=True)
    pi = b.matrix(host)

    def through_the_match(thr, off, mem):
        dsize = b.ro.sizes(pi, thr)
        _, _, ts, _, _, sk, ov = b.cover.match(pi, thr, off, mem, dsize, dense=True)
        t = ts.cpu().numpy().view(np.uint32)
        got = b.run(N, t, dsize, ov, [(0, int(ov.shape[0]))])
        ref = reference(N, t, dsize.cpu().numpy(), ov.cpu().numpy().view(np.uint32))
        check(got, ref, "planted thr=%g" % thr)
        return b.nm.NMI(thr, t, dsize.cpu().numpy(), int(sk.item()), got["HX"], got["cX"], got["HY"], got["cY"]), got

    r, got = through_the_match(0.05, off, mem)
    assert (got["cX"] == 0.0).all() and (got["cY"] == 0.0).all() and (got["HX"] > 0).all()
    assert np.array_equal(np.sort(got["HX"]), np.sort(got["HY"]))
    assert r.nmi_lfk == 1.0 and abs(r.nmi_max - 1.0) <= 4 * np.finfo(np.float64).eps, (r.nmi_lfk, r.nmi_max)
    # thr = 0: every d_k = N and H(Y_k) = 0: those k are left out of the mean, which leaves nothing on that side
    r, got = through_the_match(0.0, off, mem)
    assert (r.detected_size == N).all() and (got["HY"] == 0.0).all() and r.nmi_lfk == -1.0
    # thr above every value: every detected community is empty, H(Y_k) = 0 again; nmi_max keeps the denominator
    # sum H(X_g) > 0 and is 0 -- and -1 as well once the ground truth is empty too (every member skipped)
    r, got = through_the_match(2.0, off, mem)
    assert not r.detected_size.any() and (got["HY"] == 0.0).all() and r.nmi_lfk == -1.0 and r.nmi_max == 0.0
    assert np.array_equal(r.h_truth, r.H_truth)
    gone = np.where(np.arange(mem.size) % 2 == 0, N, NONE).astype(np.uint32)     # a member == N, a member == 2^32 - 1
    r, got = through_the_match(2.0, off, gone)
    assert r.skipped == mem.size and not r.truth_size.any() and (r.nmi_lfk, r.nmi_max) == (-1.0, -1.0)
    assert (got["cX"] == 0.0).all()            # t = d = o = 0 is an identical pair: the shortcut must not skip it
    r, got = through_the_match(0.05, off, np.concatenate([mem[:-2], [N, NONE]]).astype(np.uint32))
    assert r.skipped == 2 and r.truth_size[-1] == int(off[-1] - off[-2]) - 2

    one = lambda N, t, d, o: (b.run(N, [t], [d], np.array([[o]], np.uint32), [(0, 1)]), reference(N, [t], [d], [[o]]))   # noqa: E731
    # lhs == rhs exactly: the pair qualifies and c = 1 = H
    got, ref = one(8, 4, 4, 2)
    assert ref["gap"] == INF and got["cX"][0] == 1.0 == got["HX"][0] == got["cY"][0] == got["HY"][0]
    # a detected community that is the complement of the truth community, and the complement plus one shared node:
    # neither qualifies, +inf, and the fallback on the host
    for d, o in ((6, 0), (7, 1)):
        got, ref = one(10, 4, d, o)
        check(got, ref, "complement")
        assert got["cX"][0] == INF and got["cY"][0] == INF
        r = b.nm.NMI(0.05, [4], [d], 0, got["HX"], got["cX"], got["HY"], got["cY"])
        assert r.h_truth[0] == got["HX"][0] and r.h_detected[0] == got["HY"][0] and r.nmi_lfk == 0.0
    # the zero-overlap pair that does qualify, and its neighbour below half the nodes that the shortcut skips
    got, ref = one(1000, 1, 599, 0)
    check(got, ref, "zero overlap")
    assert ref["zero_overlap_qualifying"] == 1 and np.isfinite(got["cX"][0]) and np.isfinite(got["cY"][0])
    got, ref = one(1000, 1, 400, 0)
    check(got, ref, "zero overlap, skipped")
    assert got["cX"][0] == INF
    # inputs that break the contract are safe: o > t, o > d, t > N, d > N never qualify and give H = 0 past N
    got = b.run(100, [5, 200, 7], [3, 500, 2**40], np.array([[9, 0, 1], [0, 300, 0], [1, 1, 7]], np.uint32), [(0, 3)])
    assert got["HX"][1] == 0.0 and got["HY"][1] == 0.0 and got["HY"][2] == 0.0
    assert not np.isnan(np.concatenate(list(got.values()))).any()
    print("planted ok", flush=True)


def forms_group():
    """both kernel forms are named and reached, on both sides of the 1024-column chunk boundary, and a misaligned
    overlap takes the generic form and gives the same bits"""
    import re
    b = Bench()
    rng = np.random.default_rng(64)
    N, G = 2000, 37
    for K, form in ((4, "fast"), (1020, "fast"), (1023, "generic"), (1024, "fast"), (1025, "generic"), (1028, "fast"),
                    (2048, "fast"), (2052, "fast"), (8190, "generic"), (8192, "fast")):
        t, d, ov = hand_matrix(rng, N, G, K)
        ref = reference(N, t, d, ov)
        got = b.run(N, t, d, ov, [(0, G)])
        assert b.nm.last_kernel_name() == "nmi_" + form, (K, b.nm.last_kernel_name())
        check(got, ref, "forms K=%d" % K)
        assert ref["qualifying"] > 0
        mis = b.run(N, t, d, ov, [(0, 10), (10, G)], misalign=True)
        assert b.nm.last_kernel_name() == "nmi_generic", (K, b.nm.last_kernel_name())
        assert same_bits(got, mis), "K=%d: the misaligned base gives other bits" % K
    src = open(os.path.join(ps.ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_nmi.hip")).read()
    in_source = set(re.findall(r'"(nmi_[a-z0-9_]+)"', src))
    print("forms seen: %s" % " ".join(sorted(SEEN)), flush=True)
    assert SEEN == in_source == set(b.nm.KERNEL_FORMS)
    print("forms ok", flush=True)


def persistent_group():
    """more tiles than the grid has blocks (512 blocks of four rows x 1024 columns): 750 tiles at G = 3000, K = 64 and
    600 at G = 300, K = 8192, where a block also moves from one column chunk to the next"""
    b = Bench()
    rng = np.random.default_rng(65)
    for G, K in ((3000, 64), (300, 8192)):
        N = 4999
        t, d, ov = hand_matrix(rng, N, G, K)
        ref = reference(N, t, d, ov)
        got = b.run(N, t, d, ov, [(0, G)])
        check(got, ref, "persistent G=%d K=%d" % (G, K))
        assert same_bits(got, b.run(N, t, d, ov, slabbings(G)["ragged"]))
        print("persistent G=%d K=%d ok: %d qualifying pairs" % (G, K, ref["qualifying"]), flush=True)
    print("persistent ok", flush=True)


def _statement_over_pi(host, thr, off, mem):
    """(t, d, overlap, skipped) in integers from the checkpointed pi"""
    N = host.shape[0]
    with np.errstate(invalid="ignore"):
        M = host >= F32(thr)
    d = M.sum(0).astype(np.int64)
    G = off.size - 1
    t, ov, skipped = np.zeros(G, np.int64), np.zeros((G, host.shape[1]), np.int64), 0
    for g in range(G):
        m = mem[int(off[g]):int(off[g + 1])].astype(np.int64)
        ok = m < N
        skipped += int((~ok).sum())
        t[g] = ok.sum()
        if t[g]:
            ov[g] = M[m[ok]].sum(0)
    return t, d, ov, skipped


def _check_nmi(r, host, thr, off, mem, what):
    t, d, ov, skipped = _statement_over_pi(host, thr, off, mem)
    ref = reference(host.shape[0], t, d, ov)
    assert np.array_equal(r.truth_size, t) and np.array_equal(r.detected_size, d) and r.skipped == skipped, what
    want = dict(HX=ref["HX"], HY=ref["HY"], cX=np.minimum(ref["cX"], ref["HX"]), cY=np.minimum(ref["cY"], ref["HY"]),
                sX=np.maximum(ref["sX"], ref["HX"]), sY=np.maximum(ref["sY"], ref["HY"]))
    check(dict(HX=r.H_truth, HY=r.H_detected, cX=r.h_truth, cY=r.h_detected), want, what)
    return ref


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _nmi, hostlib
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    off, mem = hostlib.generate_cover(N, k_true, seed=20260101)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    lists = [mem[int(off[g]):int(off[g + 1])].tolist() for g in range(k_true)]
    for thr in (0.05, 0.01, 0.0, 2.0):
        first = None
        for truth, slab in (((off, mem), 256 << 20), (lists, 4 * K), (lists, 5 * 4 * K + 3)):
            r = lrn.CoverNMI(truth, thr, slab_bytes=slab)
            assert isinstance(r, _nmi.NMI)
            _check_nmi(r, host, thr, off, mem, "learner thr=%g slab=%d" % (thr, slab))
            assert np.array_equal(r.detected_size, lrn.CommunitySizes(thr).cpu().numpy())
            assert (r.nmi_lfk, r.nmi_max) == _nmi.scores(r.H_truth, r.h_truth, r.H_detected, r.h_detected)
            if first is None:
                first = r
            for name in ("H_truth", "H_detected", "h_truth", "h_detected"):
                assert np.array_equal(getattr(first, name).view(np.uint64), getattr(r, name).view(np.uint64)), (thr, slab, name)
        print("thr=%g: nmi_lfk %.4f nmi_max %.4f" % (thr, r.nmi_lfk, r.nmi_max), flush=True)
    # members the graph does not have are skipped; an empty cover is a valid call
    spoiled = np.concatenate([mem[:50], [N, NONE]]).astype(np.uint32)
    cut = np.array([0, 20, 52], np.uint64)
    r = lrn.CoverNMI((cut, spoiled), 0.05)
    _check_nmi(r, host, 0.05, cut, spoiled, "learner: spoiled")
    assert r.skipped == 2
    for none in ([], [[], []], (np.zeros(1, np.uint64), np.zeros(0, np.uint32))):
        r = lrn.CoverNMI(none, 0.05)
        assert r.nmi_lfk == -1.0 and not r.H_truth.any() and r.H_detected.size == K
    ps.rejects(AmmsbError, (lambda: lrn.CoverNMI(lists, -1.0), lambda: lrn.CoverNMI(lists, float("nan")),
                            lambda: lrn.CoverNMI((np.array([0, 9]), mem[:3]))))
    ps.rejects(ValueError, (lambda: lrn.CoverNMI([[1, 2, 1]]),))
    lrn.close()
    # Run(20), the calls, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CoverNMI((off, mem))
        a.CoverNMI(lists, 0.01, slab_bytes=1)
    ps.unperturbed_run(make, calls, "cover NMI")
    print("learner ok graph=%s" % graph, flush=True)


def _check_nmi_file(path, ckpt, K, thr, offsets, members, what):
    """a cover-NMI file against the statement over the pi of the checkpoint the same process wrote; the Python writer
    reproduces its bytes, the scores in the header line included"""
    from mcmc_ammsb_gpu_amd import _nmi
    fN, r, printed = _nmi.read_cover_nmi(path)
    assert r.H_detected.size == K and F32(r.threshold) == F32(thr), (r.H_detected.size, r.threshold)
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    _check_nmi(r, pi, thr, offsets, members, what)
    assert printed == (r.nmi_lfk, r.nmi_max), (what, printed, r.nmi_lfk, r.nmi_max)
    again = path + ".py"
    _nmi.write_cover_nmi(again, fN, r)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the Python writer's bytes differ" % what
    return fN, r


def cpp_group():
    import tempfile
    from cover_child import _check_match_file
    from mcmc_ammsb_gpu_amd import _cover, hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("nmi_test", d, 240)
        lists = [[int(w) for w in ln.split()[1:]] for ln in open(os.path.join(d, "truth.txt"))]
        offsets, members = _cover.check_cover(lists)
        fN, res = _check_nmi_file(os.path.join(d, "nmi.txt"), os.path.join(d, "cpp.ckpt"), 64, 0.05, offsets, members, "nmi_test")
        assert fN == 20000 and res.H_truth.size == 18 and res.skipped == 2
        print("cpp ok: Learner::WriteCoverNMI equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a data-set dump: the ground truth speaks of dense ids
        N = 6000
        f = os.path.join(d, "g.bin.gz")
        edges = hostlib.generate_graph(N, 8, 12, seed=3)
        hostlib.dump_dataset(f, N, 0.02, edges)
        toff, tmem = hostlib.generate_cover(N, 8, seed=3)
        truth, out, ck = os.path.join(d, "truth.cmty"), os.path.join(d, "n.txt"), os.path.join(d, "main.ckpt")
        mout = os.path.join(d, "m.txt")
        _cover.write_cover(truth, toff, tmem)
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--ground-truth", truth, "--checkpoint-out", ck]
        for extra, thr in ((["--cover-nmi-out", out], 0.05),
                           (["--cover-nmi-out", out, "--cover-match-out", mout, "--cover-match-threshold", "0.01"], 0.01)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + extra, 240)
            fN, res = _check_nmi_file(out, ck, 48, thr, toff, tmem, "ammsb_main dump thr=%g" % thr)
            assert fN == N and res.H_truth.size == 8 and res.skipped == 0
        _check_match_file(mout, ck, 48, 0.01, toff, tmem, "ammsb_main dump: the cover match beside the NMI")
        # --cover-match-out alone still works, unchanged
        os.remove(mout)
        os.remove(out)
        r = ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--cover-match-out", mout], 240)
        assert not os.path.exists(out), r.stderr[-3000:]
        _check_match_file(mout, ck, 48, 0.05, toff, tmem, "ammsb_main dump: --cover-match-out alone")
        # ... and on a text graph whose ids are not dense: the ground truth speaks of the file's ids
        name = lambda v: 7 * int(v) + 100     # noqa: E731
        txt = os.path.join(d, "g.txt")
        with open(txt, "w") as fh:
            fh.write("# a\n# b\n# c\n# d\n")
            for e in edges.tolist():
                fh.write("%d\t%d\n" % (name(e >> 32), name(e & 0xFFFFFFFF)))
        fN, _, ids = hostlib.load_snap_ids(txt)
        dense_of = {int(v): i for i, v in enumerate(ids.tolist())}
        with open(truth, "w") as fh:
            fh.write("# planted cover, in the graph file's ids\n")
            for g in range(8):
                mem = [name(a) for a in tmem[int(toff[g]):int(toff[g + 1])]]
                fh.write(" ".join("%d" % a for a in mem + [3, 5][:g % 3]) + "\n")     # (3 and 5 are nobody's id)
        woff, wmem, dropped = _cover.read_cover(truth, dense_of)
        assert dropped > 0 and woff.size == 9
        ps.run_ammsb_main(["-f", txt] + tail + ["--cover-nmi-out", out], 240)
        gN, res = _check_nmi_file(out, ck, 48, 0.05, woff, wmem, "ammsb_main text graph")
        assert gN == fN and res.H_truth.size == 8 and res.skipped == 0 and int(res.truth_size.sum()) == wmem.size
        # the three flag rules: status 2, before the graph is read
        for extra in (["--ground-truth", truth], ["--cover-nmi-out", out], ["--cover-match-out", mout]):
            r = ps.run_ammsb_main(["-f", os.path.join(d, "missing.txt"), "-k", "8"] + extra, 60, status=2)
            assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(k) for k in a) or (1, 3, 64, 65, 260, 1024, 1028, 8192)),
    "planted": lambda a: planted_group(),
    "forms": lambda a: forms_group(),
    "persistent": lambda a: persistent_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
