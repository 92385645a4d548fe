"""Child process of test_gpu_modularity.py (one per group): the overlapping modularity (include/ammsb_modularity.h,
ops.Modularity, Learner.Modularity) against the Python-integer statement of the header's definitions, written once here:

    M = pi >= np.float32(thr);  O[a] = the members of row a;  F = 2^62
    over the keys with both ends < N (m of them):  deg[a] += 1, deg[b] += 1;  IN[k] += F // (O[a] O[b]) for k in M[a] & M[b]
    SV[k] = the sum over the nodes a of k of deg[a] (F // O[a])
    in_k, s_k, q_k, q: _modularity.derive over these integers (the one host formula, applied to both sides' integers)

Python integers do not round, and the device adds modulo 2^128 in any order: everything integer must be equal, and the
float64 values, one formula over equal integers, are bit-equal.  The only tolerance below is the derived bound of the
planted group against the unquantised rationals."""
import io
import os
import sys
from fractions import Fraction

import numpy as np

import postfit_support as ps

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
F32 = np.float32
F = 1 << 62
# the kernels' constants (csrc/ammsb_modularity.hip, csrc/ammsb_postfit.h)
M_WAVES, MAX_GRID = 4, 2048


def members(pi, thr):
    return pi >= F32(thr)


def ends_of(keys):
    return (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)


def statement(M, keys):
    """-> (IN [K], SV [K] lists of Python ints, deg [N] uint32, valid, skipped)"""
    N, K = M.shape
    a, b = ends_of(keys)
    ok = (a < N) & (b < N)
    a, b = a[ok], b[ok]
    deg = np.bincount(a, minlength=N) + np.bincount(b, minlength=N)
    sets = [frozenset(np.flatnonzero(row).tolist()) for row in M]
    IN, SV = [0] * K, [0] * K
    for u, v in zip(a.tolist(), b.tolist()):
        both = sets[u] & sets[v]
        if both:
            w = F // (len(sets[u]) * len(sets[v]))
            for k in both:
                IN[k] += w
    for u in np.flatnonzero(deg).tolist():
        if sets[u]:
            t = int(deg[u]) * (F // len(sets[u]))
            for k in sets[u]:
                SV[k] += t
    return IN, SV, deg.astype(np.uint32), int(ok.sum()), int((~ok).sum())


def edge_list(rng, N, n, lonely=None):
    """n keys over N nodes, both orders of the ends: about a twentieth each self loops, repeats of earlier keys, and keys
    with an end >= N (N itself, a little past it, 2^32 - 1); node `lonely` is an end of none"""
    a, b = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    loops = rng.random(n) < 0.05
    b[loops] = a[loops]
    if lonely is not None:
        a[a == lonely] = (lonely + 1) % N
        b[b == lonely] = (lonely + 1) % N
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


def random_pi(rng, N, K, thr, empty=None):
    """about K^-1/2 of the entries at or above thr; NaNs and values equal to thr planted; row `empty` below thr throughout"""
    host = (rng.random((N, K)) * 0.9 * thr).astype(F32)
    above = rng.random((N, K)) < K ** -0.5
    host[above] = (thr + rng.random(int(above.sum())) * (1 - thr)).astype(F32)
    flat = host.reshape(-1)
    spots = rng.choice(flat.size, min(flat.size, max(2, flat.size // 50)), replace=False)
    flat[spots[::2]] = np.nan
    flat[spots[1::2]] = F32(thr)
    if empty is not None:
        host[empty] = F32(0.5) * F32(thr)
    return host


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _modularity
        super().__init__()
        self.md = _modularity
        self.lib = _modularity.load()
        self.api = self.ops.Modularity(self.ctx)
        self.links = self.ops.CommunityLinks(self.ctx)

    def sums(self, mask, N, K, cuts, what):
        """the edge call over guarded buffers, the list in the pieces `cuts`, then the node call -> (IN [K], SV [K] object
        arrays, deg [N] uint32, counts [2]) on the host"""
        import ctypes as C
        T = self.torch
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        deg = self.guarded(N, T.int32, FILL32, zero=True)
        internal, volume = self.guarded(2 * K, T.int64, FILL64, zero=True), self.guarded(2 * K, T.int64, FILL64, zero=True)
        cnt = self.guarded(2, T.int64, FILL64, zero=True)
        form = "w1" if K <= self.md.W1_MAX_COLS else "w2"
        for keys in cuts:
            dev = self.ctx.from_numpy(keys) if keys.size else None
            self.md.check(self.lib.ammsb_modularity_edges(ptr(mask), N, K, ptr(dev) if keys.size else None, keys.size, ptr(deg),
                                                          ptr(internal), ptr(cnt), None))
            if keys.size:
                assert self.md.last_kernel_name() == "modularity_edges_" + form, self.md.last_kernel_name()
        self.md.check(self.lib.ammsb_modularity_nodes(ptr(mask), N, K, ptr(deg), ptr(volume), None))
        assert self.md.last_kernel_name() == "modularity_nodes_" + form, self.md.last_kernel_name()
        d, i, v, c = deg.cpu().numpy().view(np.uint32), internal.cpu().numpy().view(np.uint64), \
            volume.cpu().numpy().view(np.uint64), cnt.cpu().numpy()
        assert (d[N:] == FILL32).all() and (i[2 * K:] == FILL64).all() and (v[2 * K:] == FILL64).all() and \
            (c[2:].view(np.uint64) == FILL64).all(), what + ": the words past an output were written"
        return self.md.wide(i[:2 * K]), self.md.wide(v[:2 * K]), d[:N].copy(), c[:2].tolist()

    def against(self, host, thr, keys, what, cuts=None):
        """one run of both calls against the statement -> what the device gave"""
        N, K = host.shape
        M = members(host, thr)
        mask = self.links.mask(self.matrix(host), float(F32(thr)))
        IN, SV, deg, valid, skipped = statement(M, keys)
        got = self.sums(mask, N, K, [keys] if cuts is None else cuts, what)
        assert got[3] == [valid, skipped], "%s: counts %s, not %s" % (what, got[3], (valid, skipped))
        assert np.array_equal(got[2], deg), what + ": degrees differ"
        assert got[0].tolist() == IN, what + ": internal differs from the statement"
        assert got[1].tolist() == SV, what + ": volume differs from the statement"
        return got, mask


def same(x, y):
    return x[0].tolist() == y[0].tolist() and x[1].tolist() == y[1].tolist() and np.array_equal(x[2], y[2]) and x[3] == y[3]


# (N, K, keys): W = 1, 1, 1, 2, 4, 16, 64 and then the two-word form; K = 65 and 4160 have a last word with unused bits
EXACT = ((2000, 1, 20000), (2000, 5, 20000), (2000, 64, 20000), (2000, 65, 20000), (2000, 256, 20000), (1500, 1024, 12000),
         (700, 4096, 5000), (700, 4160, 5000), (500, 8192, 4000))


def exact_group(which):
    b = Bench()
    rng = np.random.default_rng(17)
    for i, (N, K, n) in enumerate(EXACT):
        host = random_pi(rng, N, K, 0.05, empty=3)   # node 3 has no community, node 5 no edge
        keys = edge_list(rng, N, n, lonely=5)
        if which and i not in which:
            continue
        what = "N=%d K=%d" % (N, K)
        got, mask = b.against(host, 0.05, keys, what)
        assert got[2][5] == 0 and got[2][3] > 0
        again = b.sums(mask, N, K, [keys], what)
        assert same(got, again), what + ": two runs differ"
        print("exact %s: %d valid keys, %d communities with a link inside" % (what, got[3][0], sum(v > 0 for v in got[0])), flush=True)
    if not which or 2 in which:
        # thr = 0: every stored number but a NaN is a member, O = K for every node without a NaN
        host = (rng.random((300, 64)) * 0.5).astype(F32)
        keys = edge_list(rng, 300, 3000)
        got, _ = b.against(host, 0.0, keys, "thr=0 K=64")
        assert got[0].tolist() == [got[3][0] * (F // 4096)] * 64
        # an empty list: nothing is added and nothing launched for the edges
        got, _ = b.against(host, 0.05, np.zeros(0, np.uint64), "no key")
        assert got[3] == [0, 0] and not any(got[0].tolist()) and not any(got[1].tolist())
        print("exact thr=0, empty list ok", flush=True)
    print("exact ok", flush=True)


def carry_group():
    """5 and 9 links inside a community of single-membership nodes: IN = 5 * 2^62 and 9 * 2^62, so the low word wraps once
    and twice; node 0 has degree >= 4 in it, so deg * 2^62 has a high part.  The same links next to each other (one block)
    and spread over a list of keys that are skipped (many blocks), under both forms."""
    b = Bench()
    for K in (3, 4160):
        N = 40
        host = np.zeros((N, K), F32)
        host[:10, 0] = 0.9          # nodes 0..9 in community 0 only
        host[10:20, 1] = 0.9
        host[10:20, K - 1] = 0.9    # nodes 10..19 in two
        for links in ([(0, 1), (0, 2), (0, 3), (0, 4), (5, 6)], [(0, 1), (0, 2), (0, 3), (0, 4), (5, 6), (6, 7), (7, 8), (8, 9), (9, 0)]):
            key = np.array([(u << 32) | v for u, v in links], dtype=np.uint64)
            what = "carry K=%d links=%d" % (K, len(links))
            got, mask = b.against(host, 0.5, key, what)
            assert got[0][0] == len(links) * F and got[0][0] >> 64 == len(links) // 4
            assert got[1][0] == 2 * len(links) * F and got[2][0] >= 4
            gap = 4096
            spread = np.full(len(links) * gap, (N << 32) | 1, dtype=np.uint64)   # (an end >= N: skipped)
            spread[::gap] = key
            assert spread.size > 4 * M_WAVES * 64    # more than a handful of blocks under either form
            far, _ = b.against(host, 0.5, spread, what + " spread")
            assert far[0].tolist() == got[0].tolist() and far[1].tolist() == got[1].tolist() and np.array_equal(far[2], got[2])
            assert far[3] == [len(links), spread.size - len(links)]
        # links inside the two-membership community add 2^62 / 4 each; with the single-membership ones in one list
        mixed = np.array([(10 << 32) | 11, (11 << 32) | 12, (0 << 32) | 1, (12 << 32) | 12], dtype=np.uint64)
        got, _ = b.against(host, 0.5, mixed, "carry K=%d mixed" % K)
        assert got[0][1] == got[0][K - 1] == 3 * (F // 4) and got[0][0] == F
        print("carry K=%d ok" % K, flush=True)
    print("carry ok", flush=True)


def cut_group():
    """one call against three ragged calls, with more edges than one pass of the persistent grid: a group of 16 lanes per
    edge at K = 1024 (4 edges per wave and trip), a wave per edge at K = 4160"""
    b = Bench()
    rng = np.random.default_rng(23)
    for N, K, epw, extra in ((2000, 1024, 4, 7001), (600, 4160, 1, 1801)):
        n = MAX_GRID * M_WAVES * epw + extra
        host = random_pi(rng, N, K, 0.05)
        a, bb = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
        keys = (a << np.uint64(32)) | bb
        keys[::997] |= np.uint64(0xFFFFFFFF)
        what = "cut K=%d n=%d" % (K, n)
        M = members(host, 0.05)
        mask = b.links.mask(b.matrix(host), float(F32(0.05)))
        one = b.sums(mask, N, K, [keys], what)
        c1, c2 = n // 3 - 7, 2 * n // 3 + 5
        three = b.sums(mask, N, K, [keys[:c1], keys[c1:c2], keys[c2:]], what + " in three")
        assert same(one, three), what + ": three ragged calls differ from one"
        IN, SV, deg, valid, skipped = statement(M, keys)
        assert one[0].tolist() == IN and one[1].tolist() == SV and np.array_equal(one[2], deg) and one[3] == [valid, skipped], what
        print("%s ok" % what, flush=True)
    print("cut ok", flush=True)


def big_group():
    """pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, zero but 640 planted rows
    in four windows): run() over connect's keys of that fixture, with the mask in the 16-byte form and, from a base 4 bytes
    past a 16-byte boundary, in the generic form.  The statement is evaluated over the planted rows and the zero rows with
    the keys remapped; the degree of every other row must be 0.  The forms are modularity_edges_w2 / modularity_nodes_w2
    at this K; the _w1 forms (K <= 4096) read no pi, they index a mask whose largest word offset at this N is below 2^27,
    and are left out."""
    b = Bench()
    T = b.torch
    n, K = ps.BIG_ROWS, ps.BIG_K
    pi, compact, ids = b.big_pi(64)
    thr = ps.big_threshold(compact)
    keys = ps.big_keys(71)
    local = ps.big_remap(keys)
    IN, SV, deg, valid, skipped = statement(members(ps.big_extended(compact), thr), local)
    # a kernel that keeps row * K in 32 bits would give the wrapped figures: those that read pi differ from the true
    # ones (the degrees, valid and skipped are counted from the keys alone)
    wIN, wSV, wdeg, wvalid, wskipped = statement(members(ps.big_extended(ps.big_wrapped(compact)), thr), local)
    assert IN != wIN and SV != wSV and np.array_equal(deg, wdeg) and (valid, skipped) == (wvalid, wskipped)
    assert sum(v > 0 for v in IN) > 100 and skipped > 20 and deg[640:].all()
    print("big: the wrapped-offset reference differs in internal and volume", flush=True)
    rows = np.concatenate([ids, np.asarray(ps.BIG_ZERO_ROWS, dtype=np.int64)])
    d_rows = b.ctx.from_numpy(rows)

    def run(pi, mform):
        internal, volume, counts, degree = b.api.run(pi, thr, keys)
        assert b.api.kernel_name() == "modularity_nodes_w2", b.api.kernel_name()
        wide = lambda t: b.md.wide(t.cpu().numpy().view(np.uint64)).tolist()   # noqa: E731
        assert counts.cpu().numpy().tolist() == [valid, skipped], mform
        assert wide(internal) == IN, mform + ": internal differs from the statement"
        assert wide(volume) == SV, mform + ": volume differs from the statement"
        assert tuple(degree.shape) == (n,)
        assert np.array_equal(degree[d_rows].cpu().numpy().view(np.uint32), deg), mform + ": degrees differ"
        rest = degree.clone()
        rest[d_rows] = 0
        assert int(T.count_nonzero(rest)) == 0, mform + ": a node without a key has a degree"
        # the calls of run() one by one: the names of the forms that ran
        mask = b.links.mask(pi, float(F32(thr)))
        assert b.links.kernel_name() == mform, b.links.kernel_name()
        state = b.api.edges(mask, n, K, keys)
        assert b.api.kernel_name() == "modularity_edges_w2", b.api.kernel_name()
        assert T.equal(state[1], internal) and T.equal(state[0], degree) and T.equal(state[2], counts)
        return internal, volume, counts, degree

    first = run(pi, "connect_mask_fast")
    del pi
    b.release()
    mis, again, _ = b.big_pi(64, misaligned=True)
    assert np.array_equal(again, compact)
    second = run(mis, "connect_mask_generic")
    assert all(T.equal(x, y) for x, y in zip(first, second)), "the two forms of the mask give other sums"
    print("big ok: %d x %d, thr %.3g, %d valid keys, %d communities with a link inside" % (
        n, K, thr, valid, sum(v > 0 for v in IN)), flush=True)


def cross_group():
    """on a partition internal[k] == CommunityQuality's internal[k] << 62 and volume[k] == (2 internal + boundary)[k] << 62"""
    b = Bench()
    rng = np.random.default_rng(29)
    N, K = 2000, 65
    host = np.full((N, K), 0.001, F32)
    host[np.arange(N), rng.integers(0, K, N)] = 0.9
    keys = edge_list(rng, N, 20000)
    got, _ = b.against(host, 0.05, keys, "cross")
    quality = b.ops.CommunityQuality(b.ctx)
    q = quality.edges(quality.mask(b.matrix(host), float(F32(0.05))), N, K, keys).cpu().numpy()
    internal, boundary = q[:K].tolist(), q[K:2 * K].tolist()
    assert sum(internal) > 100 and int(q[2 * K + 1]) == got[3][1]
    assert got[0].tolist() == [v << 62 for v in internal], "internal is not CommunityQuality's << 62"
    assert got[1].tolist() == [(2 * i + o) << 62 for i, o in zip(internal, boundary)], "volume is not (2 internal + boundary) << 62"
    r = b.md.Modularity(0.05, got[0], got[1], got[3][0], got[3][1])
    m = got[3][0]
    newman = sum(Fraction(i, m) - Fraction(2 * i + o, 2 * m) ** 2 for i, o in zip(internal, boundary))
    assert abs(Fraction(r.q) - newman) <= Fraction(K * 8, 2 ** 53), "q is not Newman's modularity of the partition"
    print("cross ok: q = %.6f" % r.q, flush=True)


def planted_group():
    """hostlib's planted graph and cover at N = 10^4, pi set to the planted memberships: q > 0 and equal to the statement;
    against the unquantised rationals within the derived bound"""
    from mcmc_ammsb_gpu_amd import hostlib
    b = Bench()
    N, K = 10_000, 32
    keys = np.ascontiguousarray(hostlib.generate_graph(N, K, 32, seed=20260101), dtype=np.uint64)
    offsets, mem = hostlib.generate_cover(N, K, seed=20260101)
    M = np.zeros((N, K), dtype=bool)
    for k in range(K):
        M[mem[int(offsets[k]):int(offsets[k + 1])], k] = True
    O = M.sum(axis=1)
    assert 1 <= O.min() and O.max() <= 3 and keys.size > 100_000
    host = np.where(M, (1.0 / O)[:, None], 0.0).astype(F32)
    got, _ = b.against(host, 0.05, keys, "planted")
    api = b.api.run(b.matrix(host), 0.05, keys)
    assert b.md.wide(api[0].cpu().numpy()).tolist() == got[0].tolist() and b.md.wide(api[1].cpu().numpy()).tolist() == got[1].tolist()
    assert api[2].cpu().numpy().tolist() == got[3] and np.array_equal(api[3].cpu().numpy().view(np.uint32), got[2])
    m = got[3][0]
    r = b.md.Modularity(0.05, got[0], got[1], m, got[3][1])
    IN, SV, deg, _, _ = statement(M, keys)
    want = b.md.Modularity(0.05, IN, SV, m, 0)
    assert r.q_each.tobytes() == want.q_each.tobytes() and r.q == want.q, "the host formula over equal integers differs"
    assert r.q > 0, r.q
    # the unquantised EQ: per community the terms 1 / P and deg / O summed as counts per denominator
    a, bb = ends_of(keys)
    for k in range(K):
        both = M[a, k] & M[bb, k]
        P = (O[a] * O[bb])[both]
        i = sum(Fraction(int(c), int(p)) for p, c in zip(*np.unique(P, return_counts=True)))
        s = sum(Fraction(int(deg[M[:, k] & (O == o)].sum()), int(o)) for o in (1, 2, 3))
        exact = (2 * i - s * s / (2 * m)) / (2 * m)
        bound = Fraction(8, 2 ** 53) * (2 * Fraction(r.in_each[k]) + Fraction(r.s_each[k]) ** 2 / (2 * m)) / (2 * m) + \
            Fraction(1, 2 ** 36) * abs(Fraction(r.q_each[k]))
        delta = abs(Fraction(r.q_each[k]) - exact)
        assert delta <= bound, "community %d: |dq| = %g above the bound %g" % (k, float(delta), float(bound))
    print("planted ok: q = %.6f over %d links" % (r.q, m), flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _modularity
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    seen = []

    def calls(a):
        seen.append((a.Modularity(degree=True), a.pi.host().copy(), a.TrainingLinks().cpu().numpy().view(np.uint64).copy()))
    ps.unperturbed_run(make, calls, "modularity")
    r, host, keys = seen[0]
    assert isinstance(r, _modularity.Modularity) and r.N == N and host.shape == (N, K) and keys.size > 100_000
    IN, SV, deg, valid, skipped = statement(members(host, 0.05), keys)
    assert r.internal.tolist() == IN and r.volume.tolist() == SV and np.array_equal(r.degree, deg)
    assert (r.links, r.skipped) == (valid, skipped) == (keys.size, 0)
    want = _modularity.Modularity(0.05, IN, SV, valid, skipped)
    assert r.q_each.tobytes() == want.q_each.tobytes() and r.q == want.q
    lrn = make()
    lrn.Run(5)
    sub = keys[::7].copy()
    sub[::50] |= np.uint64(0xFFFFFFFF)
    r = lrn.Modularity(0.1, edges=sub)
    IN, SV, deg, valid, skipped = statement(members(lrn.pi.host(), 0.1), sub)
    assert r.internal.tolist() == IN and r.volume.tolist() == SV and (r.links, r.skipped) == (valid, skipped) and r.degree is None
    assert skipped == sub[::50].size
    ps.rejects(AmmsbError, (lambda: lrn.Modularity(-1.0), lambda: lrn.Modularity(float("nan"))))
    lrn.close()
    print("learner ok graph=%s: q = %.6f" % (graph, want.q), flush=True)


def _check_file(path, ckpt, lc, K, thr, what):
    """a modularity file equals, byte for byte, write_modularity of the statement over the pi of the checkpoint and the
    training links of the link-communities file the same process wrote"""
    from mcmc_ammsb_gpu_amd import _linkcomm, _modularity
    fN, r = _modularity.read_modularity(path)
    assert r.internal.size == K and F32(r.threshold) == F32(thr), what
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    keys = np.ascontiguousarray(_linkcomm.read_link_communities(lc)[4], dtype=np.uint64)
    IN, SV, _, valid, skipped = statement(members(pi, thr), keys)
    assert keys.size > 1000 and (valid, skipped) == (keys.size, 0), what
    want = _modularity.Modularity(thr, IN, SV, valid, skipped, N=fN)
    again = path + ".py"
    _modularity.write_modularity(again, fN, want)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the file is not write_modularity of the statement" % what
    return fN, r


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("modularity_test", d, 300)
        fN, r = _check_file(os.path.join(d, "modularity.txt"), os.path.join(d, "cpp.ckpt"), os.path.join(d, "links.txt"), 64, 0.05,
                            "modularity_test")
        assert fN == 20000
        print("cpp ok: Learner::WriteModularity equals the statement over the checkpoint's pi, q = %.6f" % r.q, flush=True)
        # the command-line driver on a small generated graph; the links from the link-communities file of the same run
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck, lc = os.path.join(d, "r.txt"), os.path.join(d, "main.ckpt"), os.path.join(d, "lc.txt")
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--checkpoint-out", ck, "--link-communities-out", lc]
        for extra, thr in (([], 0.05), (["--modularity-threshold", "0.02"], 0.02)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--modularity-out", out] + extra, 240)
            fN, r = _check_file(out, ck, lc, 48, thr, "ammsb_main thr=%g" % thr)
            assert fN == N
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "carry": lambda a: carry_group(),
    "cut": lambda a: cut_group(),
    "cross": lambda a: cross_group(),
    "planted": lambda a: planted_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
