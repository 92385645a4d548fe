"""Child process of test_gpu_omega.py (one per group): the node-pair pass of the Omega index (include/ammsb_omega.h,
ops.CoverOmega, Learner.CoverOmega) against the numpy statement of the header's definitions:

    MD = pi[U] >= np.float32(thr);  SD = MD.astype(np.int32) @ MD.T.astype(np.int32), ST likewise from the truth
    iu = np.triu_indices(n, 1);  bincounts of SD[iu], ST[iu] and SD[iu][SD[iu] == ST[iu]]

Only integer adds are involved on both sides, so every count must be equal: there is no tolerance anywhere below."""
import io
import os
import sys

import numpy as np

import postfit_support as ps

NONE = 0xFFFFFFFF
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
SEEN = set()
F32 = np.float32
TILE = 128


def statement(pi, thr, off, mem, U, L=None):
    """-> dict(agree, detected, truth [L] int64, clipped, skipped, outside, L) from the host pi [N, K]"""
    N, n, G = pi.shape[0], int(U.size), int(off.size) - 1
    MD = pi[U.astype(np.int64)] >= F32(thr)
    pos = np.full(N, -1, np.int64)
    pos[U.astype(np.int64)] = np.arange(n)
    MT = np.zeros((n, max(G, 1)), dtype=bool)
    m64 = mem.astype(np.int64)
    comm = np.repeat(np.arange(G, dtype=np.int64), np.diff(off.astype(np.int64)))
    valid = m64 < N
    skipped = int((~valid).sum())
    inside = valid.copy()
    inside[valid] = pos[m64[valid]] >= 0
    outside = int(valid.sum() - inside.sum())
    MT[pos[m64[inside]], comm[inside]] = True
    SD = MD.astype(np.int32) @ MD.T.astype(np.int32)
    ST = MT.astype(np.int32) @ MT.T.astype(np.int32)
    iu = np.triu_indices(n, 1)
    sd, st = SD[iu].astype(np.int64), ST[iu].astype(np.int64)
    need = 1 + max(int(MD.sum(1).max()) if n else 0, int(MT.sum(1).max()) if n else 0)
    L = need if L is None else L
    keep = (sd < L) & (st < L)
    return dict(agree=np.bincount(sd[keep & (sd == st)], minlength=L), detected=np.bincount(sd[keep], minlength=L),
                truth=np.bincount(st[keep], minlength=L), clipped=int((~keep).sum()), skipped=skipped, outside=outside,
                L=L, need=need, dcount=MD.sum(1), tcount=MT.sum(1))


def check(got, ref, what):
    for name in ("agree", "detected", "truth"):
        assert np.array_equal(got[name], ref[name]), "%s: %s differs\n%s\n%s" % (what, name, got[name][:12], ref[name][:12])
    for name in ("clipped", "skipped", "outside"):
        assert got[name] == ref[name], "%s: %s %d, the statement has %d" % (what, name, got[name], ref[name])


def same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("agree", "detected", "truth")) and \
        all(a[k] == b[k] for k in ("clipped", "skipped", "outside"))


def tiles_of(n):
    R = (n + TILE - 1) // TILE
    return R * (R + 1) // 2


def cuttings(total):
    cuts = sorted({0, total // 3, (2 * total) // 3 + (1 if total > 4 else 0), total})
    return {"whole": [(0, total)], "tiles": [(t, 1) for t in range(total)],
            "ragged": [(a, b - a) for a, b in zip(cuts[:-1], cuts[1:])]}


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _omega
        super().__init__()
        self.om = _omega
        self.lib = _omega.load()
        self.api = self.ops.CoverOmega(self.ctx)

    def run(self, pi, thr, off, mem, U, cuts, L=None, identity=False):
        """the three library calls over buffers of this test's own, each followed by GUARD words that must survive"""
        import ctypes as C
        T = self.torch
        N, K, G, M, n = int(pi.desc.num_rows), int(pi.cols), int(off.size) - 1, int(mem.size), int(U.size)
        WD, WT = (K + 31) // 32, (G + 31) // 32
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
        position = np.full(N, -1, np.int32)
        position[U.astype(np.int64)] = np.arange(n, dtype=np.int32)
        d_nodes = None if identity or n == 0 else self.ctx.from_numpy(U.astype(np.uint32))
        d_off, d_pos = self.ctx.from_numpy(off.astype(np.uint64)), self.ctx.from_numpy(position)
        d_mem = self.ctx.from_numpy(mem.astype(np.uint32)) if M else None
        dbits, dcount = self.guarded(n * WD, T.int32, FILL32), self.guarded(n, T.int32, FILL32)
        tbits, tcount = self.guarded(n * WT, T.int32, FILL32, zero=True), self.guarded(n, T.int32, FILL32, zero=True)
        tally = self.guarded(2, T.int64, FILL64, zero=True)
        self.om.check(self.lib.ammsb_omega_detected_bits(C.byref(pi.desc), float(F32(thr)), ptr(d_nodes), n, ptr(dbits),
                                                         ptr(dcount), None))
        if n:
            SEEN.add(self.om.last_kernel_name())
        self.om.check(self.lib.ammsb_omega_truth_bits(ptr(d_off), G, ptr(d_mem), M, N, ptr(d_pos), n, ptr(tbits),
                                                      ptr(tcount), ptr(tally), C.c_void_p(tally.data_ptr() + 8), None))
        if n and G:
            SEEN.add(self.om.last_kernel_name())
            if M:
                # launched before the count, whose name is the one the call leaves: that the scatter ran is shown by
                # the bits it set (tcount and the truth histogram below), not by a name the library reported
                SEEN.add("omega_truth_scatter")
        T.cuda.synchronize()
        dc, tc = dcount.cpu().numpy(), tcount.cpu().numpy()
        need = 1 + (max(int(dc[:n].max()), int(tc[:n].max())) if n else 0)
        L = need if L is None else L
        hist = self.guarded(3 * L + 1, T.int64, FILL64, zero=True)
        for t0, cnt in cuts:
            self.om.check(self.lib.ammsb_omega_pairs(ptr(dbits), K, ptr(tbits), G, n, L, t0, cnt, ptr(hist), None))
            if n and cnt:
                SEEN.add(self.om.last_kernel_name())
        T.cuda.synchronize()
        for name, buf, words, fill in (("dbits", dbits, n * WD, FILL32), ("dcount", dcount, n, FILL32),
                                       ("tbits", tbits, n * WT, FILL32), ("tcount", tcount, n, FILL32),
                                       ("tally", tally, 2, FILL64), ("hist", hist, 3 * L + 1, FILL64)):
            assert (buf.cpu().numpy()[words:] == fill).all(), "the words past %s were written" % name
        h, tl = hist.cpu().numpy(), tally.cpu().numpy()
        return dict(agree=h[:L].copy(), detected=h[L:2 * L].copy(), truth=h[2 * L:3 * L].copy(), clipped=int(h[3 * L]),
                    skipped=int(tl[0]), outside=int(tl[1]), L=L, need=need, dcount=dc[:n].copy(), tcount=tc[:n].copy())

    def everything(self, host, thr, off, mem, U, what, pi=None):
        """every cutting against the statement, bit-equal to each other and to a second call; L one below the need"""
        pi = self.matrix(host) if pi is None else pi
        ref = statement(host, thr, off, mem, U)
        n, first = int(U.size), None
        for name, cuts in cuttings(tiles_of(n)).items():
            got = self.run(pi, thr, off, mem, U, cuts)
            assert got["L"] == ref["L"], (what, got["L"], ref["L"])
            assert np.array_equal(got["dcount"], ref["dcount"]) and np.array_equal(got["tcount"], ref["tcount"]), what
            check(got, ref, "%s cut=%s" % (what, name))
            P = n * (n - 1) // 2
            assert int(got["detected"].sum()) == int(got["truth"].sum()) == P and got["clipped"] == 0, what
            if first is None:
                first = got
                assert same(first, self.run(pi, thr, off, mem, U, cuts)), what + ": two calls differ"
            else:
                assert same(first, got), "%s: cut=%s differs from the whole triangle" % (what, name)
        if ref["L"] >= 2:
            low = statement(host, thr, off, mem, U, L=ref["L"] - 1)
            got = self.run(pi, thr, off, mem, U, [(0, tiles_of(n))], L=ref["L"] - 1)
            check(got, low, what + ": L one below the need")
            assert got["clipped"] == low["clipped"], what
        return first


def random_pi(rng, N, K, thr):
    """about K^-1/2 of the entries at or above thr; NaNs and values equal to thr planted"""
    host = (rng.random((N, K)) * 0.9 * thr).astype(F32)
    above = rng.random((N, K)) < K ** -0.5
    host[above] = (thr + rng.random(int(above.sum())) * (1 - thr)).astype(F32)
    flat = host.reshape(-1)
    spots = rng.choice(flat.size, min(flat.size, max(2, flat.size // 50)), replace=False)
    flat[spots[::2]] = np.nan
    flat[spots[1::2]] = F32(thr)
    return host


def random_cover(rng, N, G, most=90):
    """communities of 0 .. most distinct members; a member == N and a member == 2^32 - 1 where the sizes allow it"""
    sizes = rng.integers(0, min(N, most) + 1, G)
    lists = [rng.choice(N, int(sz), replace=False).astype(np.uint32) for sz in sizes]
    big = [i for i, c in enumerate(lists) if c.size >= 3]
    if big:
        lists[big[0]][1] = N
        lists[big[-1]][-1] = NONE
    offsets = np.zeros(G + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([c.size for c in lists])
    return offsets, np.concatenate(lists).astype(np.uint32) if lists else np.zeros(0, np.uint32)


def universe_of(kind, rng, N, mem):
    if kind == "all":
        return np.arange(N, dtype=np.uint32)
    if kind == "covered":
        return np.unique(mem[mem < N]).astype(np.uint32)
    return np.sort(rng.choice(N, int(kind), replace=False)).astype(np.uint32)   # a ragged list of that many nodes


# (N, K, G, universe): every n of {1, 2, 63, 64, 65, 129, 300} and 257 (just past two tiles of 128), every K and every G
EXACT = ((1, 1, 1, "all"), (2, 31, 7, "all"), (63, 32, 33, "all"), (64, 33, 1, "all"), (65, 65, 300, "all"),
         (129, 260, 7, "all"), (300, 8192, 33, "all"), (300, 1028, 5000, "all"), (257, 1024, 33, "all"),
         (400, 65, 300, "covered"), (900, 260, 33, 129), (700, 1024, 7, 300))


def exact_group(which):
    b = Bench()
    rng = np.random.default_rng(11)
    for i, (N, K, G, kind) in enumerate(EXACT):
        if which and i not in which:
            continue
        thr = 0.05
        host = random_pi(rng, N, K, thr)
        off, mem = random_cover(rng, N, G)
        U = universe_of(kind, rng, N, mem)
        got = b.everything(host, thr, off, mem, U, "N=%d K=%d G=%d universe=%s" % (N, K, G, kind))
        print("exact N=%d K=%d G=%d n=%d L=%d skipped=%d outside=%d" % (N, K, G, U.size, got["L"], got["skipped"],
                                                                         got["outside"]), flush=True)
    print("exact ok", flush=True)


def planted_group():
    from mcmc_ammsb_gpu_amd import _omega
    b = Bench()
    rng = np.random.default_rng(5)

    def omega_of(host, thr, off, mem, U, what):
        got = b.everything(host, thr, off, mem, U, what)
        return _omega.Omega(thr, U.size, got["agree"], got["detected"], got["truth"], got["skipped"], got["outside"]), got

    # truth == the detected cover under a column permutation
    N, K = 300, 33
    host = random_pi(rng, N, K, 0.05)
    perm = rng.permutation(K)
    member = host >= F32(0.05)
    lists = [np.flatnonzero(member[:, perm[g]]) for g in range(K)]
    off = np.zeros(K + 1, np.uint64)
    off[1:] = np.cumsum([c.size for c in lists])
    r, _ = omega_of(host, 0.05, off, np.concatenate(lists).astype(np.uint32), np.arange(N, dtype=np.uint32), "permuted")
    assert r.omega == 1.0 and r.omega_unadjusted == 1.0, r
    # n = 4, D = {{0, 1}, {2, 3}}, T = {{0, 1, 2, 3}}
    host = np.zeros((4, 2), F32)
    host[:2, 0] = host[2:, 1] = 1
    r, got = omega_of(host, 0.5, np.array([0, 4], np.uint64), np.arange(4, dtype=np.uint32), np.arange(4, dtype=np.uint32), "n=4")
    assert got["detected"].tolist() == [4, 2] and got["truth"].tolist() == [0, 6] and got["agree"].tolist() == [0, 2]
    assert r.omega == 0.0, r
    # a pair of nodes that shares 2 communities in both covers
    host = np.zeros((5, 3), F32)
    host[0, :2] = host[1, :2] = host[2, 2] = 1
    off, mem = np.array([0, 2, 4, 5], np.uint64), np.array([0, 1, 1, 0, 3], np.uint32)
    r, got = omega_of(host, 0.5, off, mem, np.arange(5, dtype=np.uint32), "two shared")
    assert got["agree"].tolist() == [9, 0, 1] and got["detected"].tolist() == [9, 0, 1] and r.omega == 1.0
    # thr = 0 (every node in every community) and thr above every value
    N, K, G = 130, 65, 7
    host = np.nan_to_num(random_pi(rng, N, K, 0.05))
    off, mem = random_cover(rng, N, G)
    U = np.arange(N, dtype=np.uint32)
    r, got = omega_of(host, 0.0, off, mem, U, "thr=0")
    assert got["L"] == K + 1 and got["detected"][K] == N * (N - 1) // 2
    r, got = omega_of(host, 2.0, off, mem, U, "thr above every value")
    assert got["detected"][0] == N * (N - 1) // 2
    # a truth whose members are all skipped: every pair at level 0 in the truth; with no detected member either, NaN
    r, got = omega_of(host, 2.0, np.array([0, 2, 3], np.uint64), np.array([N, NONE, N + 5], np.uint32), U, "all skipped")
    assert got["skipped"] == 3 and got["L"] == 1 and r.omega != r.omega and r.omega_unadjusted == 1.0
    print("planted ok", flush=True)


def forms_group():
    """every kernel form is named and reached, on both sides of its dispatch boundary, and a misaligned pi takes the
    generic form and gives the same counts"""
    b = Bench()
    rng = np.random.default_rng(9)
    off, mem = random_cover(rng, 200, 33)
    U = np.sort(rng.choice(200, 150, replace=False)).astype(np.uint32)
    for K, form in ((256, "omega_bits_fast"), (255, "omega_bits_generic"), (257, "omega_bits_generic"),
                    (512, "omega_bits_fast"), (8192, "omega_bits_fast"), (260, "omega_bits_generic")):
        host = random_pi(rng, 200, K, 0.05)
        pi = b.matrix(host)
        ref = statement(host, 0.05, off, mem, U)
        got = b.run(pi, 0.05, off, mem, U, [(0, tiles_of(150))])
        check(got, ref, "forms K=%d" % K)
        bits, _ = b.api.detected_bits(pi, 0.05, nodes=b.ctx.from_numpy(U))
        assert b.api.kernel_name() == form, (K, b.api.kernel_name())
        if K % 256 == 0:
            mis = b.misaligned(host)
            again = b.run(mis, 0.05, off, mem, U, [(0, tiles_of(150))])
            assert same(got, again), "K=%d: the misaligned base gives other counts" % K
            mbits, _ = b.api.detected_bits(mis, 0.05, nodes=b.ctx.from_numpy(U))
            assert b.api.kernel_name() == "omega_bits_generic"
            assert b.torch.equal(bits, mbits), "K=%d: the two forms write other words" % K
        # the identity universe: nodes == NULL
        full = np.arange(200, dtype=np.uint32)
        check(b.run(pi, 0.05, off, mem, full, [(0, tiles_of(200))], identity=True), statement(host, 0.05, off, mem, full),
              "forms K=%d identity" % K)
    assert SEEN == set(b.om.KERNEL_FORMS), SEEN ^ set(b.om.KERNEL_FORMS)
    print("forms ok", flush=True)


def big_cover(rng, G=36):
    """G communities over the rows of postfit_support's big fixture, in global numbering: 5 to 60 planted rows each, a
    third of them with rows >= 2^19 only or with rows of the first window only; into the first ones go members >= N (N
    itself, a little past it, 2^32 - 1), which are skipped, and zero rows, which are valid and outside the universe"""
    ids = ps.big_ids()
    pools = (ids, ids[ids >= (1 << 19)], ids[:128])
    lists = [rng.choice(pools[g % 3], int(rng.integers(5, 61)), replace=False).astype(np.uint32) for g in range(G)]
    past = (ps.BIG_ROWS, ps.BIG_ROWS + 5, NONE)
    for j, z in enumerate(ps.BIG_ZERO_ROWS):
        lists[j] = np.concatenate([lists[j], np.array([z, past[j % 3]], dtype=np.uint32)])
        lists[j + 7] = np.concatenate([np.array([past[(j + 1) % 3], z], dtype=np.uint32), lists[j + 7]])
    offsets = np.zeros(G + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([c.size for c in lists])
    return offsets, np.concatenate(lists).astype(np.uint32)


def big_group():
    """pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, zero but 640 planted rows
    in four windows): the detected bits of the 640 planted rows as the universe, and of the last window alone, in the
    16-byte form and, from a base 4 bytes past a 16-byte boundary, in the generic form; then the truth bits and the pair
    pass against a ground truth over the planted rows with members >= N and members in zero rows.  The statement is
    evaluated over the planted rows and the zero rows, the members remapped.  omega_truth_* and omega_pairs read no pi:
    they are checked here on what the detected bits gave them."""
    b = Bench()
    n, K = ps.BIG_ROWS, ps.BIG_K
    pi, compact, ids = b.big_pi(63)
    thr = ps.big_threshold(compact)
    off, mem = big_cover(np.random.default_rng(73))
    local = ps.big_positions(mem).astype(np.uint32)
    universes = {"planted": ids.astype(np.uint32), "last window": ids[ids >= (1 << 19) - 128].astype(np.uint32)}
    ext = ps.big_extended(compact)
    refs, words = {}, {}                        # (words: what the bit words of two rows must share)
    wext = ps.big_extended(ps.big_wrapped(compact))
    for name, U in universes.items():
        pos = ps.big_positions(U).astype(np.uint32)
        refs[name] = statement(ext, thr, off, local, pos)
        MD = (ext[pos] >= F32(thr)).astype(F32)
        words[name] = MD @ MD.T                    # shared communities of every two positions (exact: below 2^24)
        # a kernel that keeps row * K in 32 bits would give the wrapped figures: each of them that reads pi differs
        # from the true ones (the truth histogram, skipped and outside are counted from the ground truth alone)
        wrap = statement(wext, thr, off, local, pos)
        WD = (wext[pos] >= F32(thr)).astype(F32)
        assert not np.array_equal(words[name], WD @ WD.T)
        assert not np.array_equal(refs[name]["dcount"], wrap["dcount"])
        assert not np.array_equal(refs[name]["detected"], wrap["detected"]) and not np.array_equal(refs[name]["agree"], wrap["agree"])
        assert refs[name]["skipped"] == 8 and refs[name]["outside"] >= 8 and refs[name]["truth"][1:].sum() > 0
    print("big: the wrapped-offset reference differs in the communities two rows share, the counts per node and the "
          "detected and agree histograms, for both universes", flush=True)

    def run(pi, form):
        out = {}
        for name, U in universes.items():
            got = b.run(pi, thr, off, mem, U, [(0, tiles_of(U.size))])
            assert form in SEEN and "omega_pairs" in SEEN, SEEN
            ref = refs[name]
            assert got["L"] == ref["L"], (name, got["L"], ref["L"])
            assert np.array_equal(got["dcount"], ref["dcount"]) and np.array_equal(got["tcount"], ref["tcount"]), name
            check(got, ref, "%s universe=%s" % (form, name))
            bits, counts = b.api.detected_bits(pi, thr, nodes=b.ctx.from_numpy(U))
            assert b.api.kernel_name() == form, b.api.kernel_name()
            # which bit stands for which community is private to the library: the bits are held to what any placement
            # must give, the members per row and the communities shared by every two rows
            B = np.unpackbits(bits.cpu().numpy().view(np.uint8), axis=1).astype(F32)
            assert B.shape == (U.size, K) and np.array_equal(B.sum(1), ref["dcount"]), "%s universe=%s: set bits per row" % (form, name)
            assert np.array_equal(B @ B.T, words[name]), "%s universe=%s: the bits two rows share differ" % (form, name)
            assert np.array_equal(counts.cpu().numpy(), ref["dcount"])
            out[name] = (got, bits)
        return out

    first = run(pi, "omega_bits_fast")
    del pi
    b.release()
    SEEN.clear()
    mis, again, _ = b.big_pi(63, misaligned=True)
    assert np.array_equal(again, compact)
    second = run(mis, "omega_bits_generic")
    for name in universes:
        assert same(first[name][0], second[name][0]) and b.torch.equal(first[name][1], second[name][1]), \
            "universe=%s: the two forms differ" % name
    r = refs["planted"]
    print("big ok: %d x %d, thr %.3g, L %d, skipped %d, outside %d" % (n, K, thr, r["L"], r["skipped"], r["outside"]), flush=True)


def persistent_group():
    """n = 3000 is 300 tiles, run also as one launch per 7 tiles; n = 4200 is 561 tiles, more than the 512 blocks of the
    grid, so that blocks go round the persistent loop"""
    b = Bench()
    rng = np.random.default_rng(21)
    for N, K, G in ((3000, 64, 64), (4200, 32, 32)):
        host = random_pi(rng, N, K, 0.05)
        off, mem = random_cover(rng, N, G, most=400)
        U = np.arange(N, dtype=np.uint32)
        ref = statement(host, 0.05, off, mem, U)
        pi = b.matrix(host)
        total = tiles_of(N)
        whole = b.run(pi, 0.05, off, mem, U, [(0, total)])
        check(whole, ref, "persistent n=%d" % N)
        assert same(whole, b.run(pi, 0.05, off, mem, U, [(t, min(7, total - t)) for t in range(0, total, 7)]))
    print("persistent ok", flush=True)


def _check_omega(r, host, thr, off, mem, U, what):
    ref = statement(host, thr, off, mem, U)
    got = dict(agree=r.agree, detected=r.detected, truth=r.truth, clipped=0, skipped=r.skipped, outside=r.outside)
    assert r.agree.size == ref["L"] and r.nodes == U.size and r.pairs == U.size * (U.size - 1) // 2, what
    check(got, ref, what)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _omega, hostlib
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, m, n, deg, k_true = ps.WORKLOADS["C1"]
    ds, make = ps.c1_learner(graph)
    off, mem = hostlib.generate_cover(N, k_true, seed=20260101)
    lrn = make()
    lrn.Run(30)
    ck = io.BytesIO()
    lrn.Serialize(ck)
    host, _ = ps.pi_beta_of_checkpoint(ck.getvalue(), N, K)
    some = np.sort(np.random.default_rng(3).choice(N, 2000, replace=False)).astype(np.uint32)
    # a truth that covers a small share of the nodes: the planted cover of the nodes below 1500
    keep = mem < 1500
    part = np.concatenate([[0], np.cumsum(keep)])[off.astype(np.int64)].astype(np.uint64)
    small = mem[keep]
    for thr in (0.05, 0.01):
        r = lrn.CoverOmega((off, mem), thr, universe=some)
        assert isinstance(r, _omega.Omega)
        _check_omega(r, host, thr, off, mem, some, "learner list thr=%g" % thr)
        cut = lrn.CoverOmega((off, mem), thr, universe=some, launch_pairs=1)
        assert np.array_equal(cut.agree, r.agree) and np.array_equal(cut.detected, r.detected) and cut.omega == r.omega
        c = lrn.CoverOmega((part, small), thr, universe="covered")
        cov = np.unique(small)
        _check_omega(c, host, thr, part, small, cov, "learner covered thr=%g" % thr)
        assert c.outside == 0 and (c.omega, c.omega_unadjusted, c.pairs) == _omega.scores(c.agree, c.detected, c.truth, cov.size)
        print("thr=%g: omega %.4f over 2000 nodes, %.4f over the %d covered" % (thr, r.omega, c.omega, cov.size), flush=True)
    # a ground truth in another id space: every member is >= N, so "covered" is empty; the members are still counted
    wrong = (np.array([0, 3, 3, 5], np.uint64), np.array([N, N + 7, NONE, N + 1, 2 * N], np.uint32))
    r = lrn.CoverOmega(wrong, 0.05, universe="covered")
    assert (r.nodes, r.pairs, r.skipped, r.outside) == (0, 0, 5, 0) and r.omega != r.omega and r.agree.tolist() == [0], r
    r = lrn.CoverOmega(((off, mem)), 0.05, universe=[])       # an empty list: every valid member is outside
    assert (r.nodes, r.skipped, r.outside) == (0, 0, mem.size) and r.detected.tolist() == [0], r
    r = lrn.CoverOmega(wrong, 0.05, universe=some[:300])      # the same counts from the device
    assert (r.nodes, r.skipped, r.outside) == (300, 5, 0) and int(r.truth[0]) == 300 * 299 // 2, r
    refused = ps.rejects(AmmsbError, (lambda: lrn.CoverOmega((off, mem), -1.0), lambda: lrn.CoverOmega((off, mem), universe=[5, 4]),
                                      lambda: lrn.CoverOmega((off, mem), universe=[1, N]),
                                      lambda: lrn.CoverOmega((off, mem), universe="all", max_bytes=1000)))
    refused += ps.rejects(ValueError, (lambda: lrn.CoverOmega([[1, 2, 1]]),))
    assert len(refused) == 5 and all("max_bytes" not in str(e) or 'universe="covered"' in str(e) for e in refused)
    lrn.close()
    # Run(20), the call, Run(20) leaves the state Run(40) leaves

    def calls(a):
        a.CoverOmega((off, mem), universe=some)
    ps.unperturbed_run(make, calls, "cover omega")
    print("learner ok graph=%s" % graph, flush=True)


def _check_omega_file(path, ckpt, K, thr, offsets, members, kind, what):
    """a cover-Omega file against the statement over the pi of the checkpoint the same process wrote; the Python writer
    reproduces its bytes, the scores in the header line included"""
    from mcmc_ammsb_gpu_amd import _omega
    fN, r, printed = _omega.read_cover_omega(path)
    assert r.K == K and F32(r.threshold) == F32(thr) and r.G == offsets.size - 1, (r.K, r.G, r.threshold)
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    U = _omega.check_universe(kind, fN, members)
    _check_omega(r, pi, thr, offsets, members, U, what)
    same_float = lambda a, b: a == b or (a != a and b != b)   # noqa: E731
    assert same_float(printed[0], r.omega) and same_float(printed[1], r.omega_unadjusted), (what, printed, r)
    again = path + ".py"
    _omega.write_cover_omega(again, fN, r)
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the Python writer's bytes differ" % what
    return fN, r


def cpp_group():
    import tempfile
    from cover_child import _check_match_file
    from nmi_child import _check_nmi_file
    from mcmc_ammsb_gpu_amd import _cover, hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("omega_test", d, 240)
        lists = [[int(w) for w in ln.split()[1:]] for ln in open(os.path.join(d, "truth.txt"))]
        offsets, members = _cover.check_cover(lists)
        fN, res = _check_omega_file(os.path.join(d, "omega.txt"), os.path.join(d, "cpp.ckpt"), 64, 0.05, offsets, members,
                                    "covered", "omega_test")
        assert fN == 20000 and res.skipped == 2 and res.outside == 0
        print("cpp ok: Learner::WriteCoverOmega equals the statement over the checkpoint's pi", flush=True)
        # the command-line driver on a data-set dump: the ground truth covers the first 900 of 3000 nodes
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        toff, tmem = hostlib.generate_cover(N, 8, seed=3)
        keep = tmem < 900
        toff = np.concatenate([[0], np.cumsum(keep)])[toff.astype(np.int64)].astype(np.uint64)
        tmem = tmem[keep]
        truth, out, ck = os.path.join(d, "truth.cmty"), os.path.join(d, "o.txt"), os.path.join(d, "main.ckpt")
        mout, nout = os.path.join(d, "m.txt"), os.path.join(d, "n.txt")
        _cover.write_cover(truth, toff, tmem)
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--ground-truth", truth, "--checkpoint-out", ck]
        for extra, thr, kind in ((["--cover-omega-out", out], 0.05, "covered"),
                                 (["--cover-omega-out", out, "--cover-omega-universe", "all", "--cover-match-threshold",
                                   "0.01"], 0.01, "all")):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + extra, 240)
            fN, res = _check_omega_file(out, ck, 48, thr, toff, tmem, kind, "ammsb_main dump universe=%s" % kind)
            assert fN == N and res.nodes == (N if kind == "all" else np.unique(tmem).size) and res.skipped == 0
        # --cover-match-out and --cover-nmi-out alone still work, unchanged
        os.remove(out)
        for flag, path, checker in (("--cover-match-out", mout, _check_match_file), ("--cover-nmi-out", nout, _check_nmi_file)):
            r = ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + [flag, path], 240)
            assert not os.path.exists(out), r.stderr[-3000:]
            checker(path, ck, 48, 0.05, toff, tmem, "ammsb_main dump: %s alone" % flag)
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "planted": lambda a: planted_group(),
    "forms": lambda a: forms_group(),
    "persistent": lambda a: persistent_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
