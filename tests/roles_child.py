"""Child process of test_gpu_roles.py (one per group): the node roles (include/ammsb_roles.h, ops.NodeRoles,
Learner.NodeRoles) against the integer statement of the header's definitions, written once here, in numpy over Python
integers:

    M = pi >= np.float32(thr)
    for each a:  R = the valid targets of row a;   c = M[R].sum(0)
    degree = |R|, own = M[a].sum(), embedded = (M[R] & M[a]).any(1).sum(), reached = (c > 0).sum(), votes = c.sum(),
    squares = (c.astype(object) ** 2).sum() mod 2^64
    slots: a stable argsort of -c over the candidates in ascending k;   ksum / ksq / kmembers: sums of c[a, k], c[a, k]^2, 1
    over the nodes a of k

Every device integer is asserted equal to the statement; the float64 fields, one host formula over equal integers, are
bit-equal.  There is no tolerance in this file."""
import os
import sys

import numpy as np

import postfit_support as ps
from modularity_child import random_pi

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
F32 = np.float32
# the kernel's constants (csrc/ammsb_roles.hip, csrc/ammsb_postfit.h)
W1_WAVES, W2_WAVES, MAX_GRID = 4, 2, 2048
NODE32, NODE64, SUMS = ("degree", "own", "embedded", "reached"), ("votes", "squares"), ("ksum", "ksq", "kmembers")
# (among, top, min_count): both ways, top 1, 4 and 16 and no selection, min_count 0 and 3
HOWS = (("all", 4, 0), ("own", 16, 3), ("all", 1, 3), ("own", 4, 0), ("all", 16, 0), ("all", 0, 0))


def members(pi, thr):
    return pi >= F32(thr)


def statement(M, off, tgt, hows, first=0, count=None):
    """-> (base, slots): base has the per-node arrays of the nodes first .. first + count - 1, the K-sized sums over them
    as lists of Python ints and counts = [valid, skipped]; slots[i] = (home, hcount, hflags) for hows[i]"""
    N, K = M.shape
    count = N - first if count is None else count
    base = {n: np.zeros(count, np.uint32) for n in NODE32}
    base.update({n: np.zeros(count, np.uint64) for n in NODE64})
    ksum, ksq, kmembers, valid, skipped = [0] * K, [0] * K, [0] * K, 0, 0
    slots = [(np.full((count, top), -1, np.int32), np.zeros((count, top), np.uint32), np.zeros(count, np.uint32))
             for _, top, _ in hows]
    for i in range(count):
        a = first + i
        R = tgt[int(off[a]):int(off[a + 1])].astype(np.int64)
        ok = R < N
        R = R[ok]
        valid += int(ok.sum())
        skipped += int((~ok).sum())
        c = M[R].sum(0).astype(np.int64)
        sq = (c.astype(object) ** 2) if R.size else np.zeros(K, dtype=object)
        base["degree"][i], base["own"][i] = R.size, M[a].sum()
        base["embedded"][i] = (M[R] & M[a]).any(1).sum()
        base["reached"][i] = (c > 0).sum()
        base["votes"][i] = int(c.sum())
        base["squares"][i] = int(sq.sum()) % 2 ** 64
        for k in np.flatnonzero(M[a]).tolist():
            ksum[k] += int(c[k])
            ksq[k] += int(sq[k])
            kmembers[k] += 1
        for (among, top, min_count), (home, hcount, hflags) in zip(hows, slots):
            cand = np.flatnonzero(M[a] & (c >= min_count) if among == "own" else c >= max(1, min_count))
            cand = cand[np.argsort(-c[cand], kind="stable")][:top]
            home[i, :cand.size], hcount[i, :cand.size] = cand, c[cand]
            hflags[i] = sum(int(M[a, k]) << j for j, k in enumerate(cand.tolist()))
    base.update(ksum=ksum, ksq=ksq, kmembers=kmembers, counts=[valid, skipped])
    return base, slots


def symmetric_csr(keys, N):
    """keys (a << 32) | b -> (offsets, targets, keys with an end >= N): b in a's row and a in b's row per valid key"""
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N)
    src, dst = np.concatenate((a[ok], b[ok])), np.concatenate((b[ok], a[ok]))
    order = np.argsort(src, kind="stable")
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=N))
    return off, dst[order].astype(np.uint32), int((~ok).sum())


def adjacency(rng, N, lengths, lead=11):
    """rows of the given lengths over N nodes with `lead` targets in front of row 0 (offsets[0] > 0): uniform targets (so a
    long row repeats some), about a twentieth each b == a and targets >= N (N itself, a little past it, 2^32 - 1)"""
    lengths = np.asarray(lengths, dtype=np.int64)
    off = np.zeros(N + 1, np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum(lengths)
    total = int(lengths.sum())
    tgt = rng.integers(0, N, lead + total).astype(np.uint32)
    row = np.repeat(np.arange(N), lengths)
    own = rng.random(total) < 0.05
    tgt[lead:][own] = row[own]
    bad = rng.random(total) < 0.05
    tgt[lead:][bad] = rng.choice(np.array([N, N + 5, 2 ** 32 - 1], dtype=np.uint32), int(bad.sum()))
    return off, tgt


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _roles
        super().__init__()
        self.rl = _roles
        self.lib = _roles.load()
        self.api = self.ops.NodeRoles(self.ctx)
        self.links = self.ops.CommunityLinks(self.ctx)

    def run(self, mask, N, K, off, tgt, how, cuts, what):
        """the call over guarded buffers, the node range in the pieces `cuts` -> name -> host array (per-node arrays whole,
        [N]: what no call handled keeps the fill)"""
        import ctypes as C
        T = self.torch
        among, top, min_count = how
        ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None   # noqa: E731
        buf = {n: self.guarded(N, T.int32, FILL32) for n in NODE32 + ("hflags",)}
        buf.update({n: self.guarded(N, T.int64, FILL64) for n in NODE64})
        buf.update({n: self.guarded(N * top, T.int32, FILL32) for n in ("home", "hcount")})
        buf.update({n: self.guarded(K, T.int64, FILL64, zero=True) for n in SUMS})
        buf["counts"] = self.guarded(2, T.int64, FILL64, zero=True)
        d_off, d_tgt = self.ctx.from_numpy(off), self.ctx.from_numpy(tgt)
        slot = [buf[n] if top else None for n in ("home", "hcount", "hflags")]
        for first, count in cuts:
            self.rl.check(self.lib.ammsb_roles_nodes(
                ptr(mask), N, K, ptr(d_off), ptr(d_tgt), first, count, self.rl.AMONG[among], top, min_count, ptr(buf["degree"]),
                ptr(buf["own"]), ptr(buf["embedded"]), ptr(buf["reached"]), ptr(buf["votes"]), ptr(buf["squares"]),
                ptr(slot[0]), ptr(slot[1]), ptr(slot[2]), ptr(buf["ksum"]), ptr(buf["ksq"]), ptr(buf["kmembers"]),
                ptr(buf["counts"]), None))
            if count:
                want = "roles_nodes_w1" if K <= self.rl.W1_MAX_COLS else "roles_nodes_w2"
                assert self.rl.last_kernel_name() == want, self.rl.last_kernel_name()
        out = {}
        for n, t in buf.items():
            words = {"home": N * top, "hcount": N * top, "counts": 2}.get(n, K if n in SUMS else N)
            host = t.cpu().numpy()
            fill = FILL64 if host.dtype == np.int64 else FILL32
            assert (host[words:].view(np.uint64 if host.dtype == np.int64 else np.uint32) == fill).all(), \
                "%s: the words past %s were written" % (what, n)
            out[n] = host[:words].copy()
        if not top:   # nothing selected, nothing written
            assert (out["hflags"].view(np.uint32) == FILL32).all(), what + ": hflags written with top = 0"
        return out

    def against(self, got, base, slots_of, how, first, count, what):
        top = how[1]
        for n in NODE32:
            assert np.array_equal(got[n][first:first + count].view(np.uint32), base[n]), "%s: %s differs" % (what, n)
        for n in NODE64:
            assert np.array_equal(got[n][first:first + count].view(np.uint64), base[n]), "%s: %s differs" % (what, n)
        for n in SUMS:
            assert got[n].view(np.uint64).tolist() == base[n], "%s: %s differs" % (what, n)
        assert got["counts"].tolist() == base["counts"], "%s: counts %s, not %s" % (what, got["counts"].tolist(), base["counts"])
        if top:
            home, hcount, hflags = slots_of
            assert np.array_equal(got["home"].reshape(-1, top)[first:first + count], home), what + ": home differs"
            assert np.array_equal(got["hcount"].reshape(-1, top)[first:first + count].view(np.uint32), hcount), what + ": hcount differs"
            assert np.array_equal(got["hflags"][first:first + count].view(np.uint32), hflags), what + ": hflags differs"


def same(x, y):
    return all(np.array_equal(x[n], y[n]) for n in x)


def result_of(rl, thr, how, base, slots_of, N, first=0):
    among, top, min_count = how
    return rl.Roles(thr, among, top, min_count, *[base[n] for n in NODE32 + NODE64], *slots_of, base["ksum"], base["ksq"],
                    base["kmembers"], *base["counts"], N=N, first=first)


def same_result(r, want, what):
    for n in NODE32 + NODE64 + SUMS + ("home", "hcount", "hflags"):
        assert np.array_equal(getattr(r, n), getattr(want, n)), "%s: %s differs" % (what, n)
    assert (r.valid, r.skipped, r.first) == (want.valid, want.skipped, want.first), what
    for n in ("embeddedness", "participation", "z"):
        assert getattr(r, n).tobytes() == getattr(want, n).tobytes(), "%s: %s is not bit-equal" % (what, n)
    assert np.array_equal(r.misplaced(), want.misplaced()) and np.array_equal(r.hubs(), want.hubs()) and \
        np.array_equal(r.connectors(), want.connectors()), what


# (N, K): W = 1, 1, 1, 2, 4, 16, 64 and then the two-word form; K = 65 and 4160 have a last word with unused bits
EXACT = ((2000, 1), (2000, 5), (2000, 64), (2000, 65), (2000, 256), (1500, 1024), (600, 4096), (600, 4160), (500, 8192))
HUB = 5000


def exact_group(which):
    b = Bench()
    rng = np.random.default_rng(31)
    for i, (N, K) in enumerate(EXACT):
        host = random_pi(rng, N, K, 0.05, empty=3)   # node 3 has no community
        lengths = rng.integers(0, 8, N)
        lengths[:8] = (0, 1, 63, 64, 65, 2, HUB, 3)     # node 6 is the hub: a row longer than any trip of 64 targets
        off, tgt = adjacency(rng, N, lengths)
        tgt[int(off[7]):int(off[8])] = 3                # every neighbour of node 7 is node 3, which has no community
        assert tgt.size - 11 <= 20000 and N <= 2000
        if which and i not in which:
            continue
        what = "N=%d K=%d" % (N, K)
        M = members(host, 0.05)
        mask = b.links.mask(b.matrix(host), float(F32(0.05)))
        base, slots = statement(M, off, tgt, HOWS)
        assert base["degree"][0] == 0 and base["own"][3] == 0 and base["votes"][7] == 0 and base["degree"][7] == 3
        assert base["counts"][1] > 0 and base["degree"][6] > 4000
        for how, slots_of in zip(HOWS, slots):
            got = b.run(mask, N, K, off, tgt, how, [(0, N)], what)
            b.against(got, base, slots_of, how, 0, N, "%s %s" % (what, how))
            if how == HOWS[0]:
                assert same(got, b.run(mask, N, K, off, tgt, how, [(0, N)], what)), what + ": two runs differ"
                if K % 64:   # garbage in the bits past K of every last word
                    dirty = mask.clone().reshape(N, -1)
                    dirty[:, -1] |= b.ctx.from_numpy(np.array([(~((1 << (K % 64)) - 1)) & (2 ** 64 - 1)], dtype=np.uint64))[0]
                    assert not b.torch.equal(dirty, mask.reshape(N, -1))
                    assert same(got, b.run(dirty.reshape(mask.shape).contiguous(), N, K, off, tgt, how, [(0, N)], what)), \
                        what + ": bits past K changed the result"
        if K == 256:   # equal counts inside one word and across the words of different lanes, both decided by the lower k
            home, hcount, _ = slots[4]
            tie = (hcount[:, :-1] == hcount[:, 1:]) & (home[:, 1:] >= 0)
            assert (tie & (home[:, :-1] >> 6 == home[:, 1:] >> 6)).any() and (tie & (home[:, :-1] >> 6 != home[:, 1:] >> 6)).any()
        print("exact %s: %d valid targets, %d skipped" % (what, base["counts"][0], base["counts"][1]), flush=True)
    if not which or 2 in which:
        # thr = 0: every stored number but a NaN is a member, O = K
        N, K = 300, 64
        host = (rng.random((N, K)) * 0.5).astype(F32)
        off, tgt = adjacency(rng, N, rng.integers(0, 12, N))
        M = members(host, 0.0)
        assert M.all()
        base, slots = statement(M, off, tgt, HOWS[:2])
        mask = b.links.mask(b.matrix(host), 0.0)
        for how, slots_of in zip(HOWS[:2], slots):
            got = b.run(mask, N, K, off, tgt, how, [(0, N)], "thr=0")
            b.against(got, base, slots_of, how, 0, N, "thr=0 %s" % (how,))
        assert (base["own"] == K).all() and np.array_equal(base["votes"], base["degree"].astype(np.uint64) * np.uint64(K))
        # an adjacency without a target, and an empty node range
        off0, tgt0 = np.zeros(N + 1, np.uint64), np.zeros(1, np.uint32)
        base, slots = statement(M, off0, tgt0, HOWS[:1])
        got = b.run(mask, N, K, off0, tgt0, HOWS[0], [(0, N), (N, 0), (5, 0)], "no target")
        b.against(got, base, slots[0], HOWS[0], 0, N, "no target")
        assert got["counts"].tolist() == [0, 0] and (got["home"] == -1).all() and got["kmembers"].tolist() == [N] * K
        print("exact thr=0, no target ok", flush=True)
    print("exact ok", flush=True)


def sparse_pi(rng, N, K, per_node=3):
    host = np.zeros((N, K), F32)
    for _ in range(per_node):
        host[np.arange(N), rng.integers(0, K, N)] = 0.9
    return host


def cut_group():
    """more nodes than one pass of the persistent grid (a wave per node: 2048 blocks of 4 waves below K = 4096, of 2 above), in
    one call and in three ragged ranges: bit-equal, the K-sized sums included"""
    b = Bench()
    rng = np.random.default_rng(37)
    for N, K, waves in ((9000, 64, W1_WAVES), (4300, 4100, W2_WAVES)):
        assert N > MAX_GRID * waves
        host = sparse_pi(rng, N, K)
        off, tgt = adjacency(rng, N, rng.integers(0, 5, N))
        what = "cut N=%d K=%d" % (N, K)
        mask = b.links.mask(b.matrix(host), float(F32(0.05)))
        how = HOWS[0]
        one = b.run(mask, N, K, off, tgt, how, [(0, N)], what)
        c1, c2 = N // 3 - 7, 2 * N // 3 + 5
        three = b.run(mask, N, K, off, tgt, how, [(c2, N - c2), (0, c1), (c1, c2 - c1)], what + " in three")
        assert same(one, three), what + ": three ragged ranges differ from one call"
        base, slots = statement(members(host, 0.05), off, tgt, [how])
        b.against(one, base, slots[0], how, 0, N, what)
        # a range alone: its nodes' entries and the sums over them, nothing outside it
        part = b.run(mask, N, K, off, tgt, how, [(c1, c2 - c1)], what + " middle")
        base, slots = statement(members(host, 0.05), off, tgt, [how], c1, c2 - c1)
        b.against(part, base, slots[0], how, c1, c2 - c1, what + " middle")
        assert (part["degree"][:c1].view(np.uint32) == FILL32).all() and (part["votes"][c2:].view(np.uint64) == FILL64).all()
        print("%s ok" % what, flush=True)
    print("cut ok", flush=True)


def big_group():
    """pi past element 2^32 (postfit_support.big_pi: 2^19 + 128 rows of K = 8192 in one block, zero but 640 planted rows
    in four windows): run() over the adjacency of connect's keys of that fixture (offsets [N + 1], a target only in the
    rows of the planted nodes and of four zero rows; targets >= N among them), with the mask in the 16-byte form and, from
    a base 4 bytes past a 16-byte boundary, in the generic form; a second state filled by two calls that cut the nodes
    128 rows before element 2^32.  The statement is evaluated over the planted rows and the zero rows in compact
    numbering; every other node's entries must be 0 (home: the empty slot).  The form is roles_nodes_w2 at this K;
    roles_nodes_w1 (K <= 4096) reads no pi, it indexes a mask whose largest word offset at this N is below 2^27, and is
    left out."""
    b = Bench()
    T = b.torch
    n, K = ps.BIG_ROWS, ps.BIG_K
    how = ("all", 4, 0)
    cut = (1 << 19) - 128
    pi, compact, ids = b.big_pi(65)
    thr = ps.big_threshold(compact)
    keys = ps.big_keys(71)
    off, tgt = ps.big_csr(keys, n)
    rows = np.concatenate([ids, np.asarray(ps.BIG_ZERO_ROWS, dtype=np.int64)])
    loff, ltgt = ps.big_csr(ps.big_remap(keys), rows.size)
    base, slots = statement(members(ps.big_extended(compact), thr), loff, ltgt, [how])
    # a kernel that keeps row * K in 32 bits would give the wrapped figures: those that read pi differ from the true
    # ones (the degrees, valid and skipped are counted from the adjacency alone)
    wbase, wslots = statement(members(ps.big_extended(ps.big_wrapped(compact)), thr), loff, ltgt, [how])
    differs = [name for name in NODE32 + NODE64 + SUMS if not np.array_equal(base[name], wbase[name])]
    assert differs == [name for name in NODE32 + NODE64 + SUMS if name != "degree"], differs
    assert all(not np.array_equal(x, y) for x, y in zip(slots[0], wslots[0])) and base["counts"] == wbase["counts"]
    assert base["counts"][1] > 20 and base["degree"][640:].all() and not base["own"][640:].any()
    print("big: the wrapped-offset reference differs in %s, home, hcount and hflags" % ", ".join(differs), flush=True)
    d_rows, d_off, d_tgt = b.ctx.from_numpy(rows), b.dev(off), b.dev(tgt)
    views = dict(home=np.int32, votes=np.uint64, squares=np.uint64)

    def check_state(st, what):
        want = dict(base, home=slots[0][0], hcount=slots[0][1], hflags=slots[0][2])
        for name in NODE32 + NODE64 + ("home", "hcount", "hflags"):
            t = st[name]
            assert t.shape[0] == n, name
            got = t[d_rows].cpu().numpy().view(views.get(name, np.uint32))
            assert np.array_equal(got, want[name]), "%s: %s differs from the statement" % (what, name)
            rest = t.clone()
            rest[d_rows] = -1 if name == "home" else 0
            empty = int(T.count_nonzero(rest + 1 if name == "home" else rest))
            assert empty == 0, "%s: %s of a node without a target and without a member is not empty" % (what, name)
        for name in SUMS:
            assert st[name].cpu().numpy().view(np.uint64).tolist() == base[name], "%s: %s differs" % (what, name)
        assert st["counts"].cpu().numpy().tolist() == base["counts"], what + ": counts differ"

    def run(pi, mform):
        st = b.api.run(pi, thr, d_off, d_tgt, among=how[0], top=how[1], min_count=how[2])
        assert b.api.kernel_name() == "roles_nodes_w2", b.api.kernel_name()
        check_state(st, mform)
        mask = b.links.mask(pi, float(F32(thr)))
        assert b.links.kernel_name() == mform, b.links.kernel_name()
        two = b.api.state(n, K, how[1])
        for first, count in ((0, cut), (cut, n - cut)):
            b.api.nodes(mask, n, K, d_off, d_tgt, first=first, count=count, among=how[0], top=how[1], min_count=how[2], state=two)
            assert b.api.kernel_name() == "roles_nodes_w2", b.api.kernel_name()
        assert sorted(two) == sorted(st) and all(T.equal(two[name], st[name]) for name in st), \
            mform + ": two calls cut at node %d differ from one" % cut
        return st

    first = run(pi, "connect_mask_fast")
    del pi
    b.release()
    mis, again, _ = b.big_pi(65, misaligned=True)
    assert np.array_equal(again, compact)
    second = run(mis, "connect_mask_generic")
    assert all(T.equal(first[name], second[name]) for name in first), "the two forms of the mask give other states"
    print("big ok: %d x %d, thr %.3g, %d valid targets, %d skipped" % (n, K, thr, base["counts"][0], base["counts"][1]), flush=True)


def cross_group():
    """from one edge list, both orders of the ends, duplicates and loops included, through the learner's other analyses"""
    from modularity_child import edge_list
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    lrn.Run(5)
    rng = np.random.default_rng(41)
    keys = edge_list(rng, N, 20000)
    thr = 0.05
    r = lrn.NodeRoles(thr, edges=keys)
    deg = lrn.Modularity(thr, edges=keys, degree=True).degree
    assert np.array_equal(r.degree, deg), "degree is not Modularity's"
    q = lrn.CommunityQuality(thr, edges=keys)
    diag = np.diagonal(lrn.CommunityLinks(thr, edges=keys).cpu().numpy()).astype(np.uint64)
    assert np.array_equal(r.ksum, diag) and np.array_equal(diag, 2 * np.asarray(q.internal).astype(np.uint64)), \
        "ksum is not the diagonal of CommunityLinks = 2 internal"
    assert np.array_equal(r.kmembers, lrn.CommunitySizes(thr).cpu().numpy().astype(np.uint64)), "kmembers is not CommunitySizes"
    assert int(r.embedded.astype(np.uint64).sum()) == 2 * (q.links - q.uncovered), "embedded does not sum to 2 (links - uncovered)"
    assert r.skipped == q.skipped > 0 and r.valid == 2 * q.links and int(diag.sum()) > 100
    # the symmetric adjacency of the same list, on the host, under the statement
    off, tgt, lost = symmetric_csr(keys, N)
    base, slots = statement(members(lrn.pi.host(), thr), off, tgt, [("all", 4, 0)])
    base["counts"][1] += lost
    same_result(r, result_of(lrn._roles().rl, thr, ("all", 4, 0), base, slots[0], N), "cross")
    lrn.close()
    print("cross ok", flush=True)


def planted_group():
    """hostlib's planted graph and cover at N = 10^4, pi set to the planted memberships"""
    from mcmc_ammsb_gpu_amd import hostlib
    b = Bench()
    N, K = 10_000, 32
    keys = np.ascontiguousarray(hostlib.generate_graph(N, K, 32, seed=20260101), dtype=np.uint64)
    offsets, mem = hostlib.generate_cover(N, K, seed=20260101)
    M = np.zeros((N, K), dtype=bool)
    for k in range(K):
        M[mem[int(offsets[k]):int(offsets[k + 1])], k] = True
    O = M.sum(axis=1)
    host = np.where(M, (1.0 / np.maximum(O, 1))[:, None], 0.0).astype(F32)
    assert np.array_equal(members(host, 0.05), M) and keys.size > 100_000
    off, tgt, lost = symmetric_csr(keys, N)
    assert lost == 0
    how = ("all", 4, 0)
    mask = b.links.mask(b.matrix(host), float(F32(0.05)))

    def run(off, tgt, what):
        base, slots = statement(M, off, tgt, [how])
        st = b.api.nodes(mask, N, K, b.dev(off), b.dev(tgt), among=how[0], top=how[1], min_count=how[2])
        host_of = lambda n, dt: st[n].cpu().numpy().view(dt)   # noqa: E731
        got = b.rl.Roles(0.05, *how, *[host_of(n, np.uint32) for n in NODE32], *[host_of(n, np.uint64) for n in NODE64],
                         host_of("home", np.int32), host_of("hcount", np.uint32), host_of("hflags", np.uint32),
                         *[host_of(n, np.uint64) for n in SUMS], *st["counts"].cpu().numpy().tolist(), N=N)
        want = result_of(b.rl, 0.05, how, base, slots[0], N)
        same_result(got, want, what)
        return got, want

    got, want = run(off, tgt, "planted")
    # misplaced() is what the statement says it is: no rate is asserted
    assert np.array_equal(got.misplaced(), want.misplaced())
    linked = got.degree > 0
    planted = float(got.embeddedness[linked].mean())
    # the same pi against the same graph with its node ids permuted: the cover no longer fits it (a sign, not a number)
    perm = np.random.default_rng(43).permutation(N).astype(np.uint64)
    a, bb = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    off2, tgt2, _ = symmetric_csr((perm[a.astype(np.int64)] << np.uint64(32)) | perm[bb.astype(np.int64)], N)
    other, _ = run(off2, tgt2, "permuted")
    shuffled = float(other.embeddedness[other.degree > 0].mean())
    assert planted > shuffled, (planted, shuffled)
    print("planted ok: mean embeddedness %.4f against %.4f permuted, %d misplaced" % (planted, shuffled, got.misplaced().size),
          flush=True)


def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _roles
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    seen = []

    def calls(a):
        seen.append((a.NodeRoles(), a.pi.host().copy()))
    ps.unperturbed_run(make, calls, "node roles")
    r, host = seen[0]
    off, tgt = ds.training_csr()
    assert isinstance(r, _roles.Roles) and r.N == N and host.shape == (N, K) and int(off[-1]) > 100_000
    how = ("all", 4, 0)
    base, slots = statement(members(host, 0.05), off, tgt, [how])
    same_result(r, result_of(_roles, 0.05, how, base, slots[0], N), "learner")
    assert r.skipped == 0 and r.valid == int(off[-1]) - int(off[0])
    lrn = make()
    lrn.Run(5)
    how = ("own", 2, 1)
    r = lrn.NodeRoles(0.1, nodes=(100, 5000), top=2, among="own", min_count=1)
    base, slots = statement(members(lrn.pi.host(), 0.1), off, tgt, [how], 100, 5000)
    same_result(r, result_of(_roles, 0.1, how, base, slots[0], N, first=100), "learner range")
    assert r.first == 100 and r.degree.size == 5000 and (r.misplaced().size == 0 or r.misplaced().min() >= 100)
    ps.rejects(AmmsbError, (lambda: lrn.NodeRoles(-1.0), lambda: lrn.NodeRoles(float("nan")), lambda: lrn.NodeRoles(top=0),
                            lambda: lrn.NodeRoles(top=17), lambda: lrn.NodeRoles(among="some"), lambda: lrn.NodeRoles(min_count=-1),
                            lambda: lrn.NodeRoles(nodes=(N - 1, 2)), lambda: lrn.NodeRoles(nodes=(-1, 2))))
    lrn.close()
    print("learner ok graph=%s: %d misplaced" % (graph, seen[0][0].misplaced().size), flush=True)


def _check_file(path, ckpt, lc, K, thr, how, what):
    """a roles file equals, byte for byte, write_roles of the statement over the pi of the checkpoint and the training
    adjacency: both directions of every training link of the link-communities file the same process wrote (c[a, k] does not
    depend on the order inside a row)"""
    from mcmc_ammsb_gpu_amd import _linkcomm, _roles
    fN, r = _roles.read_roles(path)
    assert r.ksum.size == K and F32(r.threshold) == F32(thr) and (r.among, r.top, r.min_count) == how, what
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    keys = np.ascontiguousarray(_linkcomm.read_link_communities(lc)[4], dtype=np.uint64)
    off, tgt, lost = symmetric_csr(keys, fN)
    assert keys.size > 1000 and lost == 0, what
    base, slots = statement(members(pi, thr), off, tgt, [how])
    again = path + ".py"
    _roles.write_roles(again, fN, result_of(_roles, thr, how, base, slots[0], fN))
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the file is not write_roles of the statement" % what
    return fN, r


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("roles_test", d, 300)
        fN, r = _check_file(os.path.join(d, "roles.txt"), os.path.join(d, "cpp.ckpt"), os.path.join(d, "links.txt"), 64, 0.05,
                            ("all", 4, 0), "roles_test")
        assert fN == 20000
        print("cpp ok: Learner::WriteNodeRoles equals the statement over the checkpoint's pi, %d misplaced" % r.misplaced().size,
              flush=True)
        # the command-line driver on a small generated graph; the links from the link-communities file of the same run
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck, lc = os.path.join(d, "r.txt"), os.path.join(d, "main.ckpt"), os.path.join(d, "lc.txt")
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--checkpoint-out", ck, "--link-communities-out", lc]
        for extra, thr, how in (([], 0.05, ("all", 4, 0)),
                                (["--node-roles-threshold", "0.02", "--node-roles-top", "16", "--node-roles-among", "own"], 0.02,
                                 ("own", 16, 0))):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--node-roles-out", out] + extra, 240)
            fN, r = _check_file(out, ck, lc, 48, thr, how, "ammsb_main thr=%g" % thr)
            assert fN == N
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "cut": lambda a: cut_group(),
    "cross": lambda a: cross_group(),
    "planted": lambda a: planted_group(),
    "big": lambda a: big_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
