"""Child process of test_gpu_triangles.py (one per group): the triangles inside the detected communities
(include/ammsb_triangles.h, ops.Triangles, Learner.Triangles) against the integer statement of the header's definitions,
which triangles_statement.py writes once and test_triangles_host.py checks on the CPU against powers of the dense
adjacency.  Every device integer is asserted equal to the statement; the float64 fields, one host formula over equal
integers, are bit-equal.  There is no tolerance in this file."""
import os
import sys

import numpy as np

import postfit_support as ps
import triangles_statement as ts
from modularity_child import edge_list, random_pi

FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
F32 = np.float32
# the kernel's constants (csrc/ammsb_triangles.hip, csrc/ammsb_postfit.h)
W1_WAVES, W2_WAVES, MAX_GRID = 2, 1, 2048
NODE, SUMS = ts.NODE, ts.SUMS
FIELDS = ("degree",) + NODE + SUMS + ("kmembers", "wedges")
DERIVED = ("tpr", "clustering", "local_clustering", "inside")


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _triangles
        super().__init__()
        self.tr = _triangles
        self.lib = _triangles.load()
        self.api = self.ops.Triangles(self.ctx)
        self.links = self.ops.CommunityLinks(self.ctx)

    def run(self, mask, N, K, off, tgt, cuts, what):
        """the call over guarded buffers, the node range in the pieces `cuts` -> name -> host array (per-node arrays whole,
        [N]: what no call handled keeps the fill)"""
        import ctypes as C
        T = self.torch
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        buf = {n: self.guarded(N, T.int32, FILL32) for n in NODE}
        buf.update({n: self.guarded(K, T.int64, FILL64, zero=True) for n in SUMS})
        buf["counts"] = self.guarded(2, T.int64, FILL64, zero=True)
        d_off, d_tgt = self.ctx.from_numpy(off), self.ctx.from_numpy(tgt)
        for first, count in cuts:
            self.tr.check(self.lib.ammsb_triangles_nodes(
                ptr(mask), N, K, ptr(d_off), ptr(d_tgt), first, count, ptr(buf["tri"]), ptr(buf["tri_in"]), ptr(buf["tri_comms"]),
                ptr(buf["ktri3"]), ptr(buf["kpart"]), ptr(buf["counts"]), None))
            if count:
                want = "triangles_nodes_w1" if K <= self.tr.W1_MAX_COLS else "triangles_nodes_w2"
                assert self.tr.last_kernel_name() == want, self.tr.last_kernel_name()
        out = {}
        for n, t in buf.items():
            words = 2 if n == "counts" else K if n in SUMS else N
            host = t.cpu().numpy()
            fill = FILL64 if host.dtype == np.int64 else FILL32
            assert (host[words:].view(np.uint64 if host.dtype == np.int64 else np.uint32) == fill).all(), \
                "%s: the words past %s were written" % (what, n)
            out[n] = host[:words].copy()
        return out


def against(got, base, first, count, what):
    for n in NODE:
        assert np.array_equal(got[n][first:first + count].view(np.uint32), base[n]), "%s: %s differs" % (what, n)
    for n in SUMS:
        assert got[n].view(np.uint64).tolist() == base[n], "%s: %s differs" % (what, n)
    assert got["counts"].tolist() == base["counts"], "%s: counts %s, not %s" % (what, got["counts"].tolist(), base["counts"])


def same(x, y):
    return all(np.array_equal(x[n], y[n]) for n in x)


def result_of(tr, thr, base, M, skipped, dropped, N, first=0):
    return tr.Triangles(thr, *[base[n] for n in FIELDS], M, skipped, dropped, N=N, first=first)


def same_result(r, want, what):
    for n in FIELDS + ("triangles",):
        assert np.array_equal(getattr(r, n), getattr(want, n)), "%s: %s differs" % (what, n)
    for n in ("M", "skipped", "dropped", "first", "total"):
        assert getattr(r, n) == getattr(want, n), "%s: %s is %s, not %s" % (what, n, getattr(r, n), getattr(want, n))
    for n in DERIVED:
        assert getattr(r, n).tobytes() == getattr(want, n).tobytes(), "%s: %s is not bit-equal" % (what, n)
    assert np.float64(r.transitivity).tobytes() == np.float64(want.transitivity).tobytes() and \
        np.float64(r.avg_clustering).tobytes() == np.float64(want.avg_clustering).tobytes(), what
    assert np.array_equal(r.without_triangles(), want.without_triangles()), what


def random_pairs(rng, nodes, n):
    """n unordered pairs among `nodes` (loops and repeats are left to csr_of_pairs)"""
    nodes = np.asarray(nodes, dtype=np.int64)
    return np.stack((nodes[rng.integers(0, nodes.size, n)], nodes[rng.integers(0, nodes.size, n)]), 1)


def clique(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


# ------------------------------------------------------------------------------------------------------------ exact
# K: W = 1, 1, 1, 2, 4, 16, 64 and then the two-word form; K = 65 and 4160 have a last word with unused bits
EXACT_K = (1, 5, 64, 65, 256, 1024, 4096, 4160, 8192)
EXACT_N, LEAD = 5600, 11
ROWS = (63, 64, 65)                                  # rows of exactly this many targets (nodes 90, 91, 92)


def exact_graph(tr):
    """node 0: no link; 1 2 3 and 1 2 8: triangles; 4..7: K4; 9: one target (a leaf of the star); 10..79: a clique of 70;
    80: the centre of a star of 60 leaves (600..659 and node 9), no triangle; 90 91 92: rows of 63, 64 and 65 targets in a
    pool (100..164) with links of its own; 93: a row of two targets; 95..98: hubs of ROW_LDS - 1, ROW_LDS, ROW_LDS + 1 and 5000
    neighbours in 600..5599, over a sparse random graph among those"""
    rng = np.random.default_rng(3)
    pairs = [(1, 2), (2, 3), (1, 3), (1, 8), (2, 8)] + clique(range(4, 8)) + clique(range(10, 80))
    pairs += [(80, b) for b in list(range(600, 659)) + [9]]
    pool = np.arange(100, 165)
    for node, d in zip((90, 91, 92), ROWS):
        pairs += [(node, int(b)) for b in pool[:d]]
    pairs += random_pairs(rng, pool, 300).tolist() + [(93, 100), (93, 101)]
    far = np.arange(600, 5600)
    for node, d in zip((95, 96, 97, 98), (tr.ROW_LDS - 1, tr.ROW_LDS, tr.ROW_LDS + 1, 5000)):
        pairs += [(node, int(b)) for b in far[:d]]
    pairs += random_pairs(rng, far[59:], 6000).tolist()   # (the star's leaves stay leaves)
    off, tgt = ts.csr_of_pairs(pairs, EXACT_N, lead=LEAD)
    deg = np.diff(off.astype(np.int64))
    assert int(off[0]) == LEAD and tgt.size - LEAD <= 40000 and EXACT_N <= 6000
    assert deg[0] == 0 and deg[9] == 1 and deg[93] == 2 and deg[90:93].tolist() == list(ROWS) and deg[10] == 69 and deg[80] == 60
    assert deg[95:99].tolist() == [tr.ROW_LDS - 1, tr.ROW_LDS, tr.ROW_LDS + 1, 5000]
    return off, tgt


def exact_cover(rng, K):
    """random memberships with NaNs and values equal to thr planted; node 3 without a community, so the triangle 1 2 3 has
    none and its edges at 3 take the shortcut; 1 2 8 share exactly one community; the K4 shares the first community and
    the last two (several, across words and inside the last word)"""
    host = random_pi(rng, EXACT_N, K, 0.05, empty=3)
    host[[1, 2, 8]] = F32(0.01)
    host[[1, 2, 8], min(1, K - 1)] = F32(0.9)
    if K > 3:
        host[1, 2], host[2, 3] = F32(0.05), F32(0.7)     # communities of their own: no third corner
    host[4:8, 0] = host[4:8, K - 1] = host[4:8, max(0, K - 2)] = F32(0.5)
    return host


def exact_group(which):
    b = Bench()
    off, tgt = exact_graph(b.tr)
    rng = np.random.default_rng(31)
    thr = float(F32(0.05))
    for i, K in enumerate(EXACT_K):
        host = exact_cover(rng, K)
        if which and i not in which:
            continue
        N, what = EXACT_N, "K=%d" % K
        M = ts.members(host, 0.05)
        base = ts.statement(M, off, tgt)
        assert base["tri"][0] == 0 and base["tri"][80] == 0 and base["tri"][10] == 69 * 68 // 2 and base["tri"][98] > 0
        assert base["tri"][3] == 1 and base["tri_in"][3] == 0 and base["tri"][1] == 2 and base["tri_in"][1] == 1 and base["tri_in"][8] == 1
        assert base["tri_in"][4] == 3 and base["tri_comms"][4] >= min(K, 3) and base["tri_comms"][8] == 1
        mask = b.links.mask(b.matrix(host), thr)
        got = b.run(mask, N, K, off, tgt, [(0, N)], what)
        against(got, base, 0, N, what)
        assert same(got, b.run(mask, N, K, off, tgt, [(0, N)], what)), what + ": two runs differ"
        if K % 64:   # garbage in the bits past K of every last word
            dirty = mask.clone().reshape(N, -1)
            dirty[:, -1] |= b.ctx.from_numpy(np.array([(~((1 << (K % 64)) - 1)) & (2 ** 64 - 1)], dtype=np.uint64))[0]
            assert not b.torch.equal(dirty, mask.reshape(N, -1))
            assert same(got, b.run(dirty.reshape(mask.shape).contiguous(), N, K, off, tgt, [(0, N)], what)), \
                what + ": bits past K changed the result"
        print("exact %s: %d triangle corners, %d inside a community" % (what, base["counts"][0], int(base["tri_in"].sum())), flush=True)
    if not which or 2 in which:
        N, K = EXACT_N, 64
        # thr = 0: every stored number but a NaN is a member, every bit is set, every triangle is inside every community
        host = (rng.random((N, K)) * 0.5).astype(F32)
        M = ts.members(host, 0.0)
        assert M.all()
        base = ts.statement(M, off, tgt)
        mask = b.links.mask(b.matrix(host), 0.0)
        got = b.run(mask, N, K, off, tgt, [(0, N)], "thr=0")
        against(got, base, 0, N, "thr=0")
        assert np.array_equal(base["tri_in"], base["tri"]) and base["ktri3"] == [base["counts"][0]] * K
        # an adjacency without a target, and an empty node range
        off0, tgt0 = np.zeros(N + 1, np.uint64), np.zeros(1, np.uint32)
        got = b.run(mask, N, K, off0, tgt0, [(0, N), (N, 0), (5, 0)], "no target")
        against(got, ts.statement(M, off0, tgt0), 0, N, "no target")
        assert got["counts"].tolist() == [0, 0] and not got["tri"].any() and not got["kpart"].any()
        none = b.run(mask, N, K, off, tgt, [(7, 0)], "empty range")
        assert (none["tri"].view(np.uint32) == FILL32).all() and not none["ktri3"].any()
        # what the layer below refuses, before anything is launched: the state keeps what it held
        from mcmc_ammsb_gpu_amd._capi import AmmsbError
        d_off = b.dev(off)
        state = b.api.state(N, K)
        for t in state.values():
            t.fill_(77)
        for what, at, value in (("an unsorted row", int(off[10]) + 1, int(tgt[int(off[10])])), ("a loop", int(off[10]) + 3, 10),
                                ("a target >= N", int(off[98 + 1]) - 1, N)):
            bad = tgt.copy()
            bad[at] = value
            try:
                b.api.nodes(mask, N, K, d_off, b.dev(bad), state=state)
            except AmmsbError as e:
                print("refused %s: %s" % (what, e), flush=True)
            else:
                raise AssertionError(what + " was accepted")
            assert all(bool((t == 77).all()) for t in state.values()), what + ": an output changed"
        st = b.api.nodes(mask, N, K, d_off, b.dev(tgt))
        assert np.array_equal(st["tri"].cpu().numpy().view(np.uint32), base["tri"]) and \
            st["ktri3"].cpu().numpy().view(np.uint64).tolist() == base["ktri3"], "the layer below differs from the statement"
        print("exact thr=0, no target, refusals ok", flush=True)
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cut
def sparse_pi(rng, N, K, per_node=3):
    host = np.zeros((N, K), F32)
    for _ in range(per_node):
        host[np.arange(N), rng.integers(0, 40, N) * (K // 40)] = 0.9   # (40 communities, spread over all the words)
    return host


def cut_group():
    """more nodes than one pass of the persistent grid (a wave per node: 2048 blocks of 2 waves below K = 4096, of 1 above), in
    one call and in three ragged ranges: bit-equal, the K-sized sums included"""
    b = Bench()
    rng = np.random.default_rng(37)
    for N, K, waves in ((4600, 64, W1_WAVES), (2500, 8192, W2_WAVES)):
        assert N > MAX_GRID * waves
        host = sparse_pi(rng, N, K)
        # triangles need neighbours that know each other: links inside windows of 40 consecutive nodes
        u = rng.integers(0, N, 5 * N)
        v = np.minimum(u + rng.integers(1, 40, 5 * N), N - 1)
        off, tgt = ts.csr_of_pairs(np.stack((u, v), 1), N, lead=5)
        what = "cut N=%d K=%d" % (N, K)
        M = ts.members(host, 0.05)
        mask = b.links.mask(b.matrix(host), float(F32(0.05)))
        one = b.run(mask, N, K, off, tgt, [(0, N)], what)
        c1, c2 = N // 3 - 7, 2 * N // 3 + 5
        three = b.run(mask, N, K, off, tgt, [(c2, N - c2), (0, c1), (c1, c2 - c1)], what + " in three")
        assert same(one, three), what + ": three ragged ranges differ from one call"
        base = ts.statement(M, off, tgt)
        against(one, base, 0, N, what)
        assert base["counts"][0] > N and int(base["tri_in"].sum()) > 100 and (base["tri_in"] < base["tri"]).any()
        # a range alone: its nodes' entries and the sums over them, nothing outside it
        part = b.run(mask, N, K, off, tgt, [(c1, c2 - c1)], what + " middle")
        against(part, ts.statement(M, off, tgt, c1, c2 - c1), c1, c2 - c1, what + " middle")
        assert (part["tri"][:c1].view(np.uint32) == FILL32).all() and (part["tri_comms"][c2:].view(np.uint32) == FILL32).all()
        print("%s ok: %d triangle corners" % (what, base["counts"][0]), flush=True)
    print("cut ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cross
def cross_group():
    """through the learner on one edge list, against the other analyses and against partitions whose answer is known"""
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    lrn.Run(5)
    lrn.drain()
    tr = lrn._triangles().tr
    rng = np.random.default_rng(41)
    off, tgt, _, _ = tr.simple_csr_host(*ds.training_csr(), N)
    # a partition: one community per node
    part = rng.integers(0, K, N)
    host = np.zeros((N, K), F32)
    host[np.arange(N), part] = 1.0
    lrn.pi.load(host)
    r = lrn.Triangles(0.5)
    base = ts.statement(ts.members(host, 0.5), off, tgt)
    same_result(r, result_of(tr, 0.5, base, tgt.size, 0, 0, N), "partition")
    assert int(r.ktri3.sum()) == int(r.tri_in.astype(np.uint64).sum()) > 0 and r.total > 1000
    src = np.repeat(np.arange(N), np.diff(off.astype(np.int64)))
    for k in range(K):
        ids = np.flatnonzero(part == k)
        new = np.full(N, -1, np.int64)
        new[ids] = np.arange(ids.size)
        keep = (part[src] == k) & (part[tgt.astype(np.int64)] == k)
        o, t = ts.csr_of_pairs(np.stack((new[src[keep]], new[tgt[keep].astype(np.int64)]), 1), ids.size)
        alone = ts.statement(np.ones((ids.size, 1), bool), o, t)
        assert int(r.triangles[k]) * 3 == alone["ktri3"][0] == alone["counts"][0], "community %d" % k
    assert (r.wedges >= r.ktri3).all()
    assert np.array_equal(r.degree, lrn.NodeRoles(0.5).degree), "degree is not NodeRoles' over the same adjacency"
    # every node in community 0
    host[:] = 0
    host[:, 0] = 1.0
    lrn.pi.load(host)
    r = lrn.Triangles(0.5)
    tri_sum = int(r.tri.astype(np.uint64).sum())
    assert int(r.ktri3[0]) == tri_sum == 3 * r.total and int(r.kpart[0]) == int((r.tri > 0).sum()) and np.array_equal(r.tri_in, r.tri)
    assert not r.ktri3[1:].any() and (r.wedges >= r.ktri3).all() and np.array_equal(r.tri, base["tri"])
    assert np.array_equal(r.tri_comms, (r.tri > 0).astype(np.uint32)) and int(r.kmembers[0]) == N
    # a list with repeats, loops and ends >= N gives the integers of its simplified list
    lrn.pi.load(np.where(rng.random((N, K)) < 0.2, 0.3, 0.0).astype(F32))
    u = rng.integers(0, N, 30000)
    dense = (u.astype(np.uint64) << np.uint64(32)) | np.minimum(u + rng.integers(1, 30, u.size), N - 1).astype(np.uint64)
    keys = np.concatenate((edge_list(rng, N, 20000), dense, dense[:500] >> np.uint64(32) | dense[:500] << np.uint64(32)))
    o2, t2, skipped, dropped = tr.simple_csr_of_keys(keys, N)
    assert skipped > 100 and dropped > 1000
    r = lrn.Triangles(0.25, edges=keys)
    base = ts.statement(ts.members(lrn.pi.host(), 0.25), o2, t2)
    same_result(r, result_of(tr, 0.25, base, t2.size, skipped, dropped, N), "a list with repeats and loops")
    s2 = np.repeat(np.arange(N, dtype=np.uint64), np.diff(o2.astype(np.int64)))
    once = ((s2 << np.uint64(32)) | t2.astype(np.uint64))[s2 < t2]
    again = lrn.Triangles(0.25, edges=once)
    assert (again.skipped, again.dropped, again.M) == (0, 0, t2.size) and r.total > 100
    for n in FIELDS:
        assert np.array_equal(getattr(again, n), getattr(r, n)), n
    assert (r.wedges >= r.ktri3).all()
    lrn.close()
    print("cross ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ far
FAR_ROWS, FAR_K, FAR_W = (1 << 22) + 128, 8192, 128
FAR_WINDOWS = ((0, 128), ((1 << 21) - 64, (1 << 21) + 64), ((1 << 22) - 64, FAR_ROWS))


def far_group():
    """a mask past byte offset 2^32: 2^22 + 128 rows of 128 words (4 GiB + 128 KiB), zeroed on the device, planted rows in
    [0, 128), around row 2^21 and around row 2^22; the statement in the compact numbering of the planted rows"""
    b = Bench()
    T = b.torch
    rng = np.random.default_rng(53)
    ids = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in FAR_WINDOWS])
    n = ids.size
    hot = np.array([0, 63, 64, 1000, 4095, 4096, 4100, 8000, 8191])    # both words of a lane, both ends of a word
    M = rng.random((n, FAR_K)) < 0.002
    M[:, hot] = rng.random((n, hot.size)) < 0.4
    M[5] = False
    pairs = np.concatenate((random_pairs(rng, np.arange(n), 5000), random_pairs(rng, np.arange(n - 192, n), 1500)))
    off_c, tgt_c = ts.csr_of_pairs(pairs, n)
    base = ts.statement(M, off_c, tgt_c)
    # a byte offset row * 1024 kept in 32 bits reads row - 2^22 for the last 128 rows: the statement over those rows
    wrapped = M.copy()
    high = ids >= (1 << 22)
    wrapped[high] = M[ids[high] - (1 << 22)]      # (rows 0..127 are the compact rows 0..127)
    wbase = ts.statement(wrapped, off_c, tgt_c)
    differs = [name for name in NODE + SUMS if not np.array_equal(np.asarray(base[name]), np.asarray(wbase[name]))]
    assert "tri" not in differs and all(name in differs for name in ("tri_in", "ktri3", "kpart")), differs
    assert base["counts"][0] > 3000 and int(base["tri_in"][high].sum()) > 100 and base["counts"] == wbase["counts"]
    print("far: the wrapped-offset statement differs in %s" % ", ".join(differs), flush=True)
    # the same graph over the global ids (ascending with the compact ones, so every row stays ascending)
    src = np.repeat(np.arange(n), np.diff(off_c.astype(np.int64)))
    off = np.zeros(FAR_ROWS + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(ids[src], minlength=FAR_ROWS))
    tgt = ids[tgt_c.astype(np.int64)].astype(np.uint32)
    mask = T.zeros((FAR_ROWS, FAR_W), dtype=T.int64, device="cuda")
    assert mask.numel() * 8 == (1 << 32) + (128 << 10)
    words = np.packbits(M, axis=1, bitorder="little").view(np.uint64)
    assert words.shape == (n, FAR_W)
    d_ids = b.dev(ids)
    mask[d_ids] = b.dev(words).view(T.int64)
    st = b.api.nodes(mask, FAR_ROWS, FAR_K, b.dev(off), b.dev(tgt))
    assert b.api.kernel_name() == "triangles_nodes_w2", b.api.kernel_name()
    for name in NODE:
        t = st[name]
        assert np.array_equal(t[d_ids].cpu().numpy().view(np.uint32), base[name]), "far: %s differs from the statement" % name
        rest = t.clone()
        rest[d_ids] = 0
        assert int(T.count_nonzero(rest)) == 0, "far: %s of a node without a link is not 0" % name
    for name in SUMS:
        assert st[name].cpu().numpy().view(np.uint64).tolist() == base[name], "far: %s differs" % name
    assert st["counts"].cpu().numpy().tolist() == base["counts"]
    print("far ok: %d rows, %d triangle corners, %d inside a community" % (FAR_ROWS, base["counts"][0], int(base["tri_in"].sum())),
          flush=True)


# ------------------------------------------------------------------------------------------------------------ planted
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
    host = np.where(M, (1.0 / np.maximum(M.sum(axis=1), 1))[:, None], 0.0).astype(F32)
    assert np.array_equal(ts.members(host, 0.05), M) and keys.size > 100_000
    mask = b.links.mask(b.matrix(host), float(F32(0.05)))
    roles = b.ops.NodeRoles(b.ctx)

    def run(keys, what):
        off, tgt, skipped, dropped = b.tr.simple_csr_of_keys(keys, N)
        base = ts.statement(M, off, tgt)
        d_off, d_tgt = b.dev(off), b.dev(tgt)
        st = b.api.nodes(mask, N, K, d_off, d_tgt)
        rs = roles.nodes(mask, N, K, d_off, d_tgt, top=0)
        h32 = lambda s, n: s[n].cpu().numpy().view(np.uint32)   # noqa: E731
        h64 = lambda s, n: s[n].cpu().numpy().view(np.uint64)   # noqa: E731
        got = b.tr.Triangles(0.05, h32(rs, "degree"), h32(st, "tri"), h32(st, "tri_in"), h32(st, "tri_comms"), h64(st, "ktri3"),
                             h64(st, "kpart"), h64(rs, "kmembers"), (h64(rs, "ksq") - h64(rs, "ksum")) // np.uint64(2), tgt.size,
                             skipped, dropped, N=N)
        same_result(got, result_of(b.tr, 0.05, base, tgt.size, skipped, dropped, N), what)
        assert st["counts"].cpu().numpy().tolist() == base["counts"]
        return got

    got = run(keys, "planted")
    sized = got.kmembers >= 3
    planted = float(got.tpr[sized].mean())
    # the same pi against the same graph with its node ids permuted: the cover no longer fits it (a sign, not a number)
    perm = np.random.default_rng(43).permutation(N).astype(np.uint64)
    a, bb = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    other = run((perm[a.astype(np.int64)] << np.uint64(32)) | perm[bb.astype(np.int64)], "permuted")
    shuffled = float(other.tpr[other.kmembers >= 3].mean())
    assert other.total == got.total and planted > shuffled, (planted, shuffled)
    print("planted ok: mean tpr %.4f against %.4f permuted, %d triangles" % (planted, shuffled, got.total), flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _triangles
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    seen = []

    def calls(a):
        seen.append((a.Triangles(), a.pi.host().copy()))
    ps.unperturbed_run(make, calls, "triangles")
    r, host = seen[0]
    off, tgt, _, half = _triangles.simple_csr_host(*ds.training_csr(), N)
    assert isinstance(r, _triangles.Triangles) and r.N == N and host.shape == (N, K) and tgt.size > 100_000 and 2 * half == tgt.size
    base = ts.statement(ts.members(host, 0.05), off, tgt)
    same_result(r, result_of(_triangles, 0.05, base, tgt.size, 0, 0, N), "learner")
    assert r.whole and r.total > 1000
    lrn = make()
    lrn.Run(5)
    r = lrn.Triangles(0.1, nodes=(100, 5000))
    base = ts.statement(ts.members(lrn.pi.host(), 0.1), off, tgt, 100, 5000)
    same_result(r, result_of(_triangles, 0.1, base, tgt.size, 0, 0, N, first=100), "learner range")
    assert r.first == 100 and r.degree.size == 5000 and not r.whole
    ps.rejects(AmmsbError, (lambda: lrn.Triangles(-1.0), lambda: lrn.Triangles(float("nan")), lambda: lrn.Triangles(nodes=(N - 1, 2)),
                            lambda: lrn.Triangles(nodes=(-1, 2))))
    lrn.close()
    print("learner ok graph=%s: %d triangles, %d communities without one" % (graph, seen[0][0].total, seen[0][0].without_triangles().size),
          flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def _check_file(path, ckpt, lc, K, thr, what):
    """a triangles file equals, byte for byte, write_triangles of the statement over the pi of the checkpoint and the
    training links of the link-communities file the same process wrote"""
    from mcmc_ammsb_gpu_amd import _linkcomm, _triangles
    fN, r = _triangles.read_triangles(path)
    assert r.ktri3.size == K and F32(r.threshold) == F32(thr), what
    pi, _ = ps.pi_beta_of_checkpoint(open(ckpt, "rb").read(), fN, K)
    keys = np.ascontiguousarray(_linkcomm.read_link_communities(lc)[4], dtype=np.uint64)
    off, tgt, skipped, dropped = _triangles.simple_csr_of_keys(keys, fN)
    assert keys.size > 1000 and (skipped, dropped) == (0, 0), what
    base = ts.statement(ts.members(pi, thr), off, tgt)
    again = path + ".py"
    _triangles.write_triangles(again, fN, result_of(_triangles, thr, base, tgt.size, 0, 0, fN))
    assert open(again, "rb").read() == open(path, "rb").read(), "%s: the file is not write_triangles of the statement" % what
    return fN, r


def cpp_group():
    import tempfile
    from mcmc_ammsb_gpu_amd import hostlib
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("triangles_test", d, 300)
        fN, r = _check_file(os.path.join(d, "triangles.txt"), os.path.join(d, "cpp.ckpt"), os.path.join(d, "links.txt"), 64, 0.05,
                            "triangles_test")
        assert fN == 20000 and r.total > 0
        print("cpp ok: Learner::WriteTriangles equals the statement over the checkpoint's pi, %d triangles" % r.total, flush=True)
        # the command-line driver on a small generated graph; the links from the link-communities file of the same run
        N = 3000
        f = os.path.join(d, "g.bin.gz")
        hostlib.dump_dataset(f, N, 0.02, hostlib.generate_graph(N, 8, 12, seed=3))
        out, ck, lc = os.path.join(d, "t.txt"), os.path.join(d, "main.ckpt"), os.path.join(d, "lc.txt")
        tail = ["-k", "48", "-m", "256", "-n", "16", "-x", "60", "-i", "30", "--checkpoint-out", ck, "--link-communities-out", lc]
        for extra, thr in (([], 0.05), (["--triangles-threshold", "0.02"], 0.02)):
            ps.run_ammsb_main(["--load-data", "1", "--load-file", f] + tail + ["--triangles-out", out] + extra, 240)
            fN, r = _check_file(out, ck, lc, 48, thr, "ammsb_main thr=%g" % thr)
            assert fN == N and r.total > 0
        print("cli ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "cut": lambda a: cut_group(),
    "cross": lambda a: cross_group(),
    "far": lambda a: far_group(),
    "planted": lambda a: planted_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
