"""Child process of test_gpu_cores.py (one per group): the k-core decomposition of every detected community
(include/ammsb_cores.h, ops.CommunityCores, Learner.CommunityCores) against the statement of the header's definitions, which
cores_statement.py writes once and test_cores_host.py checks on the CPU against the definition itself.  Every device integer
is asserted equal; the float64 fields, one host formula over equal integers, are bit-equal.  There is no tolerance in this
file.

What every call refuses with AMMSB_EINVAL before anything is launched (refused() below makes these calls and then checks that
no output changed):
  degrees    num_cols 0 and 8193; num_rows 2^32; num_slots 2^32; a node range past num_rows; mask NULL; offsets 4 bytes off;
             indeg 2 bytes off; counts NULL
  adjacency  num_nbr 2^32; nbr_off 4 bytes off; nbr NULL; a node range past num_rows
  scan       num_slots 2^32; tail 4 bytes off; deg NULL; next_level NULL
  peel       head > tail; tail > num_slots; num_nbr 2^32; nbr NULL with entries; deg 2 bytes off
  finish     num_slots 2^32; base NULL; degeneracy NULL; slot_comm 1 byte off; num_cols 0"""
import ctypes as C
import sys

import numpy as np

import cores_statement as cs
import postfit_support as ps
from modularity_child import edge_list

FILL = {np.dtype(np.int16): 0x5A5A, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
F32 = np.float32
# the kernels' constants (csrc/ammsb_cores.hip, csrc/ammsb_postfit.h)
WAVES, MAX_GRID, PEEL_LANES, BLOCK = 4, 2048, 16, 256
OUT = cs.PER_COMMUNITY + cs.PER_SLOT + cs.PER_NODE
VIEW = {"members": np.uint64, "inlinks2": np.uint64, "degeneracy": np.uint32, "nucleus": np.uint64, "isolated": np.uint64,
        "community": np.uint16, "indeg": np.uint32, "core": np.uint32, "best_core": np.uint32, "best_comm": np.int32,
        "in_nucleus": np.uint32, "nbr": np.uint32}


def key(a, b):
    return (int(a) << 32) | int(b)


def keys_of(pairs):
    return np.array([key(a, b) for a, b in pairs], dtype=np.uint64)


def clique(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _cores
        super().__init__()
        self.co = _cores
        self.lib = _cores.load()
        self.api = self.ops.CommunityCores(self.ctx)
        self.links = self.api.links

    def csr(self, csr):
        offsets, targets = csr
        return self.dev(offsets).view(self.torch.int64), self.dev(targets if targets.size else np.zeros(1, np.uint32)).view(self.torch.int32)

    def run(self, mask, N, K, csr, what, node_cuts=None):
        """the library's calls over guarded buffers, the node range of the two build passes in `node_cuts` -> name -> host
        array"""
        T = self.torch
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        form = lambda name: "cores_%s_w%d" % (name, 1 if K <= self.co.W1_MAX_COLS else 2)   # noqa: E731
        fill = lambda dt: FILL[np.dtype(str(dt).split(".")[1])]   # noqa: E731
        cuts = node_cuts or [(0, N)]
        offsets, targets = self.csr(csr)
        base, M = self.api.comp.base(self.api.comp.own(mask, N, K))
        slot_comm = self.api.comp.slots(mask, N, K, base, M, self.api.comp.state(N, K, M))["slot_comm"]
        sizes = {"indeg": (M, T.int32), "deg": (M, T.int32), "queue": (M, T.int32), "members": (K, T.int64), "inlinks2": (K, T.int64),
                 "degeneracy": (K, T.int32), "nucleus": (K, T.int64), "isolated": (K, T.int64), "best_core": (N, T.int32),
                 "best_comm": (N, T.int32), "in_nucleus": (N, T.int32), "counts": (4, T.int64), "ctl": (2, T.int64)}
        zeroed = ("members", "inlinks2", "degeneracy", "nucleus", "isolated", "counts", "ctl")
        buf = {n: self.guarded(w, dt, fill(dt), zero=n in zeroed) for n, (w, dt) in sizes.items()}
        for first, count in cuts:
            self.co.check(self.lib.ammsb_cores_degrees(ptr(mask), N, K, ptr(base), M, ptr(offsets), ptr(targets), first, count,
                                                       ptr(buf["indeg"]), ptr(buf["counts"]), None))
        if M:
            assert self.co.last_kernel_name() == form("degrees"), self.co.last_kernel_name()
        nbr_off, L = self.api.offsets(buf["indeg"][:M])
        sizes["nbr"] = (L, T.int32)
        buf["nbr"] = self.guarded(L, T.int32, fill(T.int32))
        for first, count in cuts:
            self.co.check(self.lib.ammsb_cores_adjacency(ptr(mask), N, K, ptr(base), M, ptr(offsets), ptr(targets), first, count,
                                                         ptr(buf["indeg"]), ptr(nbr_off), L, ptr(buf["nbr"]), None))
        if M and L:
            assert self.co.last_kernel_name() == form("adjacency"), self.co.last_kernel_name()
        buf["deg"][:M].copy_(buf["indeg"][:M])
        views = {n: buf[n][:sizes[n][0]] for n in buf}
        scans, rounds = self.api.peel(M, views["indeg"], nbr_off, views["nbr"], views)
        self.api.finish(N, K, base, M, slot_comm, views["indeg"], views)
        assert self.co.last_kernel_name() == "cores_finish_nodes"
        out = {}
        for n, t in buf.items():
            host = t.cpu().numpy()
            words = sizes[n][0]
            assert (host[words:] == host.dtype.type(FILL[host.dtype])).all() and host.size == words + ps.GUARD, \
                "%s: the words past %s were written" % (what, n)
            out[n] = host[:words].copy()
        out["offsets"], out["community"] = base.cpu().numpy().view(np.uint64), slot_comm.cpu().numpy()
        out["nbr_off"], out["core"] = nbr_off.cpu().numpy().view(np.uint64), out["deg"]
        assert out["counts"].view(np.uint64).tolist() == [M, L, scans, rounds], "%s: counts %s" % (what, out["counts"])
        return out


def against(got, base, what):
    assert np.array_equal(got["offsets"], base["offsets"]), what + ": offsets differ"
    assert np.array_equal(got["nbr_off"], base["nbr_off"]), what + ": nbr_off differs"
    for n in OUT + ("nbr",):
        assert np.array_equal(got[n].view(VIEW[n]), base[n]), "%s: %s differs" % (what, n)
    M, L, scans, rounds = got["counts"].view(np.uint64).tolist()
    assert (M, L) == (base["M"], base["L"]), "%s: counts %s" % (what, got["counts"])
    distinct = np.unique(base["core"]).size
    assert rounds <= max(M, 0) and scans <= 2 * distinct + 1, "%s: %d scans and %d rounds for %d core values" % (what, scans, rounds, distinct)
    assert sorted(got["queue"].view(np.uint32).tolist()) == list(range(M)), what + ": the queue does not hold every slot once"


def same(x, y):
    """everything but the order in which the queue filled and the launch counts"""
    return all(np.array_equal(x[n], y[n]) for n in x if n not in ("queue", "counts", "ctl"))


def same_result(r, want, what):
    for n in OUT + ("offsets",):
        assert np.array_equal(getattr(r, n), getattr(want, n)), "%s: %s differs" % (what, n)
    for n in ("M", "L", "N", "skipped", "dropped"):
        assert getattr(r, n) == getattr(want, n), "%s: %s is %s, not %s" % (what, n, getattr(r, n), getattr(want, n))
    for n in ("coreness", "nucleus_share", "mean_core"):
        assert getattr(r, n).tobytes() == getattr(want, n).tobytes(), "%s: %s is not bit-equal" % (what, n)
    assert np.array_equal(r.fringe(), want.fringe()), what
    for f in ("nuclei", "cover"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(r, f)(*((2,) if f == "cover" else ())),
                                                        getattr(want, f)(*((2,) if f == "cover" else ())))), "%s: %s differs" % (what, f)


# ------------------------------------------------------------------------------------------------------------ exact
# K: W = 1, 1, 1, 2, 4, 16, 64 and then the two-word form; K = 65 and 4160 have a last word with unused bits
EXACT_K = (1, 5, 64, 65, 256, 1024, 4096, 4160, 8192)
EXACT_N, THR = 6000, 0.05
PATH = range(0, 2000)
LEAVES, CENTRE = range(2000, 5000), 5000
CLIQUE, CYCLE = range(5100, 5140), range(5150, 5190)
K20, FR1, FR2 = range(5200, 5220), range(5220, 5260), range(5260, 5280)
SHARED, QUIET, MANY, LONE = range(5300, 5312), range(5350, 5400), range(5500, 5510), 5999


def exact_graph():
    """a clique of 40; a cycle of 40; a path of 2000 with its keys ascending, descending and shuffled; a star of 3000 leaves; a
    K20 with 40 members hanging on one of its nodes each and 20 on two; a clique two communities share; QUIET without a key
    among its nodes; a ring with chords over MANY; loops, repeats, both orders of the ends, ends >= N; random keys among the
    leaves and between QUIET and the leaves"""
    rng = np.random.default_rng(5)
    step = [(i, i + 1) for i in PATH[:-1]]
    pairs = step + step[::-1] + [(i + 1, i) for i in rng.permutation(len(PATH) - 1)]
    pairs += [(CENTRE, i) if i % 2 else (i, CENTRE) for i in LEAVES]
    pairs += clique(CLIQUE) + [(CYCLE[i], CYCLE[(i + 1) % len(CYCLE)]) for i in range(len(CYCLE))]
    pairs += clique(K20) + [(f, K20[i % 20]) for i, f in enumerate(FR1)]
    pairs += [(f, K20[i]) for i, f in enumerate(FR2)] + [(K20[(i + 7) % 20], f) for i, f in enumerate(FR2)]
    pairs += clique(SHARED) + [(q, int(rng.integers(2000, 5000))) for q in QUIET]
    pairs += [(MANY[i], MANY[(i + d) % len(MANY)]) for i in range(len(MANY)) for d in (1, 3)]
    pairs += [(7, 7), (CLIQUE[0], CLIQUE[0]), (5, 6), (6, 5), (EXACT_N, 3), (3, 2 ** 32 - 1), (EXACT_N + 9, EXACT_N)]
    noise = edge_list(rng, 3000, 20000)              # (some of its ends are past its range on purpose)
    a, b = noise >> np.uint64(32), noise & np.uint64(0xFFFFFFFF)
    noise = ((a + np.uint64(2000)) << np.uint64(32)) | (b + np.uint64(2000))   # among the leaves (and the centre, and past N)
    keys = np.concatenate((keys_of(pairs), noise))
    assert keys.size < 60000
    return keys


def exact_cover(rng, K):
    """c[i] = i % K for the planted communities: 0 the path, 1 the star, 2 the clique and the cycle, 3 the K20 with its fringe, 4
    and 5 the shared clique (5 with QUIET as well), 6 QUIET alone; MANY share K - 1, K - 3 (inside the last word), K // 2
    (another word) and 7; K - 2 stays empty; a sparse random background in the communities 8 .. K - 9 with values equal to thr
    planted, NaNs everywhere.  Below K = 64 the planted communities fall on each other, and the statement says what then
    holds."""
    N = EXACT_N
    host = (rng.random((N, K)) * 0.9 * THR).astype(F32)
    lo, hi = (8, K - 8) if K >= 64 else (0, K)
    for _ in range(2):
        host[np.arange(N), rng.integers(lo, hi, N)] = F32(0.3)
    host[rng.integers(0, N, 400), rng.integers(lo, hi, 400)] = F32(THR)
    host[rng.integers(0, N, 400), rng.integers(0, K, 400)] = np.nan
    c = [i % K for i in range(8)]
    host[list(PATH), c[0]] = 0.9
    host[list(LEAVES) + [CENTRE], c[1]] = 0.8
    host[list(CLIQUE) + list(CYCLE), c[2]] = 0.7
    host[list(K20) + list(FR1) + list(FR2), c[3]] = F32(THR)
    host[list(SHARED), c[4]] = 0.6
    host[list(SHARED) + list(QUIET), c[5]] = 0.6
    host[list(QUIET), c[6]] = 0.6
    for k in (K - 1, max(0, K - 3), K // 2, c[7]):
        host[list(MANY), k] = 0.5
    if K >= 64:
        host[:, K - 2] = F32(0.5) * F32(THR)
    host[LONE] = F32(0.5) * F32(THR)
    if K >= 64:
        host[CLIQUE[5], c[3]] = np.nan
    return host


def exact_properties(base, K):
    """what the planted graph is there for, read off the statement (K >= 64: the planted communities are apart)"""
    off = base["offsets"].astype(np.int64)

    def at(a, k):
        s = np.flatnonzero(base["community"][off[a]:off[a + 1]] == k)
        return (int(base["indeg"][off[a] + s[0]]), int(base["core"][off[a] + s[0]])) if s.size else None

    assert at(PATH[0], 0) == (1, 1) and at(PATH[1000], 0) == (2, 1) and base["degeneracy"][0] == 1
    assert at(CENTRE, 1)[0] == len(LEAVES) and at(LEAVES[5], 1)[1] >= 1
    assert at(CLIQUE[3], 2) == (39, 39) and at(CYCLE[3], 2) == (2, 2) and base["degeneracy"][2] == 39 and base["nucleus"][2] == 40
    assert at(K20[0], 3)[1] == 19 and at(FR1[4], 3) == (1, 1) and at(FR2[4], 3) == (2, 2) and base["nucleus"][3] == 20
    assert at(SHARED[2], 4) == (11, 11) == at(SHARED[2], 5) and at(QUIET[2], 5) == (0, 0) == at(QUIET[2], 6)
    assert base["isolated"][6] == base["members"][6] == len(QUIET) and base["degeneracy"][6] == 0 and base["nucleus"][6] == len(QUIET)
    assert base["members"][K - 2] == 0 and base["degeneracy"][K - 2] == 0 and base["nucleus"][K - 2] == 0
    assert off[LONE + 1] == off[LONE] and base["best_comm"][LONE] == -1 and base["best_core"][LONE] == 0
    for k in (K - 1, K - 3, K // 2, 7):
        assert at(MANY[4], k) == (4, 4)
    assert base["best_core"][CLIQUE[3]] == 39 and base["best_comm"][CLIQUE[3]] == 2 and base["in_nucleus"][MANY[0]] == 4
    assert base["skipped"] >= 3 and base["dropped"] > 2000


def refused(b, mask, N, K, csr):
    """the bad calls of this file's header: every one returns an error and no output changes"""
    T = b.torch
    ptr = lambda x, o=0: C.c_void_p(x.data_ptr() + o)   # noqa: E731
    offsets, targets = b.csr(csr)
    base, M = b.api.comp.base(b.api.comp.own(mask, N, K))
    slot_comm = b.api.comp.slots(mask, N, K, base, M, b.api.comp.state(N, K, M))["slot_comm"]
    indeg, counts = b.api.degrees(mask, N, K, base, M, offsets, targets)
    nbr_off, Lq = b.api.offsets(indeg)
    nbr = b.api.adjacency(mask, N, K, base, M, offsets, targets, indeg, nbr_off, Lq)
    st = b.api.state(N, K, M, indeg)
    outs = [indeg.clone(), nbr.clone()] + list(st.values())
    indeg2, nbr2 = outs[0], outs[1]
    for t in outs:
        t.fill_(77)
    L = b.lib
    g = lambda **kw: [kw.get("mask", ptr(mask)), kw.get("N", N), kw.get("K", K), ptr(base), kw.get("M", M),   # noqa: E731
                      kw.get("offsets", ptr(offsets)), ptr(targets), kw.get("first", 0), kw.get("n", N)]
    deg = lambda head, indeg=ptr(indeg2), counts=ptr(st["counts"]): L.ammsb_cores_degrees(*head, indeg, counts, None)   # noqa: E731
    adj = lambda head, off=ptr(nbr_off), n=Lq, nb=ptr(nbr2): L.ammsb_cores_adjacency(*head, ptr(indeg), off, n, nb, None)   # noqa: E731
    scan = lambda M=M, deg=ptr(st["deg"]), tail=ptr(st["ctl"]), nxt=ptr(st["ctl"], 8): L.ammsb_cores_scan(   # noqa: E731
        M, 0, deg, ptr(st["queue"]), tail, nxt, ptr(st["counts"]), None)
    peel = lambda head=0, tail=1, n=Lq, nb=ptr(nbr), deg=ptr(st["deg"]): L.ammsb_cores_peel(   # noqa: E731
        M, 0, head, tail, ptr(nbr_off), ptr(indeg), nb, n, deg, ptr(st["queue"]), ptr(st["ctl"]), ptr(st["counts"]), None)
    fin = [ptr(slot_comm), ptr(indeg), ptr(st["deg"])] + [ptr(st[n]) for n in ("members", "inlinks2", "degeneracy", "nucleus",
                                                                              "isolated", "best_core", "best_comm", "in_nucleus")]
    finish = lambda K=K, base=ptr(base), M=M, fin=fin: L.ammsb_cores_finish(N, K, base, M, *fin, None)   # noqa: E731
    calls = [
        lambda: deg(g(K=0)), lambda: deg(g(K=8193)), lambda: deg(g(N=1 << 32)), lambda: deg(g(M=1 << 32)),
        lambda: deg(g(first=N - 1, n=2)), lambda: deg(g(mask=None)), lambda: deg(g(offsets=ptr(offsets, 4))),
        lambda: deg(g(), indeg=ptr(indeg2, 2)), lambda: deg(g(), counts=None),
        lambda: adj(g(), n=1 << 32), lambda: adj(g(), off=ptr(nbr_off, 4)), lambda: adj(g(), nb=None), lambda: adj(g(first=1, n=N)),
        lambda: scan(M=1 << 32), lambda: scan(tail=ptr(st["ctl"], 4)), lambda: scan(deg=None), lambda: scan(nxt=None),
        lambda: peel(head=2, tail=1), lambda: peel(tail=M + 1), lambda: peel(n=1 << 32), lambda: peel(nb=None),
        lambda: peel(deg=ptr(st["deg"], 2)),
        lambda: finish(M=1 << 32), lambda: finish(base=None), lambda: finish(fin=fin[:5] + [None] + fin[6:]),
        lambda: finish(fin=[ptr(slot_comm, 1)] + fin[1:]), lambda: finish(K=0),
    ]
    assert M > 1 and Lq > 0
    for i, call in enumerate(calls):
        rc = call()
        assert rc != 0 and b.co._LIBRARY._call("last_error"), "bad call %d was accepted" % i
    T.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in outs), "a refused call changed an output"
    return len(calls)


def exact_group(which):
    b = Bench()
    keys = exact_graph()
    rng = np.random.default_rng(31)
    thr = float(F32(THR))
    N = EXACT_N
    seen = set()
    for i, K in enumerate(EXACT_K):
        host = exact_cover(rng, K)
        if which and i not in which:
            continue
        what = "K=%d" % K
        M = cs.members(host, THR)
        base = cs.statement(M, keys)
        if K >= 64:
            exact_properties(base, K)
        mask = b.links.mask(b.matrix(host), thr)
        got = b.run(mask, N, K, base["csr"], what)
        seen.add(1 if K <= b.co.W1_MAX_COLS else 2)
        against(got, base, what)
        assert same(got, b.run(mask, N, K, base["csr"], what)), what + ": two runs differ"
        if K % 64:   # garbage in the bits past K of every last word
            dirty = mask.clone().reshape(N, -1)
            dirty[:, -1] |= b.ctx.from_numpy(np.array([(~((1 << (K % 64)) - 1)) & (2 ** 64 - 1)], dtype=np.uint64))[0]
            assert not b.torch.equal(dirty, mask.reshape(N, -1))
            assert same(got, b.run(dirty.reshape(mask.shape).contiguous(), N, K, base["csr"], what)), what + ": bits past K changed the result"
        # an empty list: every member isolated
        empty = cs.statement(M, np.zeros(0, np.uint64))
        none = b.run(mask, N, K, empty["csr"], what + " no key")
        against(none, empty, what + " no key")
        assert not none["core"].any() and np.array_equal(none["isolated"], none["members"])
        print("exact %s: %d slots, %d entries, degeneracy %d, %d scans, %d rounds" % (
            what, base["M"], base["L"], int(base["degeneracy"].max()), *got["counts"].view(np.uint64).tolist()[2:]), flush=True)
    if not which or 2 in which:
        K = 64
        host = (rng.random((N, K)) * 0.5).astype(F32)   # thr = 0: every stored number but a NaN is a member
        host[rng.integers(0, N, 50), rng.integers(0, K, 50)] = np.nan
        M = cs.members(host, 0.0)
        assert M.sum() > N * K - 51
        mask = b.links.mask(b.matrix(host), 0.0)
        base = cs.statement(M, keys)
        against(b.run(mask, N, K, base["csr"], "thr=0"), base, "thr=0")
        print("exact thr=0 ok; %d bad calls refused" % refused(b, mask, N, K, base["csr"]), flush=True)
    if not which:
        assert seen == {1, 2}
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cut
def cut_group():
    """degrees and adjacency in one call, in three ragged node ranges and in the ranges reversed, under both forms; and a
    frontier larger than one pass of the peel's grid: more than 2^18 slots that leave at one level"""
    b = Bench()
    rng = np.random.default_rng(37)
    for N, K in ((3000, 4096), (3000, 8192)):
        host = np.zeros((N, K), F32)
        for _ in range(3):
            host[np.arange(N), rng.integers(0, 40, N) * (K // 40)] = 0.9   # (40 communities, spread over all the words)
        keys = edge_list(rng, N, 40000)
        what = "cut K=%d" % K
        base = cs.statement(cs.members(host, THR), keys)
        mask = b.links.mask(b.matrix(host), float(F32(THR)))
        one = b.run(mask, N, K, base["csr"], what)
        cuts = [(2000, N - 2000), (0, 991), (991, 1009)]
        three = b.run(mask, N, K, base["csr"], what + " in three", node_cuts=cuts)
        back = b.run(mask, N, K, base["csr"], what + " reversed", node_cuts=cuts[::-1])
        assert same(one, three) and same(one, back), what + ": the pieces differ from one call"
        against(one, base, what)
        assert base["L"] > 1000 and base["degeneracy"].max() >= 2
        print("%s ok: %d entries" % (what, base["L"]), flush=True)
    # 2^18 + 2^10 pairs, every one a community-0 link of its own: all slots leave at level 1, in one peel launch of more than
    # one pass of its grid (2048 blocks of 16 slots)
    pairs = (1 << 18) + (1 << 10)
    N, K = 2 * pairs, 1
    assert 2 * pairs > MAX_GRID * (BLOCK // PEEL_LANES)
    T = b.torch
    mask = T.ones((N, 1), dtype=T.int64, device="cuda")
    offsets = np.arange(N + 1, dtype=np.uint64)
    targets = (np.arange(N, dtype=np.uint32) ^ np.uint32(1))
    got = b.run(mask, N, K, (offsets, targets), "frontier")
    assert (got["core"] == 1).all() and (got["indeg"] == 1).all() and np.array_equal(got["nbr"].view(np.uint32), targets)
    assert got["counts"].view(np.uint64).tolist() == [N, N, 2, 1], got["counts"]      # the scans of 0 (nothing) and 1; one peel
    assert got["degeneracy"].tolist() == [1] and got["nucleus"].tolist() == [N] and got["members"].tolist() == [N]
    print("cut ok: a frontier of %d slots" % N, flush=True)


# ------------------------------------------------------------------------------------------------------------ contend
def contend_group():
    """N = 2048, every node in the communities 0 .. 7, 2 10^5 random keys: the same deg words are lowered from all XCDs"""
    b = Bench()
    rng = np.random.default_rng(59)
    N, K, n = 2048, 8, 200_000
    host = np.full((N, K), 0.5, F32)
    a, c = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    keys = (a << np.uint64(32)) | c
    base = cs.statement(np.ones((N, K), bool), keys)
    mask = b.links.mask(b.matrix(host), float(F32(THR)))
    got = b.run(mask, N, K, base["csr"], "contend")
    against(got, base, "contend")
    core = got["core"].view(np.uint32).reshape(N, K)
    assert (core == core[:, :1]).all() and core.max() > 50 and np.unique(core).size > 5
    for name in cs.PER_COMMUNITY:
        assert (got[name] == got[name][0]).all(), name
    print("contend ok: degeneracy %d, %d entries" % (core.max(), base["L"]), flush=True)


# ------------------------------------------------------------------------------------------------------------ cross
def cross_group():
    """through the learner on one edge list, against the other analyses and against the cores of the whole graph"""
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    lrn.Run(5)
    lrn.drain()
    co = lrn._cores().co
    rng = np.random.default_rng(41)
    keys = edge_list(rng, N, 30000)
    r = lrn.CommunityCores(0.05, edges=keys)
    same_result(r, cs.result_of(co, 0.05, cs.statement(cs.members(lrn.pi.host(), 0.05), keys)), "fitted pi")
    lrn.pi.load(np.where(rng.random((N, K)) < 0.1, 0.3, 0.0).astype(F32))
    thr = 0.25
    r = lrn.CommunityCores(thr, edges=keys)
    assert np.array_equal(r.members, lrn.CommunitySizes(thr).cpu().numpy().astype(np.uint64))
    # the simple list: every link once
    off, tgt, skipped, dropped = cs.simple_csr(keys, N)
    src = np.repeat(np.arange(N), np.diff(off.astype(np.int64)))
    once = src < tgt
    simple = (src[once].astype(np.uint64) << np.uint64(32)) | tgt[once].astype(np.uint64)
    assert (r.skipped, r.dropped) == (skipped, dropped) and skipped > 100 and dropped > 0
    roles = lrn.NodeRoles(thr, edges=simple, top=16, among="own")
    assert np.array_equal(r.inlinks2, roles.ksum)
    q = lrn.CommunityQuality(thr, edges=simple)
    assert np.array_equal(r.inlinks2, 2 * np.asarray(q.internal).astype(np.uint64))
    assert np.array_equal(r.isolated, lrn.CommunityComponents(thr, edges=simple).singletons)
    # a corner of a triangle inside k lies in a 2-core of k: a node with tri_comms > 0 has a membership of core >= 2, and a
    # community with a triangle inside has degeneracy >= 2
    # (on a list dense enough to hold such triangles: 8000 keys among 400 nodes)
    dense = edge_list(rng, 400, 8000)
    tri, rd = lrn.Triangles(thr, edges=dense), lrn.CommunityCores(thr, edges=dense)
    assert (rd.best_core[tri.tri_comms > 0] >= 2).all() and (tri.tri_comms > 0).sum() > 10
    assert (rd.degeneracy[tri.ktri3 > 0] >= 2).all() and (tri.ktri3 > 0).sum() > 10    # every node in community 0: the core numbers of the whole graph
    host = np.zeros((N, K), F32)
    host[:, 0] = 1.0
    lrn.pi.load(host)
    r = lrn.CommunityCores(0.5, edges=keys)
    whole = cs.statement(np.ones((N, 1), bool), keys)
    assert np.array_equal(r.core, whole["core"]) and np.array_equal(r.indeg, whole["indeg"]) and r.degeneracy[0] == whole["degeneracy"][0]
    assert not r.members[1:].any() and r.nucleus_share[1] == -1.0 and np.array_equal(r.best_core, whole["core"])
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    e = ps.rejects(AmmsbError, (lambda: lrn.CommunityCores(0.5, edges=keys, max_bytes=4 * r.L - 4),))
    assert str(4 * r.L - 4) in str(e[0]) and "threshold 0.5" in str(e[0])
    lrn.close()
    print("cross ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ deep
def deep_group():
    """slot ids past 2^31 in queue and nbr: K = 8192 at thr = 0 over a zeroed pi of 2^18 + 64 rows, so every node has 8192
    slots and M = 2^31 + 2^19; keys among the first 64 and the last 64 nodes.  Checked on the device."""
    b = Bench()
    T = b.torch
    K, N = 8192, (1 << 18) + 64
    M = N * K
    assert M == (1 << 31) + (1 << 19)
    rng = np.random.default_rng(61)
    ids = np.concatenate((np.arange(64), np.arange(N - 64, N)))
    pairs = np.concatenate((rng.integers(0, 64, (60, 2)), rng.integers(64, 128, (200, 2)), rng.integers(0, 128, (8, 2))))
    keys_c = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    keys = (ids[pairs[:, 0]].astype(np.uint64) << np.uint64(32)) | ids[pairs[:, 1]].astype(np.uint64)
    want = cs.statement(np.ones((128, 1), bool), keys_c)
    # a slot id wrapped at 2^31 lands the last 64 nodes on the first 64
    alias = pairs % 64
    wrapped = cs.statement(np.ones((64, 1), bool), (alias[:, 0].astype(np.uint64) << np.uint64(32)) | alias[:, 1].astype(np.uint64))
    assert want["degeneracy"][0] >= 2 and not np.array_equal(want["core"][:64], wrapped["core"])
    offsets, targets, _, _ = cs.simple_csr(keys, N)
    pi, _ = b.zeroed(N, K)
    st, base, gotM, slot_comm, indeg, nbr_off, nbr = b.api.run(pi, 0.0, *b.csr((offsets, targets)), max_bytes=1 << 30)
    del pi
    b.release()
    assert gotM == M and int(base[-1]) == M and int(nbr_off[-1]) == K * want["L"] == nbr.numel()
    counts = st["counts"].cpu().numpy().view(np.uint64).tolist()
    assert counts[:2] == [M, K * want["L"]] and counts[2] <= 2 * np.unique(want["core"]).size + 1 and counts[3] <= 130, counts
    lo, hi = 64 * K, (N - 64) * K
    core = st["deg"]
    for at in range(lo, hi, 1 << 28):
        end = min(hi, at + (1 << 28))
        assert not bool(core[at:end].any()) and not bool(indeg[at:end].any()), "slots from %d" % at
    for sl, at in ((slice(0, lo), 0), (slice(hi, M), 64)):
        for name, t in (("core", core), ("indeg", indeg)):
            assert np.array_equal(t[sl].cpu().numpy().reshape(64, K), np.repeat(want[name][at:at + 64, None], K, 1).astype(np.int32)), name
    # the neighbours of (a, k) are the slots of (b, k): checked where they lie past 2^31
    row = int(np.flatnonzero(want["indeg"][64:])[0]) + 64
    s = ids[row] * K + 5
    assert s >= 1 << 31
    first = int(nbr_off[s])
    got = nbr[first:first + int(want["indeg"][row])].cpu().numpy().view(np.uint32).astype(np.int64)
    lo_c = int(want["nbr_off"][row])
    assert np.array_equal(got, ids[want["nbr"][lo_c:lo_c + got.size].astype(np.int64)] * K + 5) and got.max() >= 1 << 31
    queue = st["queue"]
    assert bool(((queue[-(1 << 20):].to(T.int64) & 0xFFFFFFFF) < M).all())
    assert bool(((queue[-(1 << 20):].to(T.int64) & 0xFFFFFFFF) >= 1 << 31).any())   # ids past 2^31 went through the queue
    h = lambda n: st[n].cpu().numpy()   # noqa: E731
    top = int(want["degeneracy"][0])
    assert (h("members") == N).all() and (h("degeneracy") == top).all() and (h("nucleus") == int(want["nucleus"][0])).all()
    assert (h("isolated") == N - 128 + int(want["isolated"][0])).all() and (h("inlinks2") == want["L"]).all()
    best = np.zeros(N, np.int64)
    best[ids] = want["core"]
    assert np.array_equal(h("best_core").astype(np.int64), best) and (h("best_comm") == 0).all()
    inner = np.zeros(N, np.int64)
    inner[ids[want["core"] == top]] = K
    assert np.array_equal(h("in_nucleus").astype(np.int64), inner)
    print("deep ok: %d slots, degeneracy %d, %d scans, %d rounds" % (M, top, counts[2], counts[3]), flush=True)


# ------------------------------------------------------------------------------------------------------------ far
def far_group():
    """library-level calls only: nbr is an uninitialised buffer of 2^30 + 2^16 entries (4 GiB + 256 KiB) and the rows of a
    hand-made small slot graph are planted in it, through nbr_off, in three windows: the start, around byte offset 2^32, and
    the end.  Rows are not packed: the kernels read a row as (nbr_off[s], indeg[s])"""
    b = Bench()
    T = b.torch
    rng = np.random.default_rng(53)
    n, K = 300, 3
    Mb = rng.random((n, K)) < 0.7
    Mb[5] = False
    pairs = np.concatenate((rng.integers(0, n, (2500, 2)), rng.integers(0, 40, (500, 2))))
    base = cs.statement(Mb, (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64))
    M, indeg_h = base["M"], base["indeg"].astype(np.int64)
    assert base["degeneracy"].max() >= 5 and M > 500
    total = (1 << 30) + (1 << 16)
    nbr = T.empty(total, dtype=T.int32, device="cuda")
    assert nbr.numel() * 4 == (1 << 32) + (256 << 10)
    # a third of the slots in each window, every row at a place of its own with a gap before it
    place = np.zeros(M, np.int64)
    third = (M + 2) // 3
    for w, start in enumerate((0, (1 << 30) - int(indeg_h[third:2 * third].sum() + 3 * third) // 2, None)):
        sl = slice(w * third, min(M, (w + 1) * third))
        width = indeg_h[sl] + 3
        if start is None:
            start = total - int(width.sum())
        place[sl] = start + np.cumsum(width) - width + 3
    assert place[0] == 3 and place[-1] + indeg_h[-1] == total and (place[third:2 * third] < 1 << 30).any() and \
        (place[third:2 * third] >= 1 << 30).any()
    idx = np.concatenate([place[s] + np.arange(indeg_h[s]) for s in range(M)])
    nbr[b.dev(idx)] = b.dev(base["nbr"].astype(np.uint32)).view(T.int32)
    nbr_off = b.dev(np.append(place, 0).astype(np.uint64)).view(T.int64)
    indeg = b.dev(base["indeg"]).view(T.int32)
    st = b.api.state(n, K, M, indeg)
    scans, rounds = b.api.peel(M, indeg, nbr_off, nbr, st)
    assert b.api.kernel_name() in ("cores_peel", "cores_scan")
    b.api.finish(n, K, b.dev(base["offsets"]).view(T.int64), M, b.dev(base["community"].view(np.int16)), indeg, st)
    h = lambda name: st[name].cpu().numpy()   # noqa: E731
    assert np.array_equal(h("deg").view(np.uint32), base["core"])
    for name in cs.PER_COMMUNITY + cs.PER_NODE:
        assert np.array_equal(h(name).view(VIEW[name]), base[name]), name
    assert rounds <= M and scans <= 2 * np.unique(base["core"]).size + 1
    print("far ok: %d slots, %d entries in three windows of %d, degeneracy %d" % (M, base["L"], total, int(base["degeneracy"].max())), flush=True)


# ------------------------------------------------------------------------------------------------------------ planted
def planted_group():
    """hostlib's planted graph and cover at N = 10^4, pi set to the planted memberships: equal to the statement, and the mean
    degeneracy over the communities of at least 3 members is larger than with the node ids permuted (verified on the CPU
    with the statement for this seed first, then asserted of the device result)"""
    from mcmc_ammsb_gpu_amd import hostlib
    b = Bench()
    N, K = 10_000, 32
    keys = np.ascontiguousarray(hostlib.generate_graph(N, K, 32, seed=20260101), dtype=np.uint64)
    offsets, mem = hostlib.generate_cover(N, K, seed=20260101)
    M = np.zeros((N, K), dtype=bool)
    for k in range(K):
        M[mem[int(offsets[k]):int(offsets[k + 1])], k] = True
    host = np.where(M, (1.0 / np.maximum(M.sum(axis=1), 1))[:, None], 0.0).astype(F32)
    assert np.array_equal(cs.members(host, THR), M) and keys.size > 100_000
    mask = b.links.mask(b.matrix(host), float(F32(THR)))
    perm = np.random.default_rng(43).permutation(N).astype(np.uint64)
    a, c = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    other = (perm[a.astype(np.int64)] << np.uint64(32)) | perm[c.astype(np.int64)]
    mean = lambda s: float(s["degeneracy"][s["members"] >= 3].astype(np.float64).mean())   # noqa: E731
    base, shuffled = cs.statement(M, keys), cs.statement(M, other)
    assert mean(base) > mean(shuffled), (mean(base), mean(shuffled))     # the CPU first
    got, got2 = b.run(mask, N, K, base["csr"], "planted"), b.run(mask, N, K, shuffled["csr"], "permuted")
    against(got, base, "planted")
    against(got2, shuffled, "permuted")
    dev = lambda g: float(g["degeneracy"].view(np.uint32)[g["members"].view(np.uint64) >= 3].astype(np.float64).mean())   # noqa: E731
    assert dev(got) > dev(got2)
    print("planted ok: mean degeneracy %.4f against %.4f permuted" % (dev(got), dev(got2)), flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _cores
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    seen = []

    def calls(a):
        seen.append((a.CommunityCores(), a.pi.host().copy(), a.TrainingLinks().cpu().numpy().view(np.uint64)))
    ps.unperturbed_run(make, calls, "cores")
    r, host, keys = seen[0]
    assert isinstance(r, _cores.Cores) and r.N == N and host.shape == (N, K) and keys.size > 100_000
    same_result(r, cs.result_of(_cores, 0.05, cs.statement(cs.members(host, 0.05), keys)), "learner")
    assert r.skipped == 0 and r.dropped == 0 and r.rounds <= r.M and r.scans <= 2 * np.unique(r.core).size + 1
    lrn = make()
    ps.rejects(AmmsbError, (lambda: lrn.CommunityCores(-1.0), lambda: lrn.CommunityCores(float("nan")),
                            lambda: lrn.CommunityCores(0.05, max_bytes=8)))
    lrn.close()
    print("learner ok graph=%s: %d slots, %d entries, degeneracy up to %d" % (graph, r.M, r.L, int(r.degeneracy.max())), flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def cpp_group():
    """tests/cpp/cores_test.cc: the file WriteCommunityCores writes equals, byte for byte, write_cores of the statement over
    the checkpoint's pi and the training links of the link-communities file the same process wrote"""
    import os
    import tempfile
    from mcmc_ammsb_gpu_amd import _cores, _linkcomm
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("cores_test", d, 300)
        path = os.path.join(d, "cores.txt")
        r = _cores.read_cores(path)
        K, thr = 64, 0.05
        assert r.N == 20000 and r.members.size == K and F32(r.threshold) == F32(thr)
        pi, _ = ps.pi_beta_of_checkpoint(open(os.path.join(d, "cpp.ckpt"), "rb").read(), r.N, K)
        keys = np.ascontiguousarray(_linkcomm.read_link_communities(os.path.join(d, "links.txt"))[4], dtype=np.uint64)
        assert keys.size > 1000 and r.skipped == 0 and r.dropped == 0
        again = path + ".py"
        _cores.write_cores(again, cs.result_of(_cores, thr, cs.statement(cs.members(pi, thr), keys)))
        assert open(again, "rb").read() == open(path, "rb").read(), "the file is not write_cores of the statement"
        print("cpp ok: %d slots, %d entries, degeneracy up to %d" % (r.M, r.L, int(r.degeneracy.max())), flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "cut": lambda a: cut_group(),
    "contend": lambda a: contend_group(),
    "cross": lambda a: cross_group(),
    "deep": lambda a: deep_group(),
    "far": lambda a: far_group(),
    "planted": lambda a: planted_group(),
    "learner": lambda a: learner_group(a[0] == "1"),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
