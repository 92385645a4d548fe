"""Child process of test_gpu_components.py (one per group): the connected components of every detected community
(include/ammsb_components.h, ops.CommunityComponents, Learner.CommunityComponents) against the statement of the header's
definitions, which components_statement.py writes once and test_components_host.py checks on the CPU against boolean
powers of the dense induced adjacency.  Every device integer is asserted equal; the float64 fields, one host formula over
equal integers, are bit-equal.  There is no tolerance in this file."""
import ctypes as C
import sys

import numpy as np

import components_statement as cs
import postfit_support as ps
from modularity_child import edge_list

FILL = {np.dtype(np.int16): 0x5A5A, np.dtype(np.int32): 0x5A5A5A5A, np.dtype(np.int64): 0x5A5A5A5A5A5A5A5A}
F32 = np.float32
# the kernels' constants (csrc/ammsb_components.hip, csrc/ammsb_postfit.h)
WAVES, MAX_GRID = 4, 2048
OUT = cs.PER_COMMUNITY + cs.PER_SLOT + ("stray",)
VIEW = {"members": np.uint64, "components": np.uint64, "singletons": np.uint64, "largest": np.uint32,
        "largest_root": np.int32, "community": np.uint16, "root": np.uint32, "size": np.uint32, "stray": np.uint32}


def key(a, b):
    return (int(a) << 32) | int(b)


class Bench(ps.DeviceBench):
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _components
        super().__init__()
        self.cc = _components
        self.lib = _components.load()
        self.api = self.ops.CommunityComponents(self.ctx)
        self.links = self.ops.CommunityLinks(self.ctx)

    def run(self, mask, N, K, pieces, what, node_cuts=None):
        """the four calls over guarded buffers, the list in `pieces` -> name -> host array"""
        T = self.torch
        ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731
        want = lambda name: "components_%s_w%d" % (name, 1 if K <= self.cc.W1_MAX_COLS else 2)   # noqa: E731
        own = self.guarded(N, T.int32, FILL[np.dtype(np.int32)])
        self.cc.check(self.lib.ammsb_components_own(ptr(mask), N, K, ptr(own), None))
        assert self.cc.last_kernel_name() == want("own"), self.cc.last_kernel_name()
        base, M = self.api.base(own[:N])
        sizes = {"slot_node": (M, T.int32), "slot_comm": (M, T.int16), "parent": (M, T.int32), "root": (M, T.int32),
                 "size": (M, T.int32), "members": (K, T.int64), "components": (K, T.int64), "singletons": (K, T.int64),
                 "best": (K, T.int64), "largest": (K, T.int32), "largest_root": (K, T.int32), "stray": (N, T.int32),
                 "counts": (4, T.int64)}
        zeroed = ("members", "components", "singletons", "best", "counts")
        fill = lambda dt: FILL[np.dtype(str(dt).split(".")[1])]   # noqa: E731
        buf = {n: self.guarded(w, dt, fill(dt), zero=n in zeroed) for n, (w, dt) in sizes.items()}
        for first, count in node_cuts or [(0, N)]:
            self.cc.check(self.lib.ammsb_components_slots(ptr(mask), N, K, ptr(base), M, first, count, ptr(buf["slot_node"]),
                                                          ptr(buf["slot_comm"]), ptr(buf["parent"]), None))
        assert self.cc.last_kernel_name() == want("slots"), self.cc.last_kernel_name()
        for keys in pieces:
            d = self.dev(np.ascontiguousarray(keys, dtype=np.uint64)) if len(keys) else None
            self.cc.check(self.lib.ammsb_components_edges(ptr(mask), N, K, ptr(base), M, ptr(d) if d is not None else None,
                                                          len(keys), ptr(buf["parent"]), ptr(buf["counts"]), None))
            if len(keys):
                assert self.cc.last_kernel_name() == want("edges"), self.cc.last_kernel_name()
        self.cc.check(self.lib.ammsb_components_finish(
            N, K, ptr(base), M, *[ptr(buf[n]) for n in ("slot_node", "slot_comm", "parent", "root", "size", "members",
                                                        "components", "singletons", "best", "largest", "largest_root", "stray",
                                                        "counts")], None))
        assert self.cc.last_kernel_name() == "components_finish_stray"
        out = {"own": own.cpu().numpy()}
        buf["own"], sizes["own"] = own, (N, T.int32)
        for n, t in buf.items():
            host = t.cpu().numpy()
            words = sizes[n][0]
            assert (host[words:] == host.dtype.type(FILL[host.dtype])).all() and host.size == words + ps.GUARD, \
                "%s: the words past %s were written" % (what, n)
            out[n] = host[:words].copy()
        out["offsets"], out["community"] = base.cpu().numpy().view(np.uint64), out["slot_comm"]
        return out


def against(got, base, what):
    assert np.array_equal(got["offsets"], base["offsets"]), what + ": offsets differ"
    assert np.array_equal(got["own"].view(np.uint32), np.diff(base["offsets"].astype(np.int64))), what + ": own differs"
    for n in OUT:
        assert np.array_equal(got[n].view(VIEW[n]), base[n]), "%s: %s differs" % (what, n)
    slot_node = np.repeat(np.arange(base["offsets"].size - 1), np.diff(base["offsets"].astype(np.int64)))
    assert np.array_equal(got["slot_node"].view(np.uint32), slot_node), what + ": slot_node differs"
    counts = got["counts"].view(np.uint64).tolist()
    assert counts == [base["links"], base["skipped"], base["shared"], 0], "%s: counts %s" % (what, counts)


def same(x, y):
    return all(np.array_equal(x[n], y[n]) for n in x if n != "parent")   # (the forest's shape is the one thing that may differ)


def same_result(r, want, what):
    for n in OUT + ("offsets",):
        assert np.array_equal(getattr(r, n), getattr(want, n)), "%s: %s differs" % (what, n)
    for n in ("links", "skipped", "shared", "M", "N"):
        assert getattr(r, n) == getattr(want, n), "%s: %s is %s, not %s" % (what, n, getattr(r, n), getattr(want, n))
    for n in ("giant", "fragmentation"):
        assert getattr(r, n).tobytes() == getattr(want, n).tobytes(), "%s: %s is not bit-equal" % (what, n)
    assert np.float64(r.connected).tobytes() == np.float64(want.connected).tobytes(), what
    assert np.array_equal(r.disconnected(), want.disconnected()), what
    for f in ("cover", "trimmed"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(r, f)(), getattr(want, f)())), "%s: %s differs" % (what, f)


# ------------------------------------------------------------------------------------------------------------ exact
# K: W = 1, 1, 1, 2, 4, 16, 64 and then the two-word form; K = 65 and 4160 have a last word with unused bits
EXACT_K = (1, 5, 64, 65, 256, 1024, 4096, 4160, 8192)
EXACT_N, THR = 6000, 0.05
PATH, CENTRE, LONE = 5000, 5000, 5999
A, B, VIA = range(5100, 5120), range(5120, 5140), 5150
QUIET, TIE, MANY = range(5300, 5400), ((5400, 5401, 5402), (5410, 5411, 5412)), range(5500, 5510)


def clique(nodes):
    nodes = list(nodes)
    return [key(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def exact_graph():
    """the path 0 .. 4999 with its keys ascending, descending and shuffled; the star of centre 5000 over the same 5000 nodes;
    the cliques A and B joined through VIA; QUIET without a key among its nodes; two triangles (the tie); a ring over MANY; a ==
    a keys, repeats, both orders of the ends, ends >= N; random keys among the path's nodes"""
    rng = np.random.default_rng(5)
    step = [key(i, i + 1) for i in range(PATH - 1)]
    keys = step + step[::-1] + [key(i + 1, i) for i in rng.permutation(PATH - 1)]
    keys += [key(CENTRE, i) if i % 2 else key(i, CENTRE) for i in range(PATH)]
    keys += clique(A) + clique(B) + [key(A[-1], VIA), key(VIA, B[0])]
    keys += [key(q, int(rng.integers(0, PATH))) for q in QUIET]
    for t in TIE:
        keys += clique(t)
    keys += [key(MANY[i], MANY[(i + 1) % len(MANY)]) for i in range(len(MANY))]
    keys += [key(7, 7), key(A[0], A[0]), key(5, 6), key(6, 5), key(EXACT_N, 3), key(3, 2 ** 32 - 1), key(EXACT_N + 9, EXACT_N)]
    noise = edge_list(rng, PATH, 20000)              # (among the path's nodes; its ends "past" are 5000, 5005 and 2^32 - 1)
    keys = np.concatenate((np.array(keys, dtype=np.uint64), noise))
    assert keys.size < 60000
    return keys


def exact_cover(rng, K):
    """c[i] = i % K for the planted communities: 0 the path, 1 the star, 2 the cliques without VIA, 3 the cliques with VIA, 4
    QUIET, 5 the tie; MANY share K - 1, K - 3 (inside the last word), K // 2 (another word) and 6; K - 2 stays empty; a
    sparse random background in the communities 8 .. K - 9 with values equal to thr planted, NaNs everywhere.  Below K = 64 the
    planted communities fall on each other, and the statement says what then holds."""
    N = EXACT_N
    host = (rng.random((N, K)) * 0.9 * THR).astype(F32)
    lo, hi = (8, K - 8) if K >= 64 else (0, K)
    for _ in range(2):
        host[np.arange(N), rng.integers(lo, hi, N)] = F32(0.3)
    host[rng.integers(0, N, 400), rng.integers(lo, hi, 400)] = F32(THR)
    host[rng.integers(0, N, 400), rng.integers(0, K, 400)] = np.nan
    c = [i % K for i in range(7)]
    host[:PATH, c[0]] = 0.9
    host[:PATH + 1, c[1]] = 0.8
    for k, extra in ((c[2], []), (c[3], [VIA])):
        host[list(A) + list(B) + extra, k] = 0.7
    host[list(QUIET), c[4]] = 0.6
    host[[n for t in TIE for n in t], c[5]] = F32(THR)
    for k in (K - 1, max(0, K - 3), K // 2, c[6]):
        host[list(MANY), k] = 0.5
    if K >= 64:
        host[VIA, c[2]] = np.nan
        host[:, K - 2] = F32(0.5) * F32(THR)
    host[LONE] = F32(0.5) * F32(THR)
    return host


def exact_properties(base, K):
    """what the planted graph is there for, read off the statement (K >= 64: the planted communities are apart)"""
    off = base["offsets"].astype(np.int64)

    def at(a, k):
        s = np.flatnonzero(base["community"][off[a]:off[a + 1]] == k)
        return (int(base["root"][off[a] + s[0]]), int(base["size"][off[a] + s[0]])) if s.size else None

    assert at(PATH - 1, 0) == (0, PATH) and at(17, 1) == (0, PATH + 1)
    assert at(A[3], 2) == (A[0], 20) and at(B[3], 2) == (B[0], 20) and at(VIA, 2) is None     # the key through a non-member
    assert at(B[3], 3) == (A[0], 41) and at(VIA, 3) == (A[0], 41)
    assert base["singletons"][4] == base["components"][4] == base["members"][4] == len(QUIET)
    assert base["members"][K - 2] == 0 and base["largest_root"][K - 2] == -1 and base["largest"][K - 2] == 0
    assert off[LONE + 1] == off[LONE] and base["stray"][LONE] == 0
    assert at(TIE[1][2], 5) == (TIE[1][0], 3) and base["largest"][5] == 3 and base["largest_root"][5] == TIE[0][0]
    assert base["stray"][TIE[1][0]] >= 1
    for k in (K - 1, K - 3, K // 2, 6):
        assert at(MANY[4], k) == (MANY[0], len(MANY))
    assert base["skipped"] > 100 and base["shared"] > base["links"] // 2


def refused(b, mask, N, K):
    """what every call refuses with AMMSB_EINVAL before anything is launched: no output changes"""
    T = b.torch
    ptr = lambda x, o=0: C.c_void_p(x.data_ptr() + o)   # noqa: E731
    own = b.api.own(mask, N, K)
    base, M = b.api.base(own)
    st = b.api.state(N, K, M)
    for t in list(st.values()) + [own]:
        t.fill_(77)
    keys = b.dev(np.array([key(1, 2)], dtype=np.uint64))
    L = b.lib
    slot = lambda **kw: [kw.get("mask", ptr(mask)), kw.get("N", N), kw.get("K", K), ptr(base), kw.get("M", M)]   # noqa: E731
    fin = [ptr(st[n]) for n in ("slot_node", "slot_comm", "parent", "root", "size", "members", "components", "singletons",
                                "best", "largest", "largest_root", "stray", "counts")]
    calls = [
        lambda: L.ammsb_components_own(ptr(mask), N, 0, ptr(own), None),
        lambda: L.ammsb_components_own(ptr(mask), N, 8193, ptr(own), None),
        lambda: L.ammsb_components_own(ptr(mask), 1 << 32, K, ptr(own), None),
        lambda: L.ammsb_components_own(None, N, K, ptr(own), None),
        lambda: L.ammsb_components_own(ptr(mask, 4), N, K, ptr(own), None),
        lambda: L.ammsb_components_own(ptr(mask), N, K, ptr(own, 2), None),
        lambda: L.ammsb_components_slots(*slot(), N - 1, 2, ptr(st["slot_node"]), ptr(st["slot_comm"]), ptr(st["parent"]), None),
        lambda: L.ammsb_components_slots(*slot(M=1 << 32), 0, N, ptr(st["slot_node"]), ptr(st["slot_comm"]), ptr(st["parent"]), None),
        lambda: L.ammsb_components_slots(*slot(), 0, N, ptr(st["slot_node"]), ptr(st["slot_comm"], 1), ptr(st["parent"]), None),
        lambda: L.ammsb_components_slots(*slot(), 0, N, ptr(st["slot_node"]), ptr(st["slot_comm"]), None, None),
        lambda: L.ammsb_components_edges(*slot(), ptr(keys), 1 << 31, ptr(st["parent"]), ptr(st["counts"]), None),
        lambda: L.ammsb_components_edges(*slot(), None, 1, ptr(st["parent"]), ptr(st["counts"]), None),
        lambda: L.ammsb_components_edges(*slot(), ptr(keys), 1, ptr(st["parent"]), None, None),
        lambda: L.ammsb_components_edges(*slot(), ptr(keys), 1, ptr(st["parent"]), ptr(st["counts"], 4), None),
        lambda: L.ammsb_components_edges(*slot(K=0), ptr(keys), 1, ptr(st["parent"]), ptr(st["counts"]), None),
        lambda: L.ammsb_components_finish(N, K, ptr(base), 1 << 32, *fin, None),
        lambda: L.ammsb_components_finish(N, K, None, M, *fin, None),
        lambda: L.ammsb_components_finish(N, K, ptr(base), M, *(fin[:9] + [None] + fin[10:]), None),
        lambda: L.ammsb_components_finish(N, K, ptr(base), M, *(fin[:3] + [ptr(st["root"], 2)] + fin[4:]), None),
    ]
    for i, call in enumerate(calls):
        rc = call()
        assert rc != 0 and b.cc._LIBRARY._call("last_error"), "bad call %d was accepted" % i
    T.cuda.synchronize()
    assert all(bool((t == 77).all()) for t in list(st.values()) + [own]), "a refused call changed an output"
    return len(calls)


def exact_group(which):
    b = Bench()
    keys = exact_graph()
    rng = np.random.default_rng(31)
    thr = float(F32(THR))
    N = EXACT_N
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
        got = b.run(mask, N, K, [keys], what)
        against(got, base, what)
        assert same(got, b.run(mask, N, K, [keys], what)), what + ": two runs differ"
        if K % 64:   # garbage in the bits past K of every last word
            dirty = mask.clone().reshape(N, -1)
            dirty[:, -1] |= b.ctx.from_numpy(np.array([(~((1 << (K % 64)) - 1)) & (2 ** 64 - 1)], dtype=np.uint64))[0]
            assert not b.torch.equal(dirty, mask.reshape(N, -1))
            assert same(got, b.run(dirty.reshape(mask.shape).contiguous(), N, K, [keys], what)), what + ": bits past K changed the result"
        # an empty list: every member a component of its own
        none = b.run(mask, N, K, [[]], what + " no key")
        against(none, cs.statement(M, np.zeros(0, np.uint64)), what + " no key")
        assert np.array_equal(none["singletons"], none["members"]) and (none["size"] == 1).all()
        print("exact %s: %d slots, %d components, %d unions" % (what, got["root"].size, int(base["components"].sum()), base["shared"]),
              flush=True)
    if not which or 2 in which:
        K = 64
        host = (rng.random((N, K)) * 0.5).astype(F32)   # thr = 0: every stored number but a NaN is a member
        host[rng.integers(0, N, 50), rng.integers(0, K, 50)] = np.nan
        M = cs.members(host, 0.0)
        assert M.sum() > N * K - 51
        mask = b.links.mask(b.matrix(host), 0.0)
        against(b.run(mask, N, K, [keys], "thr=0"), cs.statement(M, keys), "thr=0")
        print("exact thr=0 ok; %d bad calls refused" % refused(b, mask, N, K), flush=True)
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cut
def sparse_pi(rng, N, K, per_node=3):
    host = np.zeros((N, K), F32)
    for _ in range(per_node):
        host[np.arange(N), rng.integers(0, 40, N) * (K // 40)] = 0.9   # (40 communities, spread over all the words)
    return host


def cut_group():
    """more keys than one pass of the persistent grid (2048 blocks of 4 waves, an edge per wave at W = 64 and above): in one
    call, in three ragged pieces, and the pieces in reverse order; the slots in one call and in three node ranges"""
    b = Bench()
    rng = np.random.default_rng(37)
    for N, K in ((3000, 4096), (3000, 8192)):
        n = 20000
        assert n > MAX_GRID * WAVES
        host = sparse_pi(rng, N, K)
        keys = edge_list(rng, N, n)
        what = "cut K=%d" % K
        mask = b.links.mask(b.matrix(host), float(F32(THR)))
        one = b.run(mask, N, K, [keys], what)
        c1, c2 = n // 3 - 7, 2 * n // 3 + 5
        pieces = [keys[:c1], keys[c1:c2], keys[c2:]]
        three = b.run(mask, N, K, pieces, what + " in three", node_cuts=[(2000, N - 2000), (0, 991), (991, 1009)])
        back = b.run(mask, N, K, pieces[::-1], what + " reversed")
        assert same(one, three) and same(one, back), what + ": the pieces differ from one call"
        base = cs.statement(cs.members(host, THR), keys)
        against(one, base, what)
        assert base["shared"] > 1000 and (base["largest"] > 10).any()
        print("%s ok: %d unions" % (what, base["shared"]), flush=True)
    print("cut ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ contend
def contend_group():
    """N = 4096, every node in the communities 0 .. 7, 2 10^5 random keys: every union of a community meets the same few
    roots, from all XCDs"""
    b = Bench()
    rng = np.random.default_rng(59)
    N, K, n = 4096, 8, 200_000
    host = np.full((N, K), 0.5, F32)
    a, c = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
    keys = (a << np.uint64(32)) | c
    mask = b.links.mask(b.matrix(host), float(F32(THR)))
    got = b.run(mask, N, K, [keys], "contend")
    # the statement on one community: the eight are the same sets over the same keys
    one = cs.statement(np.ones((N, 1), bool), keys)
    assert one["components"][0] == 1 and one["largest"][0] == N and one["shared"] == n
    assert got["counts"].view(np.uint64).tolist() == [n, 0, 8 * n, 0]
    assert (got["root"] == 0).all() and (got["size"].view(np.uint32) == N).all() and not got["stray"].any()
    for name in cs.PER_COMMUNITY:
        assert np.array_equal(got[name].view(VIEW[name]), np.repeat(one[name], K)), name
    assert np.array_equal(got["community"].view(np.uint16), np.tile(np.arange(K, dtype=np.uint16), N))
    print("contend ok: %d unions" % (8 * n), flush=True)


# ------------------------------------------------------------------------------------------------------------ cross
def cross_group():
    """through the learner on one edge list, against the other analyses and against covers whose answer is known"""
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    lrn.Run(5)
    lrn.drain()
    cc = lrn._components().cc
    rng = np.random.default_rng(41)
    keys = edge_list(rng, N, 30000)
    r = lrn.CommunityComponents(0.05, edges=keys)
    assert np.array_equal(r.members, lrn.CommunitySizes(0.05).cpu().numpy().astype(np.uint64))
    sc = lrn.SharedCommunities(keys, 0.05).cpu().numpy().astype(np.int64)
    assert r.shared == int(sc[sc >= 0].sum()) and r.skipped == int((sc < 0).sum()) > 100
    same_result(r, cs.result_of(cc, 0.05, cs.statement(cs.members(lrn.pi.host(), 0.05), keys)), "fitted pi")
    # a partition: each induced subgraph alone
    part = rng.integers(0, K, N)
    host = np.zeros((N, K), F32)
    host[np.arange(N), part] = 1.0
    lrn.pi.load(host)
    r = lrn.CommunityComponents(0.5, edges=keys)
    a, c = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (c < N)
    for k in range(K):
        ids = np.flatnonzero(part == k)
        new = np.full(N, -1, np.int64)
        new[ids] = np.arange(ids.size)
        keep = ok.copy()
        keep[ok] = (part[a[ok]] == k) & (part[c[ok]] == k)
        alone = cs.statement(np.ones((ids.size, 1), bool), (new[a[keep]].astype(np.uint64) << np.uint64(32)) | new[c[keep]].astype(np.uint64))
        assert (int(r.components[k]), int(r.largest[k]), int(r.singletons[k])) == \
            (int(alone["components"][0]), int(alone["largest"][0]), int(alone["singletons"][0])), "community %d" % k
        assert int(r.largest_root[k]) == int(ids[alone["largest_root"][0]])
        assert int(r.size[r.community == k].astype(np.int64).sum()) == int(alone["size"].astype(np.int64).sum())   # the sum of the squares
    assert r.M == N and (np.diff(r.offsets.astype(np.int64)) == 1).all()
    # every node in community 0: the components of the whole graph
    host[:] = 0
    host[:, 0] = 1.0
    lrn.pi.load(host)
    r = lrn.CommunityComponents(0.5, edges=keys)
    whole = cs.statement(np.ones((N, 1), bool), keys)
    assert np.array_equal(r.root, whole["root"]) and np.array_equal(r.size, whole["size"]) and r.components[0] == whole["components"][0]
    assert not r.members[1:].any() and (r.largest_root[1:] == -1).all() and r.giant[1] == -1.0
    # singletons against the node roles: a member without a neighbour inside is a singleton; a loop is a neighbour there and
    # joins nothing here, so the two are equal on a list without loops
    lrn.pi.load(np.where(rng.random((N, K)) < 0.1, 0.3, 0.0).astype(F32))
    for lst, equal in ((keys, False), (keys[a != c], True)):
        r = lrn.CommunityComponents(0.25, edges=lst)
        roles = lrn.NodeRoles(0.25, edges=lst, top=16, among="own")
        M = cs.members(lrn.pi.host(), 0.25)
        assert int(M.sum(axis=1).max()) <= 16
        seen = np.zeros((N, K), bool)               # (a, k): k is a's own and c[a, k] > 0
        rows, slots = np.nonzero(roles.home >= 0)
        hit = roles.hcount[rows, slots] > 0
        seen[rows[hit], roles.home[rows[hit], slots[hit]]] = True
        lonely = (M & ~seen).sum(axis=0)
        assert (lonely <= r.singletons).all() and (not equal or np.array_equal(r.singletons, lonely.astype(np.uint64)))
    lrn.close()
    print("cross ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ deep
def deep_group():
    """slot ids past 2^31 and byte offsets of parent past 2^32: K = 8192 at thr = 0 over a zeroed pi of 2^18 + 64 rows, so
    every node has 8192 slots and M = 2^31 + 2^19; keys among the first 64 and the last 64 nodes"""
    b = Bench()
    T = b.torch
    K, N = 8192, (1 << 18) + 64
    M = N * K
    assert M == (1 << 31) + (1 << 19)
    rng = np.random.default_rng(61)
    first, last = np.arange(64), np.arange(N - 64, N)
    ids = np.concatenate((first, last))
    pairs = np.concatenate((rng.integers(0, 64, (40, 2)), rng.integers(64, 128, (120, 2)), rng.integers(0, 128, (8, 2))))
    keys_c = (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64)
    keys = (ids[pairs[:, 0]].astype(np.uint64) << np.uint64(32)) | ids[pairs[:, 1]].astype(np.uint64)
    want = cs.statement(np.ones((128, 1), bool), keys_c)
    # a slot id wrapped at 2^31, or a byte offset 4 s wrapped at 2^32, lands the last 64 nodes on the first 64
    alias = pairs % 64
    wrapped = cs.statement(np.ones((128, 1), bool), (alias[:, 0].astype(np.uint64) << np.uint64(32)) | alias[:, 1].astype(np.uint64))
    assert not np.array_equal(want["root"], wrapped["root"]) and want["components"][0] != wrapped["components"][0]
    root_c, size_c = ids[want["root"].astype(np.int64)], want["size"].astype(np.int64)   # per planted node, in every community
    big = int(size_c.max())
    big_root = int(root_c[size_c == big].min())
    pi, _ = b.zeroed(N, K)
    st, base, gotM = b.api.run(pi, 0.0, keys)
    del pi
    b.release()
    assert gotM == M and int(base[-1]) == M
    counts = st["counts"].cpu().numpy().view(np.uint64).tolist()
    assert counts == [keys.size, 0, K * keys.size, 0], counts
    # every slot outside the planted nodes: a singleton whose root is its node; checked on the device in pieces
    lo, hi = 64 * K, (N - 64) * K
    for at in range(lo, hi, 1 << 27):
        end = min(hi, at + (1 << 27))
        s = T.arange(at, end, dtype=T.int64, device="cuda")
        assert bool((st["root"][at:end] == (s >> 13).to(T.int32)).all()) and bool((st["size"][at:end] == 1).all()), "slots from %d" % at
        assert bool((st["slot_comm"][at:end] == (s & 8191).to(T.int16)).all())
        del s
    for nodes, sl in ((first, slice(0, lo)), (last, slice(hi, M))):
        at = 0 if nodes is first else 64
        assert np.array_equal(st["root"][sl].cpu().numpy().reshape(64, K), np.repeat(root_c[at:at + 64, None], K, 1).astype(np.int32))
        assert np.array_equal(st["size"][sl].cpu().numpy().reshape(64, K), np.repeat(size_c[at:at + 64, None], K, 1).astype(np.int32))
    comps = N - 128 + int(want["components"][0])
    singles = N - 128 + int(want["singletons"][0])
    h = lambda n: st[n].cpu().numpy()   # noqa: E731
    assert (h("members") == N).all() and (h("components") == comps).all() and (h("singletons") == singles).all()
    assert (h("largest") == big).all() and (h("largest_root") == big_root).all()
    stray = np.full(N, K, np.int64)
    stray[ids[root_c == big_root]] = 0
    assert np.array_equal(h("stray").astype(np.int64), stray)
    print("deep ok: %d slots, %d components per community, the largest of %d at node %d" % (M, comps, big, big_root), flush=True)


# ------------------------------------------------------------------------------------------------------------ far
FAR_ROWS, FAR_K, FAR_W = (1 << 22) + 128, 8192, 128
FAR_WINDOWS = ((0, 128), ((1 << 21) - 64, (1 << 21) + 64), ((1 << 22) - 64, FAR_ROWS))


def far_group():
    """a mask past byte offset 2^32: 2^22 + 128 rows of 128 words (4 GiB + 128 KiB), zeroed on the device, planted rows in
    [0, 128), around row 2^21 and around row 2^22, keys inside and across the windows; the statement in the compact
    numbering of the planted rows"""
    b = Bench()
    T = b.torch
    rng = np.random.default_rng(53)
    ids = np.concatenate([np.arange(lo, hi, dtype=np.int64) for lo, hi in FAR_WINDOWS])
    n = ids.size
    hot = np.array([0, 63, 64, 1000, 4095, 4096, 4100, 8000, 8191])    # both words of a lane, both ends of a word
    M = rng.random((n, FAR_K)) < 0.002
    M[:, hot] = rng.random((n, hot.size)) < 0.4
    M[5] = False
    pairs = np.concatenate((rng.integers(0, n, (500, 2)), rng.integers(n - 192, n, (300, 2))))
    base = cs.statement(M, (pairs[:, 0].astype(np.uint64) << np.uint64(32)) | pairs[:, 1].astype(np.uint64))
    keys = (ids[pairs[:, 0]].astype(np.uint64) << np.uint64(32)) | ids[pairs[:, 1]].astype(np.uint64)
    keys = np.concatenate((keys, np.array([key(FAR_ROWS, 3), key(1000, 2000), key(1 << 20, ids[-1])], dtype=np.uint64)))
    mask = T.zeros((FAR_ROWS, FAR_W), dtype=T.int64, device="cuda")
    assert mask.numel() * 8 == (1 << 32) + (128 << 10)
    words = np.packbits(M, axis=1, bitorder="little").view(np.uint64)
    d_ids = b.dev(ids)
    mask[d_ids] = b.dev(words).view(T.int64)
    own = b.api.own(mask, FAR_ROWS, FAR_K)
    assert b.api.kernel_name() == "components_own_w2"
    bs, slots = b.api.base(own)
    st = b.api.state(FAR_ROWS, FAR_K, slots)
    b.api.slots(mask, FAR_ROWS, FAR_K, bs, slots, st)
    b.api.edges(mask, FAR_ROWS, FAR_K, bs, slots, keys, st)
    assert b.api.kernel_name() == "components_edges_w2"
    b.api.finish(FAR_ROWS, FAR_K, bs, slots, st)
    assert slots == int(M.sum()) and np.array_equal(own[d_ids].cpu().numpy(), M.sum(axis=1))
    rest = own.clone()
    rest[d_ids] = 0
    assert int(T.count_nonzero(rest)) == 0, "far: a node elsewhere has slots"
    rest = st["stray"].clone()
    rest[d_ids] = 0
    assert int(T.count_nonzero(rest)) == 0, "far: a node elsewhere is stray"
    h = lambda name: st[name].cpu().numpy()   # noqa: E731
    assert np.array_equal(h("stray")[ids].view(np.uint32), base["stray"])
    assert np.array_equal(h("slot_comm").view(np.uint16), base["community"]) and np.array_equal(h("size").view(np.uint32), base["size"])
    assert np.array_equal(h("root").view(np.uint32), ids[base["root"].astype(np.int64)].astype(np.uint32))
    for name in ("members", "components", "singletons", "largest"):
        assert np.array_equal(h(name).view(VIEW[name]), base[name]), name
    lr = base["largest_root"].astype(np.int64)
    assert np.array_equal(h("largest_root").astype(np.int64), np.where(lr >= 0, ids[np.maximum(lr, 0)], -1))
    assert h("counts").view(np.uint64).tolist() == [base["links"] + 2, 1, base["shared"], 0]
    print("far ok: %d rows, %d slots, %d unions" % (FAR_ROWS, slots, base["shared"]), flush=True)


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
    assert np.array_equal(cs.members(host, THR), M) and keys.size > 100_000
    mask = b.links.mask(b.matrix(host), float(F32(THR)))

    def run(keys, what):
        got = b.run(mask, N, K, [keys], what)
        base = cs.statement(M, keys)
        against(got, base, what)
        return cs.result_of(b.cc, THR, base)

    got = run(keys, "planted")
    planted = float(got.giant[got.members >= 3].mean())
    # the same pi against the same graph with its node ids permuted: the cover no longer fits it (a sign, not a number)
    perm = np.random.default_rng(43).permutation(N).astype(np.uint64)
    a, c = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    other = run((perm[a.astype(np.int64)] << np.uint64(32)) | perm[c.astype(np.int64)], "permuted")
    shuffled = float(other.giant[other.members >= 3].mean())
    assert planted > shuffled, (planted, shuffled)
    print("planted ok: mean giant %.4f against %.4f permuted" % (planted, shuffled), flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def learner_group(graph):
    from mcmc_ammsb_gpu_amd import _components
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    seen = []

    def calls(a):
        seen.append((a.CommunityComponents(), a.pi.host().copy(), a.TrainingLinks().cpu().numpy().view(np.uint64)))
    ps.unperturbed_run(make, calls, "components")
    r, host, keys = seen[0]
    assert isinstance(r, _components.Components) and r.N == N and host.shape == (N, K) and keys.size > 100_000
    same_result(r, cs.result_of(_components, 0.05, cs.statement(cs.members(host, 0.05), keys)), "learner")
    assert r.links == keys.size and r.skipped == 0
    lrn = make()
    ps.rejects(AmmsbError, (lambda: lrn.CommunityComponents(-1.0), lambda: lrn.CommunityComponents(float("nan"))))
    lrn.close()
    print("learner ok graph=%s: %d slots, %d communities in more than one piece" % (graph, r.M, r.disconnected().size), flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def cpp_group():
    """tests/cpp/components_test.cc: the file WriteCommunityComponents writes equals, byte for byte, write_components of the
    statement over the checkpoint's pi and the training links of the link-communities file the same process wrote"""
    import os
    import tempfile
    from mcmc_ammsb_gpu_amd import _components, _linkcomm
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("components_test", d, 300)
        path = os.path.join(d, "components.txt")
        r = _components.read_components(path)
        K, thr = 64, 0.05
        assert r.N == 20000 and r.members.size == K and F32(r.threshold) == F32(thr)
        pi, _ = ps.pi_beta_of_checkpoint(open(os.path.join(d, "cpp.ckpt"), "rb").read(), r.N, K)
        keys = np.ascontiguousarray(_linkcomm.read_link_communities(os.path.join(d, "links.txt"))[4], dtype=np.uint64)
        assert keys.size > 1000 and r.links == keys.size and r.skipped == 0
        again = path + ".py"
        _components.write_components(again, cs.result_of(_components, thr, cs.statement(cs.members(pi, thr), keys)))
        assert open(again, "rb").read() == open(path, "rb").read(), "the file is not write_components of the statement"
        print("cpp ok: %d slots, %d communities in more than one piece" % (r.M, r.disconnected().size), flush=True)


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
