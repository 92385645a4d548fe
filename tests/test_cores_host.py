"""The host side of the community cores (include/ammsb_cores.h, _cores.py): the statement the device tests compare against,
checked here against the definition itself (delete the vertices of degree < c of the dense induced adjacency until nothing
changes) and on hand-made graphs; the float64 derivations and the helpers on hand-made integers; the text file; the
refusals; the built library against its header.  No test here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import cores_statement as cs
from postfit_support import exported_symbols
from test_components_host import random_cover, random_keys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def co():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _cores
    _cores.load()
    return _cores


def key(a, b):
    return (int(a) << 32) | int(b)


def keys_of(pairs):
    return np.array([key(a, b) for a, b in pairs], dtype=np.uint64)


def clique(nodes):
    nodes = list(nodes)
    return [(a, b) for i, a in enumerate(nodes) for b in nodes[i + 1:]]


def core_of(s, a, k):
    """the core number of node a in community k, None where a is no member"""
    off = s["offsets"].astype(np.int64)
    at = np.flatnonzero(s["community"][off[a]:off[a + 1]] == k)
    return int(s["core"][off[a] + at[0]]) if at.size else None


def properties(s):
    """what holds of every slot graph: nbr symmetric and ordered, core <= indeg, core == 0 iff indeg == 0"""
    off, indeg, nbr = s["nbr_off"].astype(np.int64), s["indeg"].astype(np.int64), s["nbr"].astype(np.int64)
    assert np.array_equal(np.diff(off), indeg) and nbr.size == s["L"] == int(indeg.sum())
    src = np.repeat(np.arange(indeg.size), indeg)
    assert (s["community"][src] == s["community"][nbr]).all()                       # a row stays inside its community
    assert np.array_equal(np.sort(src * indeg.size + nbr), np.sort(nbr * indeg.size + src))   # t in row s iff s in row t
    assert ((src[1:] != src[:-1]) | (nbr[1:] > nbr[:-1])).all()                     # rows strictly ascending
    assert (s["core"] <= s["indeg"]).all() and np.array_equal(s["core"] == 0, s["indeg"] == 0)
    assert np.array_equal(s["inlinks2"], np.bincount(s["community"], weights=indeg, minlength=s["members"].size).astype(np.uint64))


def test_the_statement_equals_the_definition():
    rng = np.random.default_rng(7)
    for N, K, n, q in ((1, 1, 3, 1.0), (7, 3, 5, 0.6), (40, 5, 30, 0.5), (200, 8, 150, 0.4), (60, 70, 80, 0.2), (55, 64, 40, 1.0),
                       (30, 65, 200, 0.5), (40, 3, 600, 0.8)):
        M, keys = random_cover(rng, N, K, q), random_keys(rng, N, n)
        s = cs.statement(M, keys)
        want = cs.definitional(M, keys)
        off = s["offsets"].astype(np.int64)
        assert np.array_equal(np.diff(off), M.sum(1)) and s["core"].size == int(M.sum()) == s["M"]
        for a in range(N):
            ks = s["community"][off[a]:off[a + 1]]
            assert np.array_equal(ks, np.flatnonzero(M[a]))          # the communities of a node ascending
            for j, k in enumerate(ks):
                assert int(s["core"][off[a] + j]) == want[k][a], (N, K, a, k)
        for k in range(K):
            cores = list(want[k].values())
            top = max(cores) if cores else 0
            assert int(s["members"][k]) == len(cores) and int(s["degeneracy"][k]) == top
            assert int(s["nucleus"][k]) == sum(1 for c in cores if c == top)
            assert int(s["isolated"][k]) == sum(1 for c in cores if c == 0)
        for a in range(N):
            mine = [(want[k][a], k) for k in np.flatnonzero(M[a])]
            best = max(mine, key=lambda ck: (ck[0], -ck[1])) if mine else (0, -1)
            assert (int(s["best_core"][a]), int(s["best_comm"][a])) == best
            assert int(s["in_nucleus"][a]) == sum(1 for c, k in mine if c > 0 and c == s["degeneracy"][k])
        properties(s)
        a, b = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
        assert s["skipped"] == int(((a >= N) | (b >= N)).sum()) > 0 and (s["dropped"] > 0 or N < 7)
        if K > 2:
            assert s["members"][2] == 0 and s["degeneracy"][2] == 0 and s["nucleus"][2] == 0


def test_the_statement_does_not_depend_on_the_order_of_the_keys_or_on_repeats():
    rng = np.random.default_rng(11)
    M, keys = random_cover(rng, 120, 9, 0.4), random_keys(rng, 120, 300)
    s = cs.statement(M, keys)
    flipped = (keys << np.uint64(32)) | (keys >> np.uint64(32))
    for other in (keys[::-1], rng.permutation(keys), np.unique(keys), flipped, np.concatenate((keys, keys))):
        t = cs.statement(M, other)
        for name in cs.PER_COMMUNITY + cs.PER_SLOT + cs.PER_NODE + ("offsets", "nbr_off", "nbr"):
            assert np.array_equal(s[name], t[name]), name


def test_hand_made_graphs():
    one = lambda n: np.ones((n, 1), bool)   # noqa: E731
    for n in (2, 3, 7, 12):
        s = cs.statement(one(n), keys_of(clique(range(n))))
        assert (s["core"] == n - 1).all() and s["degeneracy"][0] == n - 1 and s["nucleus"][0] == n
    s = cs.statement(one(9), keys_of([(i, i + 1) for i in range(8)]))                       # a path
    assert (s["core"] == 1).all() and s["indeg"].tolist() == [1] + [2] * 7 + [1]
    s = cs.statement(one(9), keys_of([(i, (i + 1) % 9) for i in range(9)]))                 # a cycle
    assert (s["core"] == 2).all()
    s = cs.statement(one(9), keys_of([(0, i) if i % 2 else (i, 0) for i in range(1, 9)]))   # a star
    assert (s["core"] == 1).all() and s["indeg"][0] == 8
    # a K5 with a pendant path
    s = cs.statement(one(9), keys_of(clique(range(5)) + [(4, 5), (5, 6), (6, 7), (7, 8)]))
    assert s["core"].tolist() == [4] * 5 + [1] * 4 and s["degeneracy"][0] == 4 and s["nucleus"][0] == 5 and s["isolated"][0] == 0
    assert s["best_core"].tolist() == [4] * 5 + [1] * 4 and s["in_nucleus"].tolist() == [1] * 5 + [0] * 4
    properties(s)
    # two cliques joined through node 8: no member of community 0, a member of community 1; community 2 is empty and node 9 is
    # in no community
    M = np.zeros((10, 3), bool)
    M[:8, 0] = True
    M[:9, 1] = True
    keys = keys_of(clique(range(4)) + clique(range(4, 8)) + [(i, 8) for i in range(8)] + [(9, 0), (3, 3), (1, 0), (10, 2)])
    s = cs.statement(M, keys)
    assert [core_of(s, a, 0) for a in range(10)] == [3] * 8 + [None, None]
    assert [core_of(s, a, 1) for a in range(10)] == [4] * 9 + [None]                          # through 8 every degree is 4
    assert s["members"].tolist() == [8, 9, 0] and s["degeneracy"].tolist() == [3, 4, 0] and s["nucleus"].tolist() == [8, 9, 0]
    assert s["inlinks2"].tolist() == [24, 40, 0] and s["isolated"].tolist() == [0, 0, 0]
    assert s["best_core"].tolist() == [4] * 9 + [0] and s["best_comm"].tolist() == [1] * 9 + [-1]
    assert s["in_nucleus"].tolist() == [2] * 8 + [1, 0] and (s["skipped"], s["dropped"]) == (1, 2)
    properties(s)
    # without a key every member is isolated, and the nucleus of a community of degeneracy 0 is all of it
    s = cs.statement(M, np.zeros(0, np.uint64))
    assert not s["core"].any() and s["isolated"].tolist() == [8, 9, 0] == s["nucleus"].tolist() and not s["in_nucleus"].any()
    assert s["best_comm"].tolist() == [0] * 8 + [1, -1] and s["L"] == 0


def _hand(co):
    """N = 8, K = 3.  Community 0: the triangle 0 1 2 with 3 hanging on 2 and 6 alone; community 1: the path 3 4 5; community
    2: empty.  Node 7 is in no community."""
    M = np.zeros((8, 3), bool)
    M[[0, 1, 2, 3, 6], 0] = True
    M[[3, 4, 5], 1] = True
    keys = keys_of([(0, 1), (1, 2), (2, 0), (2, 3), (3, 4), (5, 4), (1, 0), (4, 4), (6, 7), (8, 1)])
    return cs.result_of(co, 0.05, cs.statement(M, keys))


def test_derived_values_and_helpers_on_a_hand_made_case(co):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(co)
    assert (r.N, r.M, r.L, r.skipped, r.dropped) == (8, 8, 12, 1, 2)
    assert r.members.tolist() == [5, 3, 0] and r.inlinks2.tolist() == [8, 4, 0] and r.degeneracy.tolist() == [2, 1, 0]
    assert r.nucleus.tolist() == [3, 3, 0] and r.isolated.tolist() == [1, 0, 0]
    assert r.offsets.tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 8] and r.community.tolist() == [0, 0, 0, 0, 1, 1, 1, 0]
    assert r.indeg.tolist() == [2, 2, 3, 1, 1, 2, 1, 0] and r.core.tolist() == [2, 2, 2, 1, 1, 1, 1, 0]
    assert r.best_core.tolist() == [2, 2, 2, 1, 1, 1, 0, 0] and r.best_comm.tolist() == [0, 0, 0, 0, 1, 1, 0, -1]
    assert r.in_nucleus.tolist() == [1, 1, 1, 1, 1, 1, 0, 0]
    assert r.coreness.tolist() == [1.0, 1.0, 1.0, 0.5, 1.0, 1.0, 1.0, 0.0] and r.coreness.dtype == np.float64
    assert r.nucleus_share.tolist() == [3.0 / 5.0, 1.0, -1.0] and r.mean_core.tolist() == [7.0 / 5.0, 1.0, -1.0]
    assert r.shells(0).tolist() == [1, 1, 3] and r.shells(1).tolist() == [0, 3] and r.shells(2).tolist() == [0]
    off, mem, ks = r.cover(1)
    assert off.tolist() == [0, 4, 7] and mem.tolist() == [0, 1, 2, 3, 3, 4, 5] and ks.tolist() == [0, 1] and off.dtype == np.uint64
    off, mem, ks = r.cover(2)
    assert off.tolist() == [0, 3] and mem.tolist() == [0, 1, 2] and ks.tolist() == [0]
    off, mem, ks = r.cover(0)
    assert off.tolist() == [0, 5, 8] and mem.tolist() == [0, 1, 2, 3, 6, 3, 4, 5]
    off, mem, ks = r.nuclei()
    assert off.tolist() == [0, 3, 6] and mem.tolist() == [0, 1, 2, 3, 4, 5] and ks.tolist() == [0, 1]
    assert r.fringe().tolist() == [3, 4, 5, 6, 7] and r.fringe(0).tolist() == [7] and r.fringe(2).size == 8
    assert "Cores" in repr(r)
    # a coreness of -1 where the degeneracy is 0, and nothing at all
    e = co.Cores(0.0, [2, 0], [0, 0], [0, 0], [2, 0], [2, 0], [0, 1, 2], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0], [0, 0])
    assert e.coreness.tolist() == [-1.0, -1.0] and e.nucleus_share.tolist() == [1.0, -1.0] and e.mean_core.tolist() == [0.0, -1.0]
    assert e.nuclei()[0].tolist() == [0] and e.cover(1)[0].tolist() == [0] and e.cover(0)[0].tolist() == [0, 2]
    with pytest.raises(AmmsbError):
        co.Cores(0.0, [1], [0], [1], [1], [0], [0, 1], [0], [0], [1], [1], [0], [1])      # a core above the inner degree
    with pytest.raises(AmmsbError):
        co.Cores(0.0, [1], [0], [0], [1], [1], [0, 1], [1], [0], [0], [0], [0], [0])      # a community id >= K
    with pytest.raises(AmmsbError):
        r.shells(3)


def test_the_cores_file_round_trips_byte_for_byte(co, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(co)
    path, again = str(tmp_path / "cores.txt"), str(tmp_path / "again.txt")
    co.write_cores(path, r)
    assert open(path).read() == ("# 8 3 8 12 0.0500000007 1 2\n"
                                 "c 0 5 8 2 3 1\nc 1 3 4 1 3 0\nc 2 0 0 0 0 0\n"
                                 "n 0 1 0 2 2\nn 1 1 0 2 2\nn 2 1 0 3 2\nn 3 2 0 1 1 1 1 1\nn 4 1 1 2 1\nn 5 1 1 1 1\nn 6 1 0 0 0\n"
                                 "n 7 0\n")
    back = co.read_cores(path)
    for name in cs.PER_COMMUNITY + cs.PER_SLOT + cs.PER_NODE + ("offsets",):
        assert np.array_equal(getattr(back, name), getattr(r, name)) and getattr(back, name).dtype == getattr(r, name).dtype, name
    assert (back.M, back.L, back.skipped, back.dropped, back.threshold) == (8, 12, 1, 2, float(np.float32(0.05)))
    assert back.coreness.tobytes() == r.coreness.tobytes() and back.mean_core.tobytes() == r.mean_core.tobytes()
    co.write_cores(again, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    text = open(path).read()
    for bad in (text.replace("# 8 3 8 12", "# 8 3 9 12"), text.replace("# 8 3 8 12", "# 8 3 8 13"), text.replace("c 1 3", "c 2 3"),
                text.replace("n 7 0\n", ""), text.replace("n 6 1 0 0 0", "n 6 1 0 0"), text.replace("n 6 1 0 0 0", "n 6 1 3 0 0"),
                "", "x\n"):
        open(again, "w").write(bad)
        with pytest.raises(AmmsbError):
            co.read_cores(again)


def test_the_refusals_need_no_device(co):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    with pytest.raises(AmmsbError, match="2\\^32.*threshold|threshold.*2\\^32") as e:
        co.check_slots(1 << 32, 0.0)
    assert "threshold 0" in str(e.value) and str(1 << 32) in str(e.value)
    assert co.check_slots((1 << 32) - 1) == (1 << 32) - 1
    # L against max_bytes: the message names the threshold
    with pytest.raises(AmmsbError, match="threshold 0.25") as e:
        co.check_links(1 << 30 | 1, co.MAX_BYTES, 0.25)
    assert str(4 * ((1 << 30) + 1)) in str(e.value) and str(4 << 30) in str(e.value)
    assert co.check_links(1 << 30) == 1 << 30 and co.check_links(0, 0) == 0
    with pytest.raises(AmmsbError):
        co.check_links(1 << 32, 1 << 40)
    with pytest.raises(AmmsbError):
        co.check_links(1000, 3999)
    assert co.check_links(1000, 4000) == 1000
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AmmsbError):
            co.check_threshold(bad)
    with pytest.raises(AmmsbError):
        co.check_nodes(1 << 31)


def test_bad_shapes_are_refused_without_a_device(co):
    lib = co.load()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    deg = lambda *a: lib.ammsb_cores_degrees(*a, None)       # noqa: E731
    adj = lambda *a: lib.ammsb_cores_adjacency(*a, None)     # noqa: E731
    assert deg(p, 4, 0, p, 4, p, p, 0, 4, p, p) == EINVAL and b"num_cols" in lib.ammsb_cores_last_error()
    assert deg(p, 4, 8193, p, 4, p, p, 0, 4, p, p) == EINVAL
    assert deg(p, 1 << 32, 5, p, 4, p, p, 0, 4, p, p) == EINVAL
    assert deg(p, 4, 5, p, 1 << 32, p, p, 0, 4, p, p) == EINVAL and b"slots" in lib.ammsb_cores_last_error()
    assert deg(p, 4, 5, p, 4, p, p, 3, 2, p, p) == EINVAL and b"range" in lib.ammsb_cores_last_error()
    assert deg(None, 4, 5, p, 4, p, p, 0, 4, p, p) == EINVAL and b"NULL" in lib.ammsb_cores_last_error()
    assert deg(p, 4, 5, p, 4, p + 4, p, 0, 4, p, p) == EINVAL and b"aligned" in lib.ammsb_cores_last_error()
    assert deg(p, 4, 5, p, 4, p, p, 0, 4, p + 2, p) == EINVAL
    assert adj(p, 4, 5, p, 4, p, p, 0, 4, p, p, 1 << 32, p) == EINVAL and b"nbr" in lib.ammsb_cores_last_error()
    assert adj(p, 4, 5, p, 4, p, p, 0, 4, p, p + 4, 8, p) == EINVAL
    assert adj(p, 4, 5, p, 4, p, p, 0, 4, p, p, 8, None) == EINVAL
    assert lib.ammsb_cores_scan(1 << 32, 0, p, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_scan(4, 0, p, p, p + 4, p, p, None) == EINVAL
    assert lib.ammsb_cores_scan(4, 0, None, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_peel(4, 0, 3, 2, p, p, p, 8, p, p, p, p, None) == EINVAL and b"head" in lib.ammsb_cores_last_error()
    assert lib.ammsb_cores_peel(4, 0, 0, 5, p, p, p, 8, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_peel(4, 0, 0, 2, p, p, p, 1 << 32, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_peel(4, 0, 0, 2, p, p, None, 8, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_finish(4, 5, p, 4, p + 1, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_finish(4, 5, p, 1 << 32, p, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_finish(4, 5, p, 4, p, p, p, p, p, None, p, p, p, p, p, None) == EINVAL
    assert lib.ammsb_cores_finish(0, 5, p, 4, p, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
    # the valid no-ops need no device either
    assert deg(None, 4, 5, None, 4, None, None, 2, 0, None, None) == 0
    assert adj(None, 4, 5, None, 4, None, None, 4, 0, None, None, 0, None) == 0
    assert lib.ammsb_cores_scan(0, 0, None, None, p, p, p, None) == 0
    assert lib.ammsb_cores_peel(4, 0, 2, 2, None, None, None, 0, None, None, p, p, None) == 0
    assert lib.ammsb_cores_finish(0, 5, None, 0, None, None, None, p, p, p, p, p, None, None, None, None) == 0


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(co):
    hdr = open(os.path.join(ROOT, "include", "ammsb_cores.h")).read()
    declared = set(re.findall(r"\b(ammsb_cores_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 7 and declared == set(co.SIGNATURES), declared ^ set(co.SIGNATURES)
    assert os.path.exists(co.LIB_PATH) and os.path.basename(co.LIB_PATH) == "libammsb_cores.so"
    assert exported_symbols(co.LIB_PATH) == declared
    for name in ("degrees", "adjacency", "scan", "peel", "finish"):
        decl = re.search(r"int ammsb_cores_%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(co.SIGNATURES["ammsb_cores_" + name][1]), name
    for macro, value in (("MAX_COLS", co.MAX_COLS), ("W1_MAX_COLS", co.W1_MAX_COLS), ("PEEL_LANES", co.PEEL_LANES)):
        assert value == int(re.search(r"#define AMMSB_CORES_%s (\d+)u" % macro, hdr).group(1)), macro
    for macro, value in (("MAX_SLOTS", co.MAX_SLOTS), ("MAX_NBR", co.MAX_NBR)):
        shift = int(re.search(r"#define AMMSB_CORES_%s \(1u?l?l? << (\d+)\)" % macro, hdr).group(1))
        assert value == 1 << shift, macro
    from mcmc_ammsb_gpu_amd import ops
    assert hasattr(ops, "CommunityCores")
    assert all(hasattr(ops.CommunityCores, m) for m in ("degrees", "offsets", "adjacency", "state", "peel", "finish", "run", "kernel_name"))
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_cores.hip")).read()
    assert set(re.findall(r"__global__ [^\n]*void (cores_[a-z0-9_]+)\(", src)) == set(co.KERNEL_FORMS)
    makefile = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "Makefile")).read()
    assert "cores" in re.search(r"^ONE\s*=\s*(.+)$", makefile, re.M).group(1).split()
