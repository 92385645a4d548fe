"""The host side of the community components (include/ammsb_components.h, _components.py): the statement the device tests
compare against, checked here against reachability by boolean powers of the dense induced adjacency; the float64
derivations and the helpers on hand-made integers; the text file; the refusal of a cover of 2^32 memberships; the built
library against its header.  No test here needs a GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import components_statement as cs
from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def cc():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _components
    _components.load()
    return _components


def key(a, b):
    return (int(a) << 32) | int(b)


def random_keys(rng, N, n):
    """n keys over N nodes, both orders of the ends, with loops, repeats and ends >= N among them"""
    a, b = rng.integers(0, N + 2, n), rng.integers(0, N, n)
    loops = rng.random(n) < 0.1
    b[loops] = np.minimum(a[loops], N - 1)
    swap = rng.random(n) < 0.5
    keys = np.array([key(y, x) if s else key(x, y) for x, y, s in zip(a, b, swap)] + [key(2 ** 32 - 1, 0)], dtype=np.uint64)
    return np.concatenate((keys, keys[: n // 5]))


def random_cover(rng, N, K, q):
    M = rng.random((N, K)) < q
    if K > 2:
        M[:, 2] = False     # an empty community
    if N > 5:
        M[5] = False        # a node in no community
    return M


def test_the_statement_equals_reachability_by_boolean_powers():
    rng = np.random.default_rng(7)
    for N, K, n, q in ((1, 1, 3, 1.0), (7, 3, 5, 0.6), (40, 5, 30, 0.5), (200, 8, 150, 0.4), (60, 70, 80, 0.2), (55, 64, 40, 1.0),
                       (30, 65, 200, 0.5)):
        M, keys = random_cover(rng, N, K, q), random_keys(rng, N, n)
        s = cs.statement(M, keys)
        reach = cs.reachability(M, keys)
        off = s["offsets"].astype(np.int64)
        assert np.array_equal(np.diff(off), M.sum(1)) and s["root"].size == int(M.sum())
        for a in range(N):
            ks = s["community"][off[a]:off[a + 1]]
            assert np.array_equal(ks, np.flatnonzero(M[a]))          # the communities of a node ascending
            for j, k in enumerate(ks):
                assert (int(s["root"][off[a] + j]), int(s["size"][off[a] + j])) == reach[k][a], (N, K, a, k)
        for k in range(K):
            comps = {}
            for a, (root, size) in reach[k].items():
                comps[root] = size
            assert int(s["members"][k]) == len(reach[k]) and int(s["components"][k]) == len(comps)
            assert int(s["singletons"][k]) == sum(1 for v in comps.values() if v == 1)
            best = max(comps.items(), key=lambda rv: (rv[1], -rv[0])) if comps else (-1, 0)
            assert (int(s["largest_root"][k]), int(s["largest"][k])) == best
        stray = [sum(1 for k in np.flatnonzero(M[a]) if reach[k][a][0] != s["largest_root"][k]) for a in range(N)]
        assert s["stray"].tolist() == stray
        a, b = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
        ok = (a < N) & (b < N)
        assert s["links"] == int(ok.sum()) and s["skipped"] == int((~ok).sum()) > 0
        assert s["shared"] == int((M[a[ok].astype(np.int64)] & M[b[ok].astype(np.int64)]).sum())
        if K > 2:
            assert s["members"][2] == 0 and s["largest_root"][2] == -1


def test_the_statement_does_not_depend_on_the_order_of_the_keys_or_on_repeats():
    rng = np.random.default_rng(11)
    M, keys = random_cover(rng, 120, 9, 0.4), random_keys(rng, 120, 200)
    s = cs.statement(M, keys)
    flipped = (keys << np.uint64(32)) | (keys >> np.uint64(32))
    for other in (keys[::-1], rng.permutation(keys), np.unique(keys), flipped, np.concatenate((keys, keys))):
        t = cs.statement(M, other)
        for name in cs.PER_COMMUNITY + cs.PER_SLOT + ("stray", "offsets"):
            assert np.array_equal(s[name], t[name]), name
    assert cs.statement(M, np.concatenate((keys, keys)))["shared"] == 2 * s["shared"]


def _hand(cc):
    """N = 9, K = 3.  Community 0: {0, 1} and {2, 3}, two components of two (the tie goes to root 0), and 6 alone; community 1:
    the path 3 7 8; community 2: empty.  Nodes 4 and 5 are in no community."""
    M = np.zeros((9, 3), bool)
    M[[0, 1, 2, 3, 6], 0] = True
    M[[3, 7, 8], 1] = True
    keys = np.array([key(1, 0), key(2, 3), key(3, 7), key(8, 7), key(3, 3), key(0, 4), key(9, 1), key(6, 5), key(2, 3)], dtype=np.uint64)
    return cs.result_of(cc, 0.05, cs.statement(M, keys))


def test_derived_values_and_helpers_on_a_hand_made_case(cc):
    r = _hand(cc)
    assert (r.N, r.M, r.links, r.skipped, r.shared) == (9, 8, 8, 1, 7)
    assert r.members.tolist() == [5, 3, 0] and r.components.tolist() == [3, 1, 0] and r.singletons.tolist() == [1, 0, 0]
    assert r.largest.tolist() == [2, 3, 0] and r.largest_root.tolist() == [0, 3, -1]      # the tie: the smaller root
    assert r.offsets.tolist() == [0, 1, 2, 3, 5, 5, 5, 6, 7, 8] and r.community.tolist() == [0, 0, 0, 0, 1, 0, 1, 1]
    assert r.root.tolist() == [0, 0, 2, 2, 3, 6, 3, 3] and r.size.tolist() == [2, 2, 2, 2, 3, 1, 3, 3]
    assert r.stray.tolist() == [0, 0, 1, 1, 0, 0, 1, 0, 0]
    assert r.giant.tolist() == [2.0 / 5.0, 1.0, -1.0] and r.fragmentation.tolist() == [1.0 - 2.0 / 5.0, 0.0, -1.0]
    assert r.connected == 1.0 / 2.0 and r.giant.dtype == np.float64 and "Components" in repr(r)
    assert r.disconnected().tolist() == [0] and r.disconnected(3).tolist() == [] and r.disconnected(1).tolist() == [0]
    off, mem = r.cover(2)
    assert off.tolist() == [0, 2, 4, 7] and mem.tolist() == [0, 1, 2, 3, 3, 7, 8] and off.dtype == np.uint64
    off, mem = r.cover(1)
    assert off.tolist() == [0, 2, 4, 5, 8] and mem.tolist() == [0, 1, 2, 3, 6, 3, 7, 8]
    off, mem = r.cover()
    assert off.tolist() == [0, 3] and mem.tolist() == [3, 7, 8]
    off, mem = r.trimmed()
    assert off.tolist() == [0, 2, 5, 5] and mem.tolist() == [0, 1, 3, 7, 8]
    # nothing to be connected: every -1
    e = cc.Components(0.0, [0, 0], [0, 0], [0, 0], [-1, -1], [0, 0], [0, 0, 0], [], [], [], [0, 0], 0, 3, 0)
    assert e.connected == -1.0 and e.giant.tolist() == [-1.0, -1.0] and e.fragmentation.tolist() == [-1.0, -1.0]
    assert e.disconnected().size == 0 and e.cover()[0].tolist() == [0] and e.trimmed()[0].tolist() == [0, 0, 0]
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    with pytest.raises(AmmsbError):
        cc.Components(0.0, [1], [2], [1], [0], [0], [0, 1], [0], [0], [1], [0], 0, 0, 0)      # more components than members
    with pytest.raises(AmmsbError):
        cc.Components(0.0, [1], [1], [1], [0], [1], [0, 1], [1], [0], [1], [0], 0, 0, 0)      # a community id >= K
    with pytest.raises(AmmsbError):
        cc.check_giveups(1)


def test_the_components_file_round_trips_byte_for_byte(cc, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(cc)
    path, again = str(tmp_path / "components.txt"), str(tmp_path / "again.txt")
    cc.write_components(path, r)
    assert open(path).read() == ("# 9 3 9 8 0.0500000007 1 7\n"
                                 "c 0 5 3 2 0 1\nc 1 3 1 3 3 0\nc 2 0 0 0 -1 0\n"
                                 "n 0 1 0 0 2\nn 1 1 0 0 2\nn 2 1 0 2 2\nn 3 2 0 2 2 1 3 3\nn 4 0\nn 5 0\nn 6 1 0 6 1\n"
                                 "n 7 1 1 3 3\nn 8 1 1 3 3\n")
    back = cc.read_components(path)
    for name in cs.PER_COMMUNITY + cs.PER_SLOT + ("stray", "offsets"):
        assert np.array_equal(getattr(back, name), getattr(r, name)) and getattr(back, name).dtype == getattr(r, name).dtype, name
    assert (back.links, back.skipped, back.shared, back.threshold) == (8, 1, 7, float(np.float32(0.05)))
    assert back.giant.tobytes() == r.giant.tobytes() and back.connected == r.connected
    cc.write_components(again, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    text = open(path).read()
    for bad in (text.replace("# 9 3 9 8", "# 9 3 9 9"), text.replace("c 1 3", "c 2 3"), text.replace("n 4 0\n", ""),
                text.replace("n 6 1 0 6 1", "n 6 1 0 6"), text.replace("n 6 1 0 6 1", "n 6 1 3 6 1"), "", "x\n"):
        open(again, "w").write(bad)
        with pytest.raises(AmmsbError):
            cc.read_components(again)


def test_a_cover_of_2_32_memberships_is_refused_from_the_counts_alone(cc):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    own = np.full(1 << 19, 8192, np.uint32)           # thr = 0 at N K = 2^32: every stored number is a member
    with pytest.raises(AmmsbError, match="2\\^32.*threshold|threshold.*2\\^32") as e:
        cc.slot_base(own, 0.0)
    assert "threshold 0" in str(e.value) and str(1 << 32) in str(e.value)
    base, M = cc.slot_base(own[:-1], 0.0)
    assert M == (1 << 32) - 8192 and base.dtype == np.uint64 and int(base[-1]) == M and base.size == own.size
    assert cc.check_slots((1 << 32) - 1) == (1 << 32) - 1
    with pytest.raises(AmmsbError):
        cc.check_slots(1 << 32)
    with pytest.raises(AmmsbError):
        cc.check_keys(1 << 31)
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(AmmsbError):
            cc.check_threshold(bad)


def test_bad_shapes_are_refused_without_a_device(cc):
    lib = cc.load()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    assert lib.ammsb_components_own(p, 1, 0, p, None) == EINVAL and b"num_cols" in lib.ammsb_components_last_error()
    assert lib.ammsb_components_own(p, 1 << 32, 5, p, None) == EINVAL
    assert lib.ammsb_components_own(None, 1, 5, p, None) == EINVAL and b"NULL" in lib.ammsb_components_last_error()
    assert lib.ammsb_components_own(p + 4, 1, 5, p, None) == EINVAL and b"aligned" in lib.ammsb_components_last_error()
    assert lib.ammsb_components_slots(p, 4, 5, p, 1 << 32, 0, 4, p, p, p, None) == EINVAL
    assert lib.ammsb_components_slots(p, 4, 5, p, 4, 3, 2, p, p, p, None) == EINVAL
    assert lib.ammsb_components_edges(p, 4, 5, p, 4, p, 1 << 31, p, p, None) == EINVAL
    assert lib.ammsb_components_edges(p, 4, 5, p, 4, p, 1, p, p + 4, None) == EINVAL
    assert lib.ammsb_components_finish(4, 5, p, 4, p, p + 1, p, p, p, p, p, p, p, p, p, p, p, None) == EINVAL
    # the valid no-ops need no device either
    assert lib.ammsb_components_own(None, 0, 5, None, None) == 0
    assert lib.ammsb_components_slots(None, 4, 5, None, 0, 2, 0, None, None, None, None) == 0
    assert lib.ammsb_components_edges(None, 4, 5, None, 0, None, 0, None, p, None) == 0


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(cc):
    hdr = open(os.path.join(ROOT, "include", "ammsb_components.h")).read()
    declared = set(re.findall(r"\b(ammsb_components_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 6 and declared == set(cc.SIGNATURES), declared ^ set(cc.SIGNATURES)
    assert os.path.exists(cc.LIB_PATH) and os.path.basename(cc.LIB_PATH) == "libammsb_components.so"
    assert exported_symbols(cc.LIB_PATH) == declared
    for name in ("own", "slots", "edges", "finish"):
        decl = re.search(r"int ammsb_components_%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(cc.SIGNATURES["ammsb_components_" + name][1]), name
    for macro, value in (("MAX_COLS", cc.MAX_COLS), ("W1_MAX_COLS", cc.W1_MAX_COLS)):
        assert value == int(re.search(r"#define AMMSB_COMPONENTS_%s (\d+)u" % macro, hdr).group(1)), macro
    for macro, value in (("MAX_EDGES", cc.MAX_EDGES), ("MAX_SLOTS", cc.MAX_SLOTS), ("MAX_STEPS", cc.MAX_STEPS)):
        shift = int(re.search(r"#define AMMSB_COMPONENTS_%s \(1u?l?l? << (\d+)\)" % macro, hdr).group(1))
        assert value == 1 << shift, macro
    from mcmc_ammsb_gpu_amd import ops
    assert hasattr(ops, "CommunityComponents")
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_components.hip")).read()
    assert set(re.findall(r"__global__ [^\n]*void (components_[a-z0-9_]+)\(", src)) == set(cc.KERNEL_FORMS)


def test_the_shared_test_header_rebuilds_every_post_fit_test_and_nothing_else(cc):
    """tests/cpp/postfit_test.h is a prerequisite of the C++ tests: in a built tree (the fixture's build()), a change to it
    compiles every <analysis>_test of the Makefile's POSTFIT list again, from its own source, and leaves the library"""
    import make_dry_run as dry
    makefile = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "host", "Makefile")).read()
    postfit = re.search(r"^POSTFIT\s*=\s*(.+)$", makefile, re.M).group(1).split()
    assert len(postfit) >= 13 and "components" in postfit and "readout" in postfit
    fresh = dry.commands("host", "all", remake_all=False)
    after = dry.commands("host", "all", remake_all=False, touched=("../../tests/cpp/postfit_test.h",))
    for name in postfit:
        out, src = "../%s_test" % name, "tests/cpp/%s_test.cc" % name
        assert not dry.builds(fresh, out) and dry.builds(after, out, src), name
        assert '#include "postfit_test.h"' in open(os.path.join(ROOT, src)).read(), name
    assert not dry.builds(after, "../libammsb_host.so") and not dry.builds(after, "../ammsb_main")
