"""Host half of the node roles (include/ammsb_roles.h), no GPU: the derived measures from hand-made integers against
fractions.Fraction (a star in one community, neighbours split 2 : 2, a node without a link, a community of one), the roles
read off them, the roles file written and parsed back byte for byte, argument errors returned before anything is launched,
the drop-in boundary of the new library (header == exports == signature table, built by build()), the command line's flag
rules, and that no layer has a CPU path."""
import ctypes as C
import math
import os
import re
import subprocess
from fractions import Fraction

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def rl():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _roles
    _roles.load()
    return _roles


def _hand(rl):
    """Two communities.  Nodes 0..4: a star in community 0 (centre 0, leaves 1..4).  Node 5: in community 0, neighbours split
    2 : 2 over communities 0 and 1 (its slot 0 is community 0 by the tie rule).  Node 6: no link.  Node 7: the only member
    of community 1, its neighbours all in community 0: misplaced.  -> Roles with top = 2, among all"""
    # c[a] = (c0, c1)
    c = [(4, 0), (1, 0), (1, 0), (1, 0), (1, 0), (2, 2), (0, 0), (3, 0)]
    own = [(1, 0)] * 6 + [(0, 0), (0, 1)]
    degree = [4, 1, 1, 1, 1, 4, 0, 3]
    embedded = [4, 1, 1, 1, 1, 2, 0, 0]
    home, hcount, hflags = [], [], []
    for (c0, c1), (o0, o1) in zip(c, own):
        cand = sorted((k for k in (0, 1) if (c0, c1)[k] >= 1), key=lambda k: -(c0, c1)[k])
        home.append(cand + [-1] * (2 - len(cand)))
        hcount.append([(c0, c1)[k] for k in cand] + [0] * (2 - len(cand)))
        hflags.append(sum((o0, o1)[k] << j for j, k in enumerate(cand)))
    ksum = [sum(x[0] for x, o in zip(c, own) if o[0]), sum(x[1] for x, o in zip(c, own) if o[1])]
    ksq = [sum(x[0] ** 2 for x, o in zip(c, own) if o[0]), sum(x[1] ** 2 for x, o in zip(c, own) if o[1])]
    kmembers = [6, 1]
    return rl.Roles(0.05, "all", 2, 0, degree, [sum(o) for o in own], embedded, [sum(v > 0 for v in x) for x in c],
                    [sum(x) for x in c], [x[0] ** 2 + x[1] ** 2 for x in c], home, hcount, hflags, ksum, ksq, kmembers,
                    sum(degree), 1, N=8)


def test_derived_measures_agree_with_fractions_on_hand_made_integers(rl):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(rl)
    assert r.embeddedness.dtype == r.participation.dtype == r.z.dtype == np.float64 and r.z.shape == (8, 2)
    assert r.ksum.tolist() == [10, 0] and r.ksq.tolist() == [24, 0]
    # the star: all of the centre's neighbours are in its one community
    assert r.participation[0] == 0.0 and r.embeddedness[0] == 1.0 and r.participation[1] == 0.0
    mean, var = Fraction(10, 6), Fraction(24, 6) - Fraction(10, 6) ** 2
    z0 = (4 - mean) / Fraction(math.sqrt(var))
    assert r.z[0, 0] == (4.0 - 10.0 / 6.0) / math.sqrt(24.0 / 6.0 - (10.0 / 6.0) * (10.0 / 6.0))
    assert abs(Fraction(r.z[0, 0]) - z0) <= 8 * Fraction(2) ** -52 * z0 and r.z[0, 0] > 2.0
    assert Fraction(r.z[1, 0]) < 0 and r.z[0, 1] == 0.0
    # split 2 : 2: 1 - (4 + 4) / 16, exactly; half of its neighbours share its community
    assert r.participation[5] == 0.5 == float(1 - Fraction(8, 16)) and r.embeddedness[5] == 0.5
    assert r.home[5].tolist() == [0, 1] and r.hflags[5] == 1
    # a slot in a community of one member has z 0; a node without a link has -1 and empty slots
    assert r.z[5, 1] == 0.0 and r.z[7].tolist()[1] == 0.0
    assert r.embeddedness[6] == -1.0 and r.participation[6] == -1.0 and r.home[6].tolist() == [-1, -1] and r.z[6].tolist() == [0.0, 0.0]
    assert r.embeddedness[7] == 0.0 and r.participation[7] == 0.0
    # the roles
    assert r.hubs(2.0).tolist() == [0] and r.hubs().tolist() == [] and r.hubs(-10.0).tolist() == [0, 1, 2, 3, 4, 5]
    assert r.connectors(0.5).tolist() == [5] and r.connectors().tolist() == [] and r.connectors(0.0).tolist() == [0, 1, 2, 3, 4, 5, 7]
    assert r.misplaced().tolist() == [7]
    assert "Roles" in repr(r)
    # a range of nodes reports absolute ids
    part = rl.Roles(0.05, "own", 1, 0, [3], [1], [0], [1], [3], [9], [[0]], [[3]], [0], [0, 0], [0, 0], [0, 1], 3, 0, N=8, first=7)
    assert part.misplaced().tolist() == [7] and part.z.tolist() == [[0.0]]
    # the conversion of a uint64 rounds once, to nearest even: 2^53 + 1 is a tie
    big = rl.Roles(0.0, "all", 0, 0, [1], [1], [1], [1], [2 ** 32], [2 ** 53 + 1], np.zeros((1, 0)), np.zeros((1, 0)), [], [0], [0], [1], 1, 0)
    assert big.participation[0] == 1.0 - 2.0 ** 53 / 2.0 ** 64 and big.misplaced().size == 0 and big.hubs().size == 0
    for bad in (lambda: rl.Roles(0.05, "some", 1, 0, [1], [1], [1], [1], [1], [1], [[0]], [[1]], [1], [1], [1], [1], 1, 0),
                lambda: rl.Roles(0.05, "all", 17, 0, [1], [1], [1], [1], [1], [1], [[0] * 17], [[1] * 17], [1], [1], [1], [1], 1, 0),
                lambda: rl.Roles(0.05, "all", 1, 0, [1], [1, 2], [1], [1], [1], [1], [[0]], [[1]], [1], [1], [1], [1], 1, 0),
                lambda: rl.Roles(0.05, "all", 1, 0, [1], [1], [1], [1], [1], [1], [[5]], [[1]], [1], [1], [1], [1], 1, 0),
                lambda: rl.Roles(0.05, "all", 1, 0, [1], [1], [1], [1], [1], [1], [[0]], [[1]], [1], [1], [1, 2], [1], 1, 0),
                lambda: rl.Roles(0.05, "all", 1, 0, [1], [1], [1], [1], [1], [1], [[0]], [[1]], [1], [1], [1], [1], -1, 0)):
        with pytest.raises(AmmsbError):
            bad()


def test_the_roles_file_round_trips_byte_for_byte(rl, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(rl)
    path, again = str(tmp_path / "roles.txt"), str(tmp_path / "again.txt")
    rl.write_roles(path, 8, r)
    lines = open(path).read().splitlines()
    assert lines[0] == "# 8 2 16 0.0500000007 all 2 0 1" and len(lines) == 1 + 2 + 8
    assert lines[1] == "c 0 6 10 24" and lines[2] == "c 1 1 0 0"
    assert lines[3] == "n 0 4 1 4 1 4 16 1 0 4 1" and lines[8] == "n 5 4 1 2 2 4 8 2 0 2 1 1 2 0" and lines[9] == "n 6 0 0 0 0 0 0 0"
    N, back = rl.read_roles(path)
    assert N == 8 and (back.valid, back.skipped, back.among, back.top, back.min_count) == (15, 1, "all", 2, 0)
    assert back.threshold == float(np.float32(0.05)) and np.array_equal(back.home, r.home) and np.array_equal(back.hflags, r.hflags)
    assert back.z.tobytes() == r.z.tobytes() and back.participation.tobytes() == r.participation.tobytes()
    rl.write_roles(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # a range of nodes, sums past 2^32, no selection
    part = rl.Roles(0.0, "own", 0, 7, [3, 0], [1, 0], [0, 0], [1, 0], [2 ** 40, 0], [2 ** 64 - 1, 0], np.zeros((2, 0)), np.zeros((2, 0)),
                    [], [2 ** 63], [2 ** 64 - 1], [5_000_000_000], 3, 0, N=5_000_000_000, first=4_999_999_998)
    rl.write_roles(path, 5_000_000_000, part)
    assert open(path).read() == ("# 5000000000 1 3 0 own 0 7 0\nc 0 5000000000 %d %d\nn 4999999998 3 1 0 1 %d %d 0\n"
                                 "n 4999999999 0 0 0 0 0 0 0\n" % (2 ** 63, 2 ** 64 - 1, 2 ** 40, 2 ** 64 - 1))
    N, back = rl.read_roles(path)
    assert N == 5_000_000_000 and back.first == 4_999_999_998 and back.squares.tolist() == [2 ** 64 - 1, 0]
    rl.write_roles(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    rl.write_roles(path, 8, r)
    good = open(path).read()
    for bad in ("", "# 1 2\n", good.replace("# 8 2", "# eight 2"), good.replace("# 8 2 16", "# 8 3 16"), good.replace(" all 2 ", " some 2 "),
                good.replace("\nc 1 ", "\nc 2 "), good.replace("c 0 6 10 24", "c 0 6 10"), good.replace("c 0 6 10 24", "c 0 6 10 24 1"),
                good.replace("c 0 6 10 24", "c 0 6 10 2x"), good.replace("\nn 3 ", "\nn 4 "), good.replace("n 0 4 1 4 1 4 16 1 0 4 1", "n 0 4 1 4 1 4 16 2 0 4 1"),
                good.replace("n 0 4 1 4 1 4 16 1 0 4 1", "n 0 4 1 4 1 4 16 1 2 4 1"), good.replace("n 0 4 1 4 1 4 16 1 0 4 1", "n 0 4 1 4 1 4 16 1 0 4 2"),
                good.replace("n 5 4 1 2 2 4 8 2 0 2 1 1 2 0", "n 5 4 1 2 2 4 8 3 0 2 1 1 2 0 1 1 0"), good.replace(" 0 1\n", " 0 99\n"),
                good + "c 2 0 0 0\n", good + "n 9 0 0 0 0 0 0 0\n", good.replace("n 6 0 0 0 0 0 0 0", "m 6 0 0 0 0 0 0 0"),
                good.replace("n 6 0 0 0 0 0 0 0", "n 6 %d 0 0 0 0 0 0" % 2 ** 32), good.replace("n 6 0 0 0 0 0 0 0", "n 6 -1 0 0 0 0 0 0")):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            rl.read_roles(path)


def test_argument_errors_are_returned_before_anything_is_launched(rl):
    lib = rl.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_roles_last_error
    names = ("mask", "offsets", "targets", "degree", "own", "embedded", "reached", "votes", "squares", "home", "hcount", "hflags",
             "ksum", "ksq", "kmembers", "counts")

    def nodes(rows=1000, K=64, first=0, n=10, among=0, top=4, min_count=0, **ptrs):
        a = {name: p for name in names}
        a.update(ptrs)
        return lib.ammsb_roles_nodes(a["mask"], rows, K, a["offsets"], a["targets"], first, n, among, top, min_count, a["degree"],
                                     a["own"], a["embedded"], a["reached"], a["votes"], a["squares"], a["home"], a["hcount"],
                                     a["hflags"], a["ksum"], a["ksq"], a["kmembers"], a["counts"], None)

    for name in names:
        assert nodes(**{name: None}) == EINVAL and b"NULL" in err(), name
        if name not in ("home", "hcount", "hflags"):
            assert nodes(**{name: None}, n=0) == EINVAL and nodes(**{name: None}, top=0) == EINVAL, name
    assert nodes(top=0, home=None, hcount=None, hflags=None, n=0) == 0   # the selection is skipped: no slot array is needed
    for K in (0, 8193, 2 ** 32 - 1):
        assert nodes(K=K) == EINVAL and b"num_cols" in err(), K
        assert nodes(K=K, n=0) == EINVAL and b"num_cols" in err(), K
    assert nodes(rows=2 ** 32) == EINVAL and b"2^32" in err()
    for first, n in ((991, 10), (1001, 0), (0, 1001), (2 ** 64 - 1, 2), (5, 2 ** 64 - 1)):
        assert nodes(first=first, n=n) == EINVAL and b"past num_rows" in err(), (first, n)
    for top in (17, 2 ** 32 - 1):
        assert nodes(top=top) == EINVAL and b"top" in err(), top
    for among in (2, 2 ** 32 - 1):
        assert nodes(among=among) == EINVAL and b"among" in err(), among
    for name in names:
        by = 4 if name in ("mask", "offsets", "votes", "squares", "ksum", "ksq", "kmembers", "counts") else 2
        assert nodes(**{name: p + by}) == EINVAL and b"aligned" in err(), name
        assert nodes(**{name: p + by}, n=0) == EINVAL, name
        assert nodes(**{name: p + 1}) == EINVAL and b"aligned" in err(), name
    # n_rows == 0 needs no device, at either end of the range
    assert nodes(n=0) == 0 and nodes(first=1000, n=0) == 0 and nodes(rows=0, n=0) == 0 and nodes(n=0, among=1, top=16, min_count=2 ** 32 - 1) == 0
    assert lib.ammsb_roles_last_kernel_name() == b""
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    assert rl.check_top(1) == 1 and rl.check_top(16) == 16 and rl.check_among("all") == rl.ALL and rl.check_among("own") == rl.OWN
    assert rl.check_min_count(0) == 0 and rl.check_min_count(2 ** 32 - 1) == 2 ** 32 - 1
    assert rl.check_nodes(None, 7) == (0, 7) and rl.check_nodes((2, 5), 7) == (2, 5) and rl.check_nodes((7, 0), 7) == (7, 0)
    assert rl.check_rows(2 ** 25) == 2 ** 25 and rl.check_threshold(0) == 0.0 and rl.check_threshold(0.05) == float(np.float32(0.05))
    for bad in (lambda: rl.check_top(0), lambda: rl.check_top(17), lambda: rl.check_top(1.5), lambda: rl.check_among("ALL"),
                lambda: rl.check_among(0), lambda: rl.check_min_count(-1), lambda: rl.check_min_count(2 ** 32),
                lambda: rl.check_nodes((2, 6), 7), lambda: rl.check_nodes((-1, 2), 7), lambda: rl.check_nodes(3, 7),
                lambda: rl.check_rows(2 ** 25 + 1), lambda: rl.check_threshold(-1e-9), lambda: rl.check_threshold(float("nan")),
                lambda: rl.check_threshold(float("inf")), lambda: rl.check_threshold(1e39)):
        with pytest.raises(AmmsbError):
            bad()


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(rl):
    from mcmc_ammsb_gpu_amd import _capi, _connect, _modularity, _quality
    hdr = open(os.path.join(ROOT, "include", "ammsb_roles.h")).read()
    declared = set(re.findall(r"\b(ammsb_roles_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 3 and declared == set(rl.SIGNATURES), declared ^ set(rl.SIGNATURES)
    assert os.path.exists(rl.LIB_PATH) and os.path.basename(rl.LIB_PATH) == "libammsb_roles.so"
    lib = C.CDLL(rl.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(rl.LIB_PATH)
    assert own == declared, own ^ declared
    # the arguments of the one call, counted in the header's declaration
    decl = re.search(r"int ammsb_roles_nodes\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(rl.SIGNATURES["ammsb_roles_nodes"][1]) == 24
    for macro, value in (("MAX_COLS", rl.MAX_COLS), ("W1_MAX_COLS", rl.W1_MAX_COLS), ("MAX_TOP", rl.MAX_TOP), ("MAX_ROW", rl.MAX_ROW),
                         ("ALL", rl.ALL), ("OWN", rl.OWN)):
        assert value == int(re.search(r"#define AMMSB_ROLES_%s (\d+)u" % macro, hdr).group(1)), macro
    assert (rl.MAX_COLS, rl.MAX_TOP, rl.MAX_ROW, rl.ALL, rl.OWN) == (8192, 16, 33554432, 0, 1)
    src = open(os.path.join(PKG, "csrc", "ammsb_roles.hip")).read()
    assert set(re.findall(r'"(roles_[a-z0-9_]+)"', src)) == set(rl.KERNEL_FORMS) == {"roles_nodes_w1", "roles_nodes_w2"}
    for form in rl.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef") and "AMMSB_EINVAL" in hdr
    assert "asm" not in src   # plain HIP
    # a library of its own: the existing ones do not know it, and its kernels are gfx950 code objects
    for other in (_capi, _quality, _connect, _modularity):
        assert not [n for n in other.SIGNATURES if "roles" in n]
        assert b"ammsb_roles" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_roles.h":
            assert "ammsb_roles" not in open(os.path.join(ROOT, "include", name)).read(), name
    for name in os.listdir(PKG):
        if name.startswith("libammsb_") and name.endswith(".so") and name not in ("libammsb_roles.so", "libammsb_host.so"):
            assert b"ammsb_roles" not in open(os.path.join(PKG, name), "rb").read(), name
    raw = open(rl.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in rl.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    assert '#include "ammsb_postfit.h"' in src
    import make_dry_run as dry
    assert dry.header_rebuilds_object("roles") and dry.csrc_all_builds("../libammsb_roles.so", "ammsb_roles.o")
    assert "ammsb_roles" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert dry.host_all_builds("../roles_test", "tests/cpp/roles_test.cc", "-lammsb_roles")
    for exe in ("roles_test", "ammsb_main"):
        assert os.access(os.path.join(PKG, exe), os.X_OK), exe


def test_no_cpu_path_without_a_gpu(rl, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.NodeRoles(), lambda: lrn.NodeRoles(0.01, edges=[1, 2]), lambda: lrn.NodeRoles(nodes=(3, 10), top=16, among="own")):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.NodeRoles(-1.0), lambda: lrn.NodeRoles(float("nan")), lambda: lrn.NodeRoles(top=0), lambda: lrn.NodeRoles(top=17),
                lambda: lrn.NodeRoles(among="every"), lambda: lrn.NodeRoles(min_count=-1), lambda: lrn.NodeRoles(nodes=(45, 6))):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    assert hasattr(ops, "NodeRoles")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(rl, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    out = str(tmp_path / "out.txt")
    base = ["-f", missing, "-k", "8"]
    o = ["--node-roles-out", out]
    for extra in (["--node-roles-threshold", "0.1"], ["--node-roles-top", "4"], ["--node-roles-among", "own"],   # a modifier without -out
                  o + ["--node-roles-among", "some"], o + ["--node-roles-among", "ALL"],
                  o + ["--node-roles-top", "0"], o + ["--node-roles-top", "17"], o + ["--node-roles-top", "-1"], o + ["--node-roles-top", "four"],
                  o + ["--node-roles-top", "4x"],
                  o + ["--node-roles-threshold", "-0.1"], o + ["--node-roles-threshold", "inf"],
                  o + ["--node-roles-threshold", "1e39"],                  # not finite as a binary32
                  o + ["--node-roles-threshold", "nan"], o + ["--node-roles-threshold", "half"],
                  o + ["--node-roles-threshold", "0.1x"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        assert "need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (o, o + ["--node-roles-threshold", "0", "--node-roles-top", "16", "--node-roles-among", "own"],
                  o + ["--node-roles-top", "1", "--modularity-out", out + "2"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
