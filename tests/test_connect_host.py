"""Host half of the community links (include/ammsb_connect.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, the existing libraries untouched), argument errors returned before anything is launched, the
derived densities and the bridged pairs on hand-worked cases, the linked-communities file written and parsed back byte
for byte, the command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
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
def cn():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _connect
    _connect.load()
    return _connect


def test_header_exports_and_signature_table_agree(cn):
    hdr = open(os.path.join(ROOT, "include", "ammsb_connect.h")).read()
    declared = set(re.findall(r"\b(ammsb_connect_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 7 and declared == set(cn.SIGNATURES), declared ^ set(cn.SIGNATURES)
    lib = C.CDLL(cn.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(cn.LIB_PATH)
    assert own == declared, own ^ declared
    for macro, value in (("MAX_COLS", cn.MAX_COLS), ("MAX_TOP", cn.MAX_TOP), ("RUNS_MAX_COLS", cn.RUNS_MAX_COLS),
                         ("LINKS", cn.LINKS), ("DENSITY", cn.DENSITY)):
        assert value == int(re.search(r"#define AMMSB_CONNECT_%s (\d+)u" % macro, hdr).group(1)), macro
    assert (cn.MAX_COLS, cn.MAX_TOP, cn.RUNS_MAX_COLS) == (8192, 64, 4096)
    assert cn.MEASURES == {"links": cn.LINKS, "density": cn.DENSITY}
    src = open(os.path.join(PKG, "csrc", "ammsb_connect.hip")).read()
    assert set(re.findall(r'"(connect_[a-z0-9_]+)"', src)) == set(cn.KERNEL_FORMS)
    for form in cn.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef")


def test_the_kernels_are_a_library_of_their_own(cn):
    from mcmc_ammsb_gpu_amd import _capi, _quality, _relate
    for other in (_capi, _quality, _relate):
        assert not [n for n in other.SIGNATURES if "connect" in n]
        assert b"ammsb_connect" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_connect.h":
            assert "ammsb_connect" not in open(os.path.join(ROOT, "include", name)).read(), name
    raw = open(cn.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    hip = open(_capi.LIB_PATH, "rb").read()
    for form in cn.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
        assert form.encode() not in hip, form
    import make_dry_run as dry
    assert dry.header_rebuilds_object("connect") and dry.csrc_all_builds("../libammsb_connect.so", "ammsb_connect.o")
    assert "ammsb_connect" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert '#include "ammsb_postfit.h"' in open(os.path.join(PKG, "csrc", "ammsb_connect.hip")).read()
    assert dry.builds(dry.commands("host", "../connect_test"), "../connect_test", "tests/cpp/connect_test.cc", "-lammsb_connect")
    assert dry.host_all_builds("../connect_test", "tests/cpp/connect_test.cc", "-lammsb_connect")
    # every line of a full host build that links device libraries carries this one too
    lines = dry.host_links()
    assert lines and all("-lammsb_connect " in ln + " " for ln in lines), [ln for ln in lines if "-lammsb_connect " not in ln + " "]


def test_argument_errors_are_returned_before_anything_is_launched(cn, monkeypatch):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    monkeypatch.delenv("AMMSB_CONNECT_FORM", raising=False)
    lib = cn.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_connect_last_error

    def desc(K=64, rows=1000, rib=None, blocks=1):
        d = Rpm()
        for b in range(blocks):
            d.blocks[b] = p
        d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows if rib is None else rib, rows, K, blocks
        return d

    def mask(pi=True, thr=0.05, out=p, **kw):
        return lib.ammsb_connect_mask(C.byref(desc(**kw)) if pi else None, thr, out, None)

    def edges(m=p, rows=1000, K=64, e=p, n=10, d=p, c=p):
        return lib.ammsb_connect_edges(m, rows, K, e, n, d, c, None)

    def finish(d=p, K=64, links=0x4000):
        return lib.ammsb_connect_finish(d, K, links, None)

    def top(links=p, ov=p, K=64, measure=1, T=4, min_links=1, partner=p, plinks=p, pshared=p):
        return lib.ammsb_connect_top(links, ov, K, measure, T, min_links, partner, plinks, pshared, None)

    for kw in (dict(pi=False), dict(out=None)):
        assert mask(**kw) == EINVAL and b"NULL" in err(), kw
    for thr in (-1.0, -1e-9, float("nan"), float("inf")):
        assert mask(thr=thr) == EINVAL and b"thr" in err(), thr
    for K in (0, 8193):
        assert mask(K=K) == EINVAL and b"num_cols" in err(), K
        assert edges(K=K) == EINVAL and b"num_cols" in err(), K
        assert edges(K=K, n=0) == EINVAL and b"num_cols" in err(), K
        assert finish(K=K) == EINVAL and b"num_cols" in err(), K
        assert top(K=K) == EINVAL and b"num_cols" in err(), K
    d = desc()
    d.num_rows = d.rows_in_block = 2**32
    assert lib.ammsb_connect_mask(C.byref(d), 0.05, p, None) == EINVAL and b"2^32" in err()
    assert mask(rib=400, blocks=2) == EINVAL and b"cover" in err()     # 800 < 1000 rows
    assert mask(rib=0) == EINVAL and b"cover" in err()
    d = desc(blocks=2, rib=500)
    d.blocks[1] = None
    assert lib.ammsb_connect_mask(C.byref(d), 0.05, p, None) == EINVAL and b"NULL" in err()
    assert mask(out=p + 4) == EINVAL and b"aligned" in err()
    assert mask(rows=0, rib=10) == 0 and mask(rows=0, rib=10, thr=-1.0) == EINVAL    # the empty pi is a no-op, after the checks
    for name in ("m", "e", "d", "c"):
        assert edges(**{name: None}) == EINVAL and b"NULL" in err(), name
    assert edges(rows=2**32) == EINVAL and b"2^32" in err()
    # n == 0 needs neither a mask nor a list nor a device
    assert edges(n=0) == 0 and edges(m=None, e=None, n=0) == 0
    assert edges(d=None, n=0) == EINVAL and edges(c=None, n=0) == EINVAL
    for bad in ("x", "", "direct", "dr", "R"):
        monkeypatch.setenv("AMMSB_CONNECT_FORM", bad)
        assert edges() == EINVAL and b"AMMSB_CONNECT_FORM" in err(), bad
        assert edges(n=0) == EINVAL, bad
    for good in ("d", "r"):
        monkeypatch.setenv("AMMSB_CONNECT_FORM", good)
        assert edges(n=0) == 0
    monkeypatch.delenv("AMMSB_CONNECT_FORM")
    assert finish(d=None) == EINVAL and b"NULL" in err() and finish(links=None) == EINVAL and b"NULL" in err()
    assert finish(links=p) == EINVAL and b"same buffer" in err()
    for name in ("links", "ov", "partner", "plinks", "pshared"):
        assert top(**{name: None}) == EINVAL and b"NULL" in err(), name
    for measure in (2, 7, 2**32 - 1):
        assert top(measure=measure) == EINVAL and b"measure" in err(), measure
    for T in (0, 65, 2**32 - 1):
        assert top(T=T) == EINVAL and b"top" in err(), T
    assert lib.ammsb_connect_last_kernel_name() == b""


def test_mask_bytes_on_hand_shapes(cn):
    f = cn.load().ammsb_connect_mask_bytes
    assert f(1, 1) == 8 and f(1, 64) == 8 and f(1, 65) == 16 and f(3, 65) == 48 and f(128, 8192) == 128 * 128 * 8
    assert f(2**32 - 1, 8192) == (2**32 - 1) * 128 * 8
    assert f(0, 5) == 0 and f(10, 0) == 0 and f(10, 8193) == 0 and f(2**32, 4) == 0


def _hand_case(cn):
    # four communities of sizes 8, 8, 2, 4; 0 and 1 share 3 nodes; internal links 12, 10, 1, 0 (community 3 has none)
    # links between: (0,1) 30, (0,2) 4, (0,3) 1, (1,2) 4, (1,3) 2, (2,3) 0
    size, internal = [8, 8, 2, 4], [12, 10, 1, 0]
    partner = [[1, 2, 3], [0, 2, 3], [0, 1, -1], [1, 0, -1]]
    links = [[30, 4, 1], [30, 4, 2], [4, 4, 0], [2, 1, 0]]
    shared = [[3, 0, 0], [3, 0, 0], [0, 0, 0], [0, 0, 0]]
    return cn.Linked(0.05, "density", 1, size, internal, partner, links, shared, 60, 2, N=20)


def test_derived_numbers_agree_with_fractions_and_bridged_on_a_hand_worked_case(cn):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand_case(cn)
    assert r.top == 3 and r.size.dtype == np.int64 and r.internal.dtype == np.int64 and r.partner.dtype == np.int32
    assert r.links.dtype == np.uint64 and r.shared.dtype == np.uint32 and r.matrix is None
    assert r.density.dtype == r.within.dtype == np.float64 and (r.valid, r.skipped) == (60, 2)
    for k in range(4):
        d = int(r.size[k])
        assert r.within[k] == float(Fraction(2 * int(r.internal[k]), d * (d - 1)))
        for t in range(3):
            l = int(r.partner[k, t])
            if l < 0:
                assert r.density[k, t] == 0.0
            else:
                pairs = d * int(r.size[l]) - int(r.shared[k, t])
                assert r.density[k, t] == float(Fraction(int(r.links[k, t]), pairs)), (k, t)
    assert r.density[0, 0] == 30 / 61 and r.within.tolist() == [24 / 56, 20 / 56, 1.0, 0.0]
    # (0, 1): 30/61 = 0.49 >= min(0.43, 0.36); (0, 2): 4/16 = 0.25 < 0.43; (1, 2): 0.25 < 0.36; community 3 has no
    # link inside (within == 0), so it bridges nothing
    assert r.bridged() == [(0, 1)] and r.bridged(1.4) == [] and r.bridged(0.5) == [(0, 1), (0, 2), (1, 2)]
    assert r.bridged(0.0) == [(0, 1), (0, 2), (1, 2)]
    one = cn.Linked(0.05, "links", 1, [1, 3], [5, 0], [[1], [0]], [[7], [7]], [[1], [1]], 12, 0)
    assert one.within.tolist() == [-1.0, 0.0] and one.density.tolist() == [[3.5], [3.5]]
    none = cn.Linked(0.05, "links", 1, [1, 1], [1, 1], [[1], [0]], [[2], [2]], [[1], [1]], 1, 0)    # no pair of distinct nodes
    assert none.density.tolist() == [[0.0], [0.0]] and none.bridged() == []
    assert "Linked" in repr(r)
    for bad in (lambda: cn.Linked(0.05, "jaccard", 1, [1], [0], [[-1]], [[0]], [[0]], 0, 0),
                lambda: cn.Linked(0.05, "links", 1, [1, 2], [0, 0], [[-1]], [[0]], [[0]], 0, 0),
                lambda: cn.Linked(0.05, "links", 1, [1], [0, 0], [[-1]], [[0]], [[0]], 0, 0),
                lambda: cn.Linked(0.05, "links", 1, [1], [0], [[-1, -1]], [[0]], [[0, 0]], 0, 0)):
        with pytest.raises(AmmsbError):
            bad()
    assert cn.check_args("density", 64, 0) == (cn.DENSITY, 64, 0) and cn.check_args("links", 1, 2**64 - 1)[2] == 2**64 - 1
    for by, T, ml in (("jaccard", 4, 1), ("links", 0, 1), ("links", 65, 1), ("density", 4, -1), ("density", 4, 2**64)):
        with pytest.raises(AmmsbError):
            cn.check_args(by, T, ml)


def test_the_linked_communities_file_round_trips_byte_for_byte(cn, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand_case(cn)
    path, again = str(tmp_path / "linked.txt"), str(tmp_path / "again.txt")
    cn.write_linked(path, 20, r)
    assert open(path).read() == ("# 20 4 62 0.0500000007 density 3 1 2\n0 8 12 3 1 30 3 2 4 0 3 1 0\n1 8 10 3 0 30 3 2 4 0 3 2 0\n"
                                 "2 2 1 2 0 4 0 1 4 0\n3 4 0 2 1 2 0 0 1 0\n")
    N, back = cn.read_linked(path)
    assert N == 20 and back.by == "density" and back.top == 3 and back.min_links == 1 and (back.valid, back.skipped) == (60, 2)
    assert back.threshold == float(np.float32(0.05))
    for name in ("size", "internal", "partner", "links", "shared", "density", "within"):
        assert np.array_equal(getattr(back, name), getattr(r, name)), name
    cn.write_linked(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # counts past 2^32 keep their digits
    big = cn.Linked(0.0, "links", 3, [4_000_000_000, 3_000_000_000], [2**40, 7], [[1], [0]], [[2**41 + 1], [2**41 + 1]],
                    [[2_999_999_999], [2_999_999_999]], 2**42, 0)
    cn.write_linked(path, 5_000_000_000, big)
    assert open(path).read() == ("# 5000000000 2 4398046511104 0 links 1 3 0\n0 4000000000 1099511627776 1 1 2199023255553 2999999999\n"
                                 "1 3000000000 7 1 0 2199023255553 2999999999\n")
    N, back = cn.read_linked(path)
    assert N == 5_000_000_000 and back.links.tolist() == [[2**41 + 1]] * 2 and back.internal.tolist() == [2**40, 7]
    good = "# 12 2 9 0.05 links 2 1 0\n0 8 3 1 1 2 0\n1 2 0 1 0 2 0\n"
    open(path, "w").write(good)
    assert cn.read_linked(path)[1].density.tolist() == [[2 / 16, 0.0], [2 / 16, 0.0]]
    for bad in ("", "# 1 2\n", good.replace("links 2", "jaccard 2"), good.replace("\n1 2 0", "\n2 2 0"), good.replace("0 8 3 1 1 2 0", "0 8 3 1 1 2"),
                good.replace("0 8 3 1 1 2 0", "0 8 3 3 1 2 0 1 2 0 1 2 0"), good.replace("0 8 3 1 1 2 0", "0 8 3 1 x 2 0"),
                good.replace("1 2 0 1 0 2 0", "1 2 0 1 2 2 0"), good.replace("1 2 0 1 0 2 0", "1 2 0 1 -1 2 0"),
                good.splitlines()[0] + "\n0 8 3 0\n", good + "2 1 0 0\n", good.replace("# 12", "# twelve"),
                good.replace("links 2 1 0", "links 65 1 0"), good.replace("links 2 1 0", "links 2 1 10"), good.replace("# 12 2 9", "# 12 2")):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            cn.read_linked(path)


def test_no_cpu_path_without_a_gpu(cn, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.CommunityLinks(), lambda: lrn.CommunityLinks(0.01, edges=[1, 2]),
                 lambda: lrn.LinkedCommunities(), lambda: lrn.LinkedCommunities(0.1, 64, "links", 0, None, 1, True),
                 lambda: lrn.LinkedCommunities(by="links", top=1)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.CommunityLinks(-1.0), lambda: lrn.CommunityLinks(float("nan")), lambda: lrn.LinkedCommunities(max_bytes=0),
                lambda: lrn.LinkedCommunities(threshold=float("inf")), lambda: lrn.LinkedCommunities(top=0),
                lambda: lrn.LinkedCommunities(top=65), lambda: lrn.LinkedCommunities(by="jaccard"),
                lambda: lrn.LinkedCommunities(min_links=-1)):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    assert hasattr(ops, "CommunityLinks")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(cn, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    out = str(tmp_path / "out.txt")
    base = ["-f", missing, "-k", "8"]
    o = ["--linked-communities-out", out]
    for extra in (["--linked-communities-threshold", "0.1"],                    # a modifier without -out
                  ["--linked-communities-top", "4"],
                  ["--linked-communities-by", "density"],
                  ["--linked-communities-min-links", "2"],
                  o + ["--linked-communities-by", "jaccard"], o + ["--linked-communities-by", "Density"],
                  o + ["--linked-communities-top", "0"], o + ["--linked-communities-top", "65"],
                  o + ["--linked-communities-top", "-3"], o + ["--linked-communities-top", "four"],
                  o + ["--linked-communities-top", "4.5"],
                  o + ["--linked-communities-min-links", "-1"], o + ["--linked-communities-min-links", "two"],
                  o + ["--linked-communities-threshold", "-0.1"], o + ["--linked-communities-threshold", "inf"],
                  o + ["--linked-communities-threshold", "1e39"],                  # not finite as a binary32
                  o + ["--linked-communities-threshold", "nan"], o + ["--linked-communities-threshold", "half"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        assert "need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (o, o + ["--linked-communities-by", "links"], o + ["--linked-communities-by", "density", "--linked-communities-top", "64"],
                  o + ["--linked-communities-threshold", "0", "--linked-communities-top", "1", "--linked-communities-min-links", "0"],
                  o + ["--related-communities-out", out + "2"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
