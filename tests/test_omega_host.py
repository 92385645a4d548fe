"""Host half of the Omega index (include/ammsb_omega.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, the existing libraries untouched), argument errors returned before anything is launched,
the score on hand-worked integers in exact arithmetic, the cover-Omega file written and parsed back byte for byte, the
command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
import fractions
import math
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def om():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _omega
    _omega.load()
    return _omega


def test_header_exports_and_signature_table_agree(om):
    hdr = open(os.path.join(ROOT, "include", "ammsb_omega.h")).read()
    declared = set(re.findall(r"\b(ammsb_omega_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 5 and declared == set(om.SIGNATURES), declared ^ set(om.SIGNATURES)
    lib = C.CDLL(om.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(om.LIB_PATH)
    assert own == declared, own ^ declared
    for macro, value in (("MAX_COLS", om.MAX_COLS), ("MAX_TRUTH", om.MAX_TRUTH), ("MAX_LEVELS", om.MAX_LEVELS), ("TILE", om.TILE)):
        assert value == int(re.search(r"#define AMMSB_OMEGA_%s (\d+)u" % macro, hdr).group(1)), macro
    assert om.MAX_LAUNCH_TILES == 1 << int(re.search(r"#define AMMSB_OMEGA_MAX_LAUNCH_TILES \(1ull << (\d+)\)", hdr).group(1))
    assert (om.MAX_COLS, om.MAX_TRUTH, om.MAX_LEVELS) == (8192, 65536, 4096)
    src = open(os.path.join(PKG, "csrc", "ammsb_omega.hip")).read()
    assert set(re.findall(r'"(omega_[a-z0-9_]+)"', src)) == set(om.KERNEL_FORMS)
    for form in om.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    # the contract stands at the top of the header, and it says why undefined is NaN here
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef") and "can itself be negative" in hdr


def test_the_kernels_are_a_library_of_their_own(om):
    from mcmc_ammsb_gpu_amd import _capi, _cover, _nmi, _quality
    for other in (_capi, _cover, _nmi, _quality):
        assert not [n for n in other.SIGNATURES if "omega" in n]
        assert b"ammsb_omega" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_omega.h":
            assert "ammsb_omega" not in open(os.path.join(ROOT, "include", name)).read(), name
    raw = open(om.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in om.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    import make_dry_run as dry
    assert dry.header_rebuilds_object("omega") and dry.csrc_all_builds("../libammsb_omega.so", "ammsb_omega.o")
    assert "ammsb_omega" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert '#include "ammsb_postfit.h"' in open(os.path.join(PKG, "csrc", "ammsb_omega.hip")).read()
    assert dry.builds(dry.commands("host", "omega_test"), "../omega_test", "tests/cpp/omega_test.cc", "-lammsb_omega")
    assert dry.host_all_builds("../omega_score_test", "tests/cpp/omega_score_test.cc")


def test_argument_errors_are_returned_before_anything_is_launched(om):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    lib = om.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_omega_last_error

    def desc(K=64, rows=100):
        d = Rpm()
        d.blocks[0] = p
        d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows, rows, K, 1
        return d

    def dbits(pi=True, K=64, thr=0.05, nodes=p, n=10, bits=p, counts=p):
        return lib.ammsb_omega_detected_bits(C.byref(desc(K)) if pi else None, thr, nodes, n, bits, counts, None)

    def tbits(off=p, G=5, mem=p, M=7, N=100, pos=p, n=10, bits=p, counts=p, sk=p, out=p):
        return lib.ammsb_omega_truth_bits(off, G, mem, M, N, pos, n, bits, counts, sk, out, None)

    def pairs(db=p, K=64, tb=p, G=5, n=300, L=4, t0=0, cnt=6, hist=p):
        return lib.ammsb_omega_pairs(db, K, tb, G, n, L, t0, cnt, hist, None)

    for kw in (dict(pi=False), dict(bits=None), dict(counts=None)):
        assert dbits(**kw) == EINVAL and b"NULL" in err(), kw
    for thr in (-1.0, -1e-9, float("nan"), float("inf")):
        assert dbits(thr=thr) == EINVAL and b"thr" in err(), thr
    for K in (0, 8193):
        assert dbits(K=K) == EINVAL and b"num_cols" in err(), K
        assert pairs(K=K) == EINVAL and b"num_cols" in err(), K
    assert dbits(n=2**31) == EINVAL and dbits(nodes=None, n=101) == EINVAL and b"num_rows" in err()
    assert dbits(n=0) == 0 and dbits(n=0, nodes=None) == 0            # a valid no-op without a device
    for name in ("off", "pos", "bits", "counts", "sk", "out", "mem"):
        assert tbits(**{name: None}) == EINVAL and b"NULL" in err(), name
    assert tbits(G=65537) == EINVAL and b"65536" in err() and pairs(G=65537) == EINVAL and b"65536" in err()
    assert tbits(N=2**32) == EINVAL and tbits(M=2**32) == EINVAL and tbits(n=2**31) == EINVAL
    assert tbits(n=0) == 0 and tbits(G=0, M=0, off=None, mem=None) == 0
    for L in (0, 4097, 2**32 - 1):
        assert pairs(L=L) == EINVAL and b"num_levels" in err() and b"LDS" in err(), L
    assert pairs(hist=None) == EINVAL and pairs(db=None) == EINVAL and pairs(tb=None) == EINVAL and b"NULL" in err()
    # n = 300 is 3 tile rows: 6 tiles
    for t0, cnt in ((0, 7), (6, 1), (7, 0), (3, 4), (2**63, 2**63), (1, 2**64 - 1)):
        assert pairs(t0=t0, cnt=cnt) == EINVAL and b"triangle" in err(), (t0, cnt)
    assert pairs(n=2**31 - 1, cnt=2**26 + 1) == EINVAL and b"32-bit" in err()
    # bad arguments are refused before the empty range is accepted, which is a valid call without a device
    assert pairs(cnt=0, L=0) == EINVAL and pairs(n=0, cnt=0, K=0) == EINVAL
    assert pairs(cnt=0) == 0 and pairs(t0=6, cnt=0) == 0 and pairs(n=0, cnt=0, db=None, tb=None) == 0
    assert pairs(n=1, cnt=0) == 0 and pairs(G=0, tb=None, cnt=0) == 0
    assert lib.ammsb_omega_last_kernel_name() == b""


def test_scores_on_hand_worked_integers(om):
    # n = 4, D = {{0, 1}, {2, 3}}, T = {{0, 1, 2, 3}}: 4 pairs share nothing and 2 share one in D; all 6 share one in T
    assert om.scores([0, 2], [4, 2], [0, 6], 4) == (0.0, 2 / 6, 6)
    # identical histograms with every pair agreeing
    assert om.scores([7, 2, 1], [7, 2, 1], [7, 2, 1], 5)[:2] == (1.0, 1.0)
    # all pairs at level 0 in both covers: P^2 == Se
    o, u, P = om.scores([10], [10], [10], 5)
    assert math.isnan(o) and u == 1.0 and P == 10
    o, u, P = om.scores([0], [0], [0], 1)
    assert math.isnan(o) and math.isnan(u) and P == 0
    assert math.isnan(om.scores([0], [0], [0], 0)[0])
    # worse than chance is negative, which is why undefined is NaN and not -1
    assert om.scores([0, 0], [3, 3], [3, 3], 4)[0] < 0
    # P near 5e11: the value of the exact fraction, rounded once
    n = 1_000_001
    P = n * (n - 1) // 2
    detected = [P - 123_456_789_012 - 3_333_333, 123_456_789_012, 3_333_333]
    truth = [P - 98_765_432_101 - 7_777_777 - 11, 98_765_432_101, 7_777_777, 11]
    agree = [P - 150_000_000_003, 60_000_000_001, 1_234_567, 0]
    detected.append(0)
    Sa, Se = sum(agree), sum(d * t for d, t in zip(detected, truth))
    want = fractions.Fraction(Sa * P - Se, P * P - Se)
    o, u, pairs = om.scores(np.array(agree), np.array(detected), np.array(truth), n)
    assert pairs == P and o == float(want) and u == float(fractions.Fraction(Sa, P))
    r = om.Omega(0.05, 4, [0, 2], [4, 2], [0, 6], 3, 1, K=2, G=1)
    assert r.omega == 0.0 and r.pairs == 6 and r.nodes == 4 and r.agree.dtype == np.int64 and "omega" in repr(r)


def test_the_cpp_score_rounds_the_exact_quotient_once(om):
    """mcmc::Learner::OmegaIndex::Derive (tests/cpp/omega_score_test.cc, no device) against fractions.Fraction rounded
    once: negative values, ties to even, quotients at and past 2^64, tiny quotients, and random histograms (entries below
    2^62, so that every intermediate fits the 128 bits the header names)"""
    import random
    exe = os.path.join(PKG, "omega_score_test")
    rnd = random.Random(5)
    U = 2**64 - 1
    cases = [(4, [0, 2], [4, 2], [0, 6]), (5, [10], [10], [10]), (1, [0], [0], [0]), (4, [0, 0], [3, 3], [3, 3]),
             # n = 2: P = 1, so omega_unadjusted = Sa and omega = (Sa - Se) / (1 - Se)
             (2, [U, U, U], [0, 0, 0], [0, 0, 0]),                      # q = 3 (2^64 - 1) >= 2^64
             (2, [2**53 + 1], [0], [0]), (2, [2**53 + 3], [0], [0]),    # ties: to even, down and up
             (2, [2**54 + 2], [0], [0]), (2, [2**54 + 6], [0], [0]),
             (2, [U, U], [2**32, 3], [2**31, 7]), (2, [0, 0], [2**60, 5], [2**60, 9]),    # negative numerator or denominator
             (3, [1], [0], [0]), (2**32 - 1, [1], [U], [3]), (2**31, [2**61 + 12345, 0], [2**62, 1], [1, 2**62])]
    for _ in range(200):
        L = rnd.randrange(1, 5)
        big = lambda: rnd.randrange(0, 2**rnd.randrange(1, 62))   # noqa: E731
        cases.append((rnd.randrange(2, 2**32), [big() for _ in range(L)], [big() for _ in range(L)], [big() for _ in range(L)]))
    text = "".join("%d %s %s %s\n" % (n, *(",".join(map(str, h)) for h in (a, d, t))) for n, a, d, t in cases)
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr[-500:]
    lines = out.stdout.split("\n")[:len(cases)]
    for (n, a, d, t), line in zip(cases, lines):
        P = n * (n - 1) // 2
        Sa, Se = sum(a), sum(x * y for x, y in zip(d, t))
        want_u = "nan" if n < 2 else "%.17g" % float(fractions.Fraction(Sa, P))
        want_o = "nan" if n < 2 or P * P == Se else "%.17g" % float(fractions.Fraction(Sa * P - Se, P * P - Se))
        assert line.split() == [want_o, want_u], (n, a, d, t, line)
        if n >= 2 and max(a + d + t) < 2**63:
            o, u, _ = om.scores(np.array(a), np.array(d), np.array(t), n)
            assert line.split() == [om._g17(o), om._g17(u)]


def test_the_cover_omega_file_round_trips_byte_for_byte(om, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    n = 1_000_001
    P = n * (n - 1) // 2
    r = om.Omega(0.05, n, [P - 10**11, 5 * 10**10, 17], [P - 10**11 - 3, 10**11, 3], [P - 6 * 10**10, 6 * 10**10, 0],
                 12345678901, 42, K=1024, G=5000)
    path, again = str(tmp_path / "omega.txt"), str(tmp_path / "again.txt")
    om.write_cover_omega(path, 4_000_000_000, r)
    lines = open(path).read().splitlines()
    assert len(lines) == 4 and lines[0].split()[:4] == ["#", "4000000000", "1024", "5000"] and len(lines[0].split()) == 10
    N, back, printed = om.read_cover_omega(path)
    assert N == 4_000_000_000 and (back.nodes, back.skipped, back.outside, back.K, back.G) == (n, 12345678901, 42, 1024, 5000)
    assert back.threshold == float(np.float32(0.05)) and printed == (r.omega, r.omega_unadjusted) == (back.omega, back.omega_unadjusted)
    for name in ("agree", "detected", "truth"):
        assert np.array_equal(getattr(back, name), getattr(r, name)), name
    om.write_cover_omega(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # NaN is printed as nan and comes back as NaN
    om.write_cover_omega(path, 10, om.Omega(0.0, 1, [0], [0], [0], 0, 0, K=2, G=0))
    assert open(path).readline() == "# 10 2 0 0 1 0 0 nan nan\n"
    N, back, printed = om.read_cover_omega(path)
    assert math.isnan(printed[0]) and math.isnan(back.omega) and back.agree.tolist() == [0]
    om.write_cover_omega(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    good = "# 10 2 1 0.5 4 0 0 0 0.33333333333333331\n0 0 4 0\n1 2 2 6\n"
    for bad in ("", "# 1 2\n", good.replace("\n1 2", "\n2 2"), good.replace("0 0 4 0", "0 0 x 0"), good.replace("1 2 2 6", "1 2 2"),
                good.replace("1 2 2 6", "1 2 -2 6"), good.splitlines()[0] + "\n", good.replace("# 10", "# ten")):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            om.read_cover_omega(path)


def test_universes_and_sets_are_checked_on_the_host(om):
    from mcmc_ammsb_gpu_amd import _cover
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    off, mem = _cover.check_cover([[7, 2, 100], [2, 9], [], [2**32 - 1]])
    assert om.check_universe("all", 10, mem).tolist() == list(range(10))
    assert om.check_universe("covered", 10, mem).tolist() == [2, 7, 9]
    assert om.check_universe([1, 3, 9], 10, mem).dtype == np.uint32 and om.check_universe([], 10, mem).size == 0
    for bad in ([3, 1], [1, 1], [1, 10], [-1, 2], "some", [[1, 2]], [0.5]):
        with pytest.raises(AmmsbError):
            om.check_universe(bad, 10, mem)
    om.check_sets(off, mem)
    with pytest.raises(ValueError, match="community 1 lists node 4 twice"):
        om.check_sets(*_cover.check_cover([[1, 2], [4, 0, 4]]))
    assert om.tiles(0) == 0 and om.tiles(1) == 1 and om.tiles(128) == 1 and om.tiles(129) == 3 and om.tiles(300) == 6


def test_no_cpu_path_without_a_gpu(om, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.CoverOmega([[0, 1], [2]]), lambda: lrn.CoverOmega((np.array([0, 1]), np.array([3])), 0.01, "all"),
                 lambda: lrn.CoverOmega([], universe=[1, 5, 7], launch_pairs=1)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.CoverOmega([[0]], threshold=-1.0), lambda: lrn.CoverOmega([[0]], universe=[5, 4]),
                lambda: lrn.CoverOmega([[0]], universe=[1, 50]), lambda: lrn.CoverOmega([[0]], universe="some"),
                lambda: lrn.CoverOmega((np.array([0, 2]), np.array([3]))), lambda: lrn.CoverOmega([[0]], launch_pairs=0)):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    with pytest.raises(AmmsbError, match='universe="covered"'):
        lrn.CoverOmega([[0, 1]], universe="all", max_bytes=100)
    with pytest.raises(ValueError, match="twice"):
        lrn.CoverOmega([[0, 1, 0]])
    assert hasattr(ops, "CoverOmega")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(om, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    truth, out = str(tmp_path / "truth.cmty"), str(tmp_path / "out.txt")
    open(truth, "w").write("0 1 2\n")
    base = ["-f", missing, "-k", "8"]
    for extra in (["--ground-truth", truth],                                    # none of the three -out flags
                  ["--cover-omega-out", out],                                   # an -out flag without the ground truth
                  ["--cover-omega-out", out, "--cover-nmi-out", out, "--cover-match-out", out],
                  ["--ground-truth", truth, "--cover-nmi-out", out, "--cover-omega-universe", "all"],
                  ["--cover-omega-universe", "covered"],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-omega-universe", "some"],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-omega-universe", "ALL"],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-match-threshold", "-1"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr and ("need" in r.stderr or "must be" in r.stderr), r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (["--ground-truth", truth, "--cover-omega-out", out],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-omega-universe", "all"],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-omega-universe", "covered",
                   "--cover-match-threshold", "0.1"],
                  ["--ground-truth", truth, "--cover-omega-out", out, "--cover-nmi-out", out + "2", "--cover-match-out", out + "3"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
