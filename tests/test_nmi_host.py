"""Host half of the overlapping NMI (include/ammsb_nmi.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, the existing libraries untouched), argument errors returned before anything is launched,
the two scores on hand-made entropy arrays with their -1 cases, the cover-NMI file written and parsed back bit for bit,
the check that a ground truth is made of sets, the command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
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
INF = float("inf")


@pytest.fixture(scope="module")
def nm():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _nmi
    _nmi.load()
    return _nmi


def test_header_exports_and_signature_table_agree(nm):
    hdr = open(os.path.join(ROOT, "include", "ammsb_nmi.h")).read()
    declared = set(re.findall(r"\b(ammsb_nmi_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 4 and declared == set(nm.SIGNATURES), declared ^ set(nm.SIGNATURES)
    lib = C.CDLL(nm.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(nm.LIB_PATH)
    assert own == declared, own ^ declared
    assert nm.MAX_COLS == int(re.search(r"#define AMMSB_NMI_MAX_COLS (\d+)u", hdr).group(1)) == 8192
    src = open(os.path.join(PKG, "csrc", "ammsb_nmi.hip")).read()
    assert set(re.findall(r'"(nmi_[a-z0-9_]+)"', src)) == set(nm.KERNEL_FORMS)
    for form in nm.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    # the contract stands at the top of the header, and the shortcut is stated there
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef") and "shortcut" in hdr


def test_the_kernels_are_a_library_of_their_own(nm):
    from mcmc_ammsb_gpu_amd import _capi, _cover
    assert not [n for n in _capi.SIGNATURES if "nmi" in n] and not [n for n in _cover.SIGNATURES if "nmi" in n]
    assert "ammsb_nmi" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    assert "ammsb_nmi" not in open(os.path.join(ROOT, "include", "ammsb_cover.h")).read()
    raw = open(nm.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for other in (_capi.LIB_PATH, _cover.LIB_PATH):
        assert b"ammsb_nmi" not in open(other, "rb").read()
    for form in nm.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    import make_dry_run as dry
    assert dry.header_rebuilds_object("nmi") and dry.csrc_all_builds("../libammsb_nmi.so", "ammsb_nmi.o")
    assert "ammsb_nmi" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert '#include "ammsb_postfit.h"' in open(os.path.join(PKG, "csrc", "ammsb_nmi.hip")).read()


def test_argument_errors_are_returned_before_anything_is_launched(nm):
    lib = nm.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op

    def begin(N=1000, G=5, K=64, ts=p, ds=p, HX=p, HY=p, cX=p, cY=p):
        return lib.ammsb_nmi_begin(N, ts, G, ds, K, HX, HY, cX, cY, None)

    def acc(ov=p, g0=0, Gs=5, N=1000, G=5, K=64, ts=p, ds=p, HX=p, HY=p, cX=p, cY=p):
        return lib.ammsb_nmi_accumulate(ov, g0, Gs, N, ts, G, ds, K, HX, HY, cX, cY, None)

    for call in (begin, acc):
        for name in ("ts", "ds", "HX", "HY", "cX", "cY"):
            assert call(**{name: None}) == EINVAL, (call.__name__, name)
            assert b"NULL" in lib.ammsb_nmi_last_error()
        for K in (0, 8193, 2**32 - 1):
            assert call(K=K) == EINVAL and b"num_cols" in lib.ammsb_nmi_last_error()
        for N in (0, 2**32, 2**40):
            assert call(N=N) == EINVAL and b"num_nodes" in lib.ammsb_nmi_last_error()
        assert call(G=2**31) == EINVAL
        # the detected side is needed also without ground-truth communities; the truth side only with them
        assert call(G=0, ds=None) == EINVAL and call(G=0, HY=None) == EINVAL and call(G=0, cY=None) == EINVAL
    assert acc(ov=None) == EINVAL and b"overlap" in lib.ammsb_nmi_last_error()
    for g0, Gs in ((0, 6), (5, 1), (6, 0), (3, 3), (2**63, 2**63), (1, 2**64 - 1)):
        assert acc(g0=g0, Gs=Gs) == EINVAL, (g0, Gs)
        assert b"slab" in lib.ammsb_nmi_last_error()
    # bad arguments are refused before the empty slab is accepted ...
    assert acc(Gs=0, K=0) == EINVAL and acc(Gs=0, N=0) == EINVAL and acc(Gs=0, ds=None) == EINVAL
    # ... which is a valid call without a device: nothing is launched
    assert acc(Gs=0) == 0 and acc(g0=5, Gs=0) == 0 and acc(Gs=0, ov=None) == 0
    assert acc(G=0, g0=0, Gs=0, ts=None, HX=None, cX=None, ov=None) == 0
    assert lib.ammsb_nmi_last_kernel_name() == b""


def test_scores_on_hand_made_entropies(nm):
    # two ground-truth communities, three detected: H and H(. | other) by hand
    HX, hX = np.array([1.0, 0.5]), np.array([0.25, 0.5])
    HY, hY = np.array([0.5, 0.0, 0.25]), np.array([0.125, 0.0, 0.0])
    lfk, mx = nm.scores(HX, hX, HY, hY)
    # the means are over the communities with H > 0: (0.25 + 1) / 2 and (0.25 + 0) / 2 (k = 1 is left out)
    assert lfk == 1.0 - 0.5 * (0.625 + 0.125) == 0.625
    assert mx == 0.5 * (1.5 - 0.75 + 0.75 - 0.125) / 1.5
    # identical covers: every conditional entropy 0
    assert nm.scores(HX, 0 * HX, HX, 0 * HX) == (1.0, 1.0)
    # independent covers: every conditional entropy is the entropy itself
    assert nm.scores(HX, HX, HY, HY) == (0.0, 0.0)
    # a side with nothing to average makes nmi_lfk -1, as avg_f1 does; nmi_max stands while one side has entropy
    zero = np.zeros(3)
    assert nm.scores(HX, hX, zero, zero) == (-1.0, 0.5 * (1.5 - 0.75) / 1.5)
    assert nm.scores(zero, zero, HY, hY) == (-1.0, 0.5 * (0.75 - 0.125) / 0.75)
    assert nm.scores(zero, zero, zero, zero) == (-1.0, -1.0)
    assert nm.scores(np.zeros(0), np.zeros(0), HY, hY)[0] == -1.0 and nm.scores(HX, hX, np.zeros(0), np.zeros(0))[0] == -1.0
    assert nm.scores(np.zeros(0), np.zeros(0), np.zeros(0), np.zeros(0)) == (-1.0, -1.0)
    # sums are added in index order (numpy's pairwise sum gives another last bit on such arrays)
    rng = np.random.default_rng(3)
    H = rng.random(1000) + 0.5
    h = H * rng.random(1000)
    total_H = total_h = ratio = 0.0
    for a, b in zip(H.tolist(), h.tolist()):
        total_H, total_h, ratio = total_H + a, total_h + b, ratio + b / a
    assert nm.scores(H, h, H, h) == (1.0 - 0.5 * (ratio / 1000 + ratio / 1000),
                                     0.5 * (total_H - total_h + total_H - total_h) / total_H)
    # the fallback: a community no pair qualifies for keeps its own entropy; a minimum above the entropy too
    r = nm.NMI(0.05, [3, 2], [2, 3, 0], 1, HX, [INF, 0.125], HY, [0.75, INF, 0.0])
    assert r.h_truth.tolist() == [1.0, 0.125] and r.h_detected.tolist() == [0.5, 0.0, 0.0]
    assert (r.nmi_lfk, r.nmi_max) == nm.scores(HX, r.h_truth, HY, r.h_detected)
    assert r.truth_size.dtype == np.uint32 and r.detected_size.dtype == np.int64 and r.H_truth.dtype == np.float64
    assert r.skipped == 1 and "nmi_lfk" in repr(r)


def test_the_cover_nmi_file_round_trips_bit_for_bit(nm, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    rng = np.random.default_rng(7)
    G, K = 9, 5
    HX = rng.random(G) * np.array([1, 1e-7, 1, 0, 1, 1e-300, 1, 1, 1])
    HY = rng.random(K)
    cX = np.where(rng.random(G) < 0.3, INF, rng.random(G) / 3)
    cY = np.array([0.0, INF, np.nextafter(HY[2], 0), 5e-324, HY[4] / 3])
    r = nm.NMI(0.05, rng.integers(0, 2**32, G, dtype=np.uint64), rng.integers(0, 2**40, K), 12345678901, HX, cX, HY, cY)
    path = str(tmp_path / "nmi.txt")
    nm.write_cover_nmi(path, 4_000_000_000, r)
    lines = open(path).read().splitlines()
    assert len(lines) == 1 + G + K and lines[0].split()[:4] == ["#", "4000000000", "5", "9"]
    assert lines[1].startswith("t 0 ") and lines[G + 1].startswith("d 0 ") and len(lines[1].split()) == 5
    N, back, printed = nm.read_cover_nmi(path)
    assert N == 4_000_000_000 and back.skipped == r.skipped and back.threshold == float(np.float32(0.05))
    for name in ("H_truth", "H_detected", "h_truth", "h_detected"):
        assert np.array_equal(getattr(back, name).view(np.uint64), getattr(r, name).view(np.uint64)), name
    assert np.array_equal(back.truth_size, r.truth_size) and np.array_equal(back.detected_size, r.detected_size)
    assert printed == (r.nmi_lfk, r.nmi_max) == (back.nmi_lfk, back.nmi_max)
    again = str(tmp_path / "again.txt")
    nm.write_cover_nmi(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # the -1 scores and empty sides
    empty = nm.NMI(0.0, [], [0, 0], 0, [], [], [0.0, 0.0], [INF, INF])
    nm.write_cover_nmi(path, 10, empty)
    assert open(path).readline() == "# 10 2 0 0 0 -1 -1\n"
    N, back, printed = nm.read_cover_nmi(path)
    assert printed == (-1.0, -1.0) and back.H_truth.size == 0 and back.h_detected.tolist() == [0.0, 0.0]
    # malformed files are refused
    good = open(again).read()
    for bad in ("", "# 1 2\n", good.replace("\nt 3 ", "\nt 4 ", 1), good.replace("\nd 0 ", "\nt 0 ", 1),
                good[:good.rindex("\nd ")] + "\n", good + "d 5 1 0.5 0.25\n", good.replace("\nt 1 ", "\nt 1 x ", 1)):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            nm.read_cover_nmi(path)


def test_a_ground_truth_that_is_not_made_of_sets_is_refused(nm):
    from mcmc_ammsb_gpu_amd import _cover
    nm.check_sets(*_cover.check_cover([[1, 2, 3], [3, 2], [], [7]]))        # a node in two communities is a cover
    nm.check_sets(*_cover.check_cover([]))
    nm.check_sets(*_cover.check_cover([[], [5]]))
    for lists in ([[1, 2, 2]], [[4, 1, 9, 4]], [[1, 2], [], [3, 0, 5, 3]], [[2**32 - 1, 0, 2**32 - 1]]):
        with pytest.raises(ValueError, match="twice"):
            nm.check_sets(*_cover.check_cover(lists))
    with pytest.raises(ValueError, match="community 2 lists node 3 twice"):
        nm.check_sets(np.array([0, 2, 2, 6], np.uint64), np.array([1, 2, 3, 0, 5, 3], np.uint32))


def test_no_cpu_path_without_a_gpu(nm, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.CoverNMI([[0, 1], [2]]), lambda: lrn.CoverNMI((np.array([0, 1]), np.array([3])), 0.01),
                 lambda: lrn.CoverNMI([], slab_bytes=1)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    with pytest.raises(AmmsbError):
        lrn.CoverNMI([[0]], threshold=-1.0)
    with pytest.raises(AmmsbError):
        lrn.CoverNMI((np.array([0, 2]), np.array([3])))
    with pytest.raises(ValueError, match="twice"):
        lrn.CoverNMI([[0, 1, 0]])
    assert hasattr(ops, "CoverNMI")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(nm, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    truth, out = str(tmp_path / "truth.cmty"), str(tmp_path / "out.txt")
    open(truth, "w").write("0 1 2\n")
    base = ["-f", missing, "-k", "8"]
    for extra in (["--ground-truth", truth],                                    # no -out flag at all
                  ["--cover-nmi-out", out],                                     # an -out flag without the ground truth
                  ["--cover-match-out", out],
                  ["--cover-nmi-out", out, "--cover-match-out", out],
                  ["--cover-match-threshold", "0.1"],
                  ["--ground-truth", truth, "--cover-nmi-out", out, "--cover-match-threshold", "-1"],
                  ["--ground-truth", truth, "--cover-nmi-out", out, "--cover-match-threshold", "nan"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr and ("need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr), r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (["--ground-truth", truth, "--cover-nmi-out", out],
                  ["--ground-truth", truth, "--cover-match-out", out],
                  ["--ground-truth", truth, "--cover-nmi-out", out, "--cover-match-out", out + "2",
                   "--cover-match-threshold", "0.1"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
