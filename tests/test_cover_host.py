"""Host half of the cover match (include/ammsb_cover.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, and the existing library's yardsticks untouched), argument errors returned before anything
is launched, the workspace on hand-worked shapes, the derived measures on a hand-worked example, the SNAP cmty reader,
the cover-match file written and parsed back byte for byte, that no layer has a CPU path, and the planted cover of the
synthetic generator."""
import ctypes as C
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL
FORM_RE = r'"(cover_[a-z0-9_]+)"'


@pytest.fixture(scope="module")
def cv():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _cover
    _cover.load()
    return _cover


def test_header_exports_and_signature_table_agree(cv):
    hdr = open(os.path.join(ROOT, "include", "ammsb_cover.h")).read()
    declared = set(re.findall(r"\b(ammsb_cover_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(cv.SIGNATURES), declared ^ set(cv.SIGNATURES)
    lib = C.CDLL(cv.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(cv.LIB_PATH)
    assert own == declared, own ^ declared
    assert cv.MAX_COLS == int(re.search(r"#define AMMSB_COVER_MAX_COLS (\d+)u", hdr).group(1)) == 8192
    assert cv.UNIT == int(re.search(r"#define AMMSB_COVER_UNIT (\d+)u", hdr).group(1))
    # the kernel forms: the names in the source are the names the signature module lists and the header describes
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_cover.hip")).read()
    assert set(re.findall(FORM_RE, src)) == set(cv.KERNEL_FORMS)
    for form in cv.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form


def test_the_kernels_did_not_land_in_the_existing_library(cv):
    from mcmc_ammsb_gpu_amd import _capi
    assert not [n for n in _capi.SIGNATURES if "cover" in n]
    assert "ammsb_cover" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    assert b"ammsb_cover" not in open(_capi.LIB_PATH, "rb").read()
    raw = open(cv.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in cv.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
        assert form.encode() not in open(_capi.LIB_PATH, "rb").read(), form
    import make_dry_run as dry
    assert dry.csrc_all_builds("../libammsb_cover.so", "ammsb_cover.o") and dry.csrc_all_builds("ammsb_cover.o", "-c ammsb_cover.hip")
    assert "ammsb_cover" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert "*.so" in open(os.path.join(ROOT, ".gitignore")).read().split()


def _rpm(rows, cols, rows_in_block=0, blocks=1, ptr=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for i in range(blocks):
        d.blocks[i] = ptr
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows_in_block or rows, rows, cols, blocks
    return d


def test_argument_errors_are_returned_before_anything_is_launched(cv):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    lib = cv.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    good = _rpm(100, 64)
    names = ("offsets", "members", "dsize", "tb", "to", "ts", "db", "do", "sk", "ov", "ws")

    def match(d=good, thr=0.05, G=5, M=40, wsb=1 << 20, **kw):
        a = {n: p for n in names}
        a.update(kw)
        return lib.ammsb_cover_match(C.byref(d) if d is not None else None, thr, a["offsets"], G, a["members"], M,
                                     a["dsize"], a["tb"], a["to"], a["ts"], a["db"], a["do"], a["sk"], a["ov"],
                                     a["ws"], wsb, None)

    assert match(d=None) == EINVAL
    for n in names:
        if n != "ov":                       # (the dense overlap is optional)
            assert match(**{n: None}) == EINVAL, n
            assert lib.ammsb_cover_last_error() != b""
    for thr in (-1e-30, -1.0, float("nan"), float("inf"), -float("inf")):
        assert match(thr=thr) == EINVAL
        assert b"thr" in lib.ammsb_cover_last_error()
    assert match(d=_rpm(100, 0)) == EINVAL and match(d=_rpm(100, 8193)) == EINVAL
    assert b"num_cols" in lib.ammsb_cover_last_error()
    assert match(d=_rpm(2**32, 64)) == EINVAL
    assert match(d=_rpm(100, 64, rows_in_block=10, blocks=9)) == EINVAL      # 90 rows of blocks for 100 rows
    assert b"do not cover" in lib.ammsb_cover_last_error()
    assert match(d=_rpm(100, 64, ptr=0)) == EINVAL and match(d=_rpm(100, 64, blocks=0)) == EINVAL
    assert match(G=2**31) == EINVAL and match(M=2**32) == EINVAL
    need = lib.ammsb_cover_workspace_bytes(40, 64)
    assert match(wsb=need - 1) == EINVAL and b"workspace" in lib.ammsb_cover_last_error()
    assert match(ws=p + 4) == EINVAL and b"aligned" in lib.ammsb_cover_last_error()
    # G == 0 or M == 0 is a valid no-op, also without a device: nothing is launched, nothing is written
    assert match(G=0) == 0 and match(M=0) == 0 and match(G=0, M=0) == 0
    assert match(G=0, offsets=None, tb=None, to=None, ts=None) == 0
    assert match(M=0, members=None, ws=None, wsb=0) == 0
    assert match(G=0, thr=-1.0) == EINVAL and match(M=0, d=_rpm(100, 0)) == EINVAL and match(G=0, dsize=None) == EINVAL
    assert lib.ammsb_cover_last_kernel_name() == b""
    # the workspace, with U = ceil(M / 128) and W = ceil(K / 64): 8 K + 8 ceil(U / 2) + 256 U W
    wb = lib.ammsb_cover_workspace_bytes
    assert cv.UNIT == 128
    assert wb(1, 1) == 8 + 8 + 256                       # U = 1, W = 1
    assert wb(128, 64) == 512 + 8 + 256                  # still one unit, one word
    assert wb(129, 65) == 520 + 8 + 256 * 2 * 2          # U = 2, W = 2
    assert wb(385, 8192) == 65536 + 16 + 256 * 4 * 128   # U = 4 (three whole units and one entry), W = 128
    assert wb(2_000_000, 1024) == 8192 + 8 * 7813 + 256 * 15625 * 16
    assert wb(0, 64) == 0 and wb(10, 0) == 0 and wb(10, 8193) == 0 and wb(2**32, 64) == 0
    for thr in (-1e-9, float("nan"), float("inf"), 1e39):
        with pytest.raises(AmmsbError):
            cv.check_threshold(thr)
    assert cv.check_threshold(0.05) == float(np.float32(0.05)) and cv.check_threshold(0) == 0.0


def test_derived_measures_on_a_hand_worked_example(cv):
    # five nodes; truth {0, 1, 2}, {2, 3}, {4}, {} against detected {0, 1}, {2, 3, 4}, {}:
    #   overlap      k0  k1  k2        F1(g, k) = 2 o / (t + d)
    #   g0 (t = 3)    2   1   0        4/5  2/6  -     -> best 0, overlap 2
    #   g1 (t = 2)    0   2   0        -    4/5  -     -> best 1, overlap 2
    #   g2 (t = 1)    0   1   0        -    2/4  -     -> best 1, overlap 1
    #   g3 (t = 0)                                     -> unmatched, and not part of the mean
    #   k0 (d = 2): g0 2/5                             -> best 0;  k1 (d = 3): g0 1/6, g1 2/5, g2 1/4 -> best 1
    #   k2 (d = 0): unmatched, and not part of the mean
    m = cv.Match(0.05, [0, 1, 1, -1], [2, 2, 1, 0], [3, 2, 1, 0], [0, 1, -1], [2, 2, 0], [2, 3, 0], 0)
    assert np.array_equal(m.f1_truth_each, [0.8, 0.8, 0.5, 0.0])
    assert np.array_equal(m.f1_detected_each, [0.8, 0.8, 0.0])
    assert np.array_equal(m.jaccard_truth_each, [2 / 3, 2 / 3, 1 / 3, 0.0])
    assert m.f1_truth == (0.8 + 0.8 + 0.5) / 3 and m.f1_detected == (0.8 + 0.8) / 2
    assert m.avg_f1 == (m.f1_truth + m.f1_detected) / 2
    assert m.truth_best.dtype == m.detected_best.dtype == np.int32 and m.truth_overlap.dtype == np.uint32
    assert m.truth_size.dtype == m.detected_overlap.dtype == np.uint32 and m.detected_size.dtype == np.int64
    assert m.f1_truth_each.dtype == np.float64 and m.overlap is None
    # an unmatched, non-empty community scores 0 in its mean
    m = cv.Match(0.05, [0, -1], [1, 0], [1, 4], [0], [1], [1], 3)
    assert m.f1_truth == 0.5 and m.f1_detected == 1.0 and m.avg_f1 == 0.75 and m.skipped == 3
    # means over nothing are -1, and so is the average
    m = cv.unmatched(0.05, 3, np.zeros(4, np.int64))
    assert (m.f1_truth, m.f1_detected, m.avg_f1) == (-1.0, -1.0, -1.0)
    assert (m.truth_best == -1).all() and (m.detected_best == -1).all() and m.truth_best.size == 3
    m = cv.unmatched(0.05, 0, np.array([5, 0], np.int64))
    assert (m.f1_truth, m.f1_detected, m.avg_f1) == (-1.0, 0.0, -1.0)
    assert cv.f1(10**9, 10**9, 10**9) == 1.0 and cv.jaccard(10**9, 10**9, 10**9) == 1.0


def test_read_cover_and_write_cover(cv, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    f = tmp_path / "c.cmty"
    f.write_text("# a SNAP cmty file\n7 3 3 5\n\n  \n10\t20 10\n#1 2 3\n4\n")
    off, mem, dropped = cv.read_cover(str(f))
    assert off.dtype == np.uint64 and mem.dtype == np.uint32 and dropped == 0
    assert off.tolist() == [0, 3, 5, 6] and mem.tolist() == [3, 5, 7, 10, 20, 4]
    off, mem, dropped = cv.read_cover(str(f), {3: 0, 5: 1, 7: 2, 10: 9, 4: 8})     # 20 is not in the graph
    assert off.tolist() == [0, 3, 4, 5] and mem.tolist() == [0, 1, 2, 9, 8] and dropped == 1
    g = tmp_path / "again.cmty"
    cv.write_cover(str(g), off, mem)
    assert g.read_text() == "0 1 2\n9\n8\n"
    off2, mem2, _ = cv.read_cover(str(g))
    assert np.array_equal(off2, off) and np.array_equal(mem2, mem)
    for text in ("1 2 x\n", "1 -2\n", "1 2.5\n", "1 4294967296\n"):
        f.write_text(text)
        with pytest.raises(AmmsbError):
            cv.read_cover(str(f))
    # the argument forms of a cover: (offsets, members) or a list of id lists, taken as written
    off, mem = cv.check_cover([[5, 5, 1], [], [2]])
    assert off.tolist() == [0, 3, 3, 4] and mem.tolist() == [5, 5, 1, 2]
    off, mem = cv.check_cover((np.array([0, 2]), np.array([1, 0])))
    assert off.dtype == np.uint64 and mem.dtype == np.uint32
    off, mem = cv.check_cover([])
    assert off.tolist() == [0] and mem.size == 0
    for bad in ((np.array([0, 3]), np.array([1, 0])), (np.array([1, 2]), np.array([1, 0])),
                (np.array([0, 2, 1, 2]), np.array([1, 0])), (np.array([0, 1]), np.array([-1])), [[2**32]],
                (np.array([0.0, 1.0]), np.array([1]))):
        with pytest.raises(AmmsbError):
            cv.check_cover(bad)


def test_file_round_trip_is_byte_exact(cv, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    rng = np.random.default_rng(12)
    G, K, N = 40, 7, 5000
    ts, ds = rng.integers(1, N, G), rng.integers(1, N, K)
    ts[3], ds[2] = 0, 0
    tb, db = rng.integers(0, K, G), rng.integers(0, G, K)
    to = np.minimum(ts, rng.integers(1, 50, G))
    do = np.minimum(ds, rng.integers(1, 50, K))
    tb[[3, 5]], to[[3, 5]], db[2], do[2] = -1, 0, -1, 0
    m = cv.Match(0.05, tb, to, ts, db, do, ds, 9)
    f = str(tmp_path / "m.txt")
    cv.write_cover_match(f, N, m)
    lines = open(f).read().splitlines()
    assert len(lines) == 1 + G + K
    assert lines[0] == "# 5000 7 40 0.0500000007 9 %.9g %.9g %.9g" % (m.f1_truth, m.f1_detected, m.avg_f1)
    assert lines[4] == "t 3 0 -1 0 0" and lines[1 + G + 2] == "d 2 0 -1 0 0"
    assert lines[1] == "t 0 %d %d %d %.9g" % (ts[0], tb[0], to[0], 2.0 * to[0] / (ts[0] + ds[tb[0]]))
    N2, m2, (ft, fd, fa, fte, fde) = cv.read_cover_match(f)
    assert N2 == N and m2.skipped == 9 and np.float32(m2.threshold) == np.float32(0.05)
    for a in ("truth_best", "truth_overlap", "truth_size", "detected_best", "detected_overlap", "detected_size"):
        assert np.array_equal(getattr(m2, a), getattr(m, a)) and getattr(m2, a).dtype == getattr(m, a).dtype, a
    assert np.array_equal(m2.f1_truth_each, m.f1_truth_each) and m2.avg_f1 == m.avg_f1    # the same formula, the same ints
    assert np.allclose(fte, m.f1_truth_each, rtol=1e-8, atol=0) and np.allclose(fde, m.f1_detected_each, rtol=1e-8, atol=0)
    assert np.allclose([ft, fd, fa], [m.f1_truth, m.f1_detected, m.avg_f1], rtol=1e-8, atol=0)
    g = str(tmp_path / "again.txt")
    cv.write_cover_match(g, N2, m2)
    assert open(g, "rb").read() == open(f, "rb").read()
    ok = "# 5 1 1 0.05 0 1 1 1\nt 0 2 0 2 1\nd 0 2 0 2 1\n"
    bad = tmp_path / "bad.txt"
    bad.write_text(ok)
    cv.read_cover_match(str(bad))
    for text in ("# 5 1 1 0.05 0 1 1\nt 0 2 0 2 1\nd 0 2 0 2 1\n",         # a short header
                 "5 1 1 0.05 0 1 1 1\n",                                  # no header
                 "# 5 1 1 0.05 0 1 1 1\nt 0 2 0 2 1\n",                   # a line short
                 "# 5 1 1 0.05 0 1 1 1\nt 0 2 0 2\nd 0 2 0 2 1\n",        # a field short
                 "# 5 1 1 0.05 0 1 1 1\nd 0 2 0 2 1\nt 0 2 0 2 1\n",      # the sections swapped
                 "# 5 1 1 0.05 0 1 1 1\nt 1 2 0 2 1\nd 0 2 0 2 1\n",      # the ids do not count up
                 "# 5 1 1 0.05 0 1 1 1\nt 0 2 0 2 1\nd 0 2 0 2 1\nd 1 2 0 2 1\n",   # a line too many
                 "# 5 1 1 0.05 0 1 1 1\nt 0 x 0 2 1\nd 0 2 0 2 1\n"):
        bad.write_text(text)
        with pytest.raises(AmmsbError):
            cv.read_cover_match(str(bad))


def test_no_cpu_path_without_a_gpu(cv, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.CompareCover([[0, 1], [2]]), lambda: lrn.CompareCover((np.array([0, 1]), np.array([3])), 0.01),
                 lambda: lrn.CompareCover([], dense=True)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    with pytest.raises(AmmsbError):
        lrn.CompareCover([[0]], threshold=-1.0)
    with pytest.raises(AmmsbError):
        lrn.CompareCover((np.array([0, 2]), np.array([3])))
    assert hasattr(ops, "CoverMatch")


# sha256 of generate_graph(N, K_true, avg_degree, seed).tobytes() (uint64 keys, little-endian), taken from a build of the
# commit before the membership loop was factored out of the generator (da9f273), with hostlib.generate_graph
PARENT_GRAPHS = {
    (2000, 8, 8.0, 5): (8096, "e1c6e9404ea0eb912d88e7d406060dfc38dc5f134e444bfcd5d60fd6779911c7"),
    (10000, 32, 32.0, 20260101): (160502, "9962bb0df4efbbe390370fc1cf33253db767a9662a1cfbb9b2204771e2e74441"),
    (6000, 8, 12.0, 3): (36587, "38f4eefb1cb38ce84b823fe95d6254c153549bdc3555e86a3e6e93711ee33226"),
    (3001, 300, 10.0, 77): (12790, "2a913531c9ba35919f463b84c273084bfbf34039e8c9ed445de575ddc82c1ef3"),
}


@pytest.mark.parametrize("shape", sorted(PARENT_GRAPHS))
def test_the_generator_keeps_its_cover_and_its_graph(cv, shape):
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, k_true, deg, seed = shape
    edges = hostlib.generate_graph(N, k_true, deg, seed=seed)
    assert (edges.size, hashlib.sha256(edges.tobytes()).hexdigest()) == PARENT_GRAPHS[shape]
    off, mem = hostlib.generate_cover(N, k_true, seed=seed)
    assert off.dtype == np.uint64 and mem.dtype == np.uint32 and off.size == k_true + 1
    assert off[0] == 0 and off[-1] == mem.size and (np.diff(off.astype(np.int64)) >= 0).all()
    M = np.zeros((N, k_true), dtype=bool)
    for k in range(k_true):
        m = mem[int(off[k]):int(off[k + 1])]
        assert (np.diff(m.astype(np.int64)) > 0).all() and (m < N).all()      # ascending: distinct inside a community
        M[m, k] = True
    per_node = M.sum(1)
    assert per_node.min() >= 1 and per_node.max() <= 3 and set(np.unique(per_node)) == {1, 2, 3}
    a, b = (edges >> np.uint64(32)).astype(np.int64), (edges & np.uint64(0xFFFFFFFF)).astype(np.int64)
    assert (M[a] & M[b]).any(1).all(), "an edge whose ends share no planted community"
    again = hostlib.generate_cover(N, k_true, seed=seed)
    assert np.array_equal(again[0], off) and np.array_equal(again[1], mem)
    assert not np.array_equal(hostlib.generate_cover(N, k_true, seed=seed + 1)[1], mem)
    cv.check_cover((off, mem))
    for bad in ((1, 8), (100, 2), (100, 0)):
        with pytest.raises(AmmsbError):
            hostlib.generate_cover(*bad)


EXE = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "ammsb_main")


def test_command_line_refuses_the_bad_combinations():
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(EXE)
    pair = ["--ground-truth", "t.txt", "--cover-match-out", "x.txt"]
    cases = [(["--ground-truth", "t.txt"], "need each other"),
             (["--cover-match-out", "x.txt"], "need each other"),
             (["--cover-match-threshold", "0.1"], "--cover-match-threshold needs"),
             (["--ground-truth", "t.txt", "--cover-match-threshold", "0.1"], "need each other"),
             (pair + ["--cover-match-threshold", "-0.5"], "--cover-match-threshold must be"),
             (pair + ["--cover-match-threshold", "inf"], ""),
             (pair + ["--cover-match-threshold", "1e39"], ""),
             (pair + ["--cover-match-threshold", "nan"], ""),
             (pair + ["--cover-match-threshold", "0.1x"], ""),
             (pair + ["--cover-match-threshold", ""], "")]
    for args, msg in cases:
        r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stderr[-500:])
        assert any(ln.startswith("F ") and msg in ln for ln in r.stderr.splitlines()), (args, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, args       # refused before the graph file is touched
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    for flag, default in (("ground-truth", None), ("cover-match-out", None), ("cover-match-threshold", "0.05")):
        assert re.search(r"--%s arg%s" % (flag, r" \(=%s " % re.escape(default) if default else ""), r.stdout), flag
    # a good combination gets past the flag checks (and stops at the missing file, like any run)
    r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + pair + ["--cover-match-threshold", "0.01"],
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Failed to detect file" in r.stderr


def test_host_build_and_link_lines_carry_the_new_library(cv):
    import make_dry_run as dry
    links = dry.host_links()   # (every one of them carries every device library)
    assert len(links) >= 11 and all("-lammsb_quality" in ln and "-lammsb_cover" in ln for ln in links)
    asan = [ln for ln in links if "libammsb_host_asan.so" in ln or "-lrccl" in ln]
    assert len(asan) >= 4                                           # the host library twice, ammsb_main_asan, exchange_test_asan
    # the host library is linked again once libammsb_cover.so is newer, its objects compiled again once the header is
    relinked = dry.commands("host", "../libammsb_host.so", remake_all=False, touched=("../libammsb_cover.so",))
    assert dry.builds(relinked, "../libammsb_host.so") and not dry.builds(relinked, "learner.o")
    recompiled = dry.commands("host", "../libammsb_host.so", remake_all=False, touched=("../../include/ammsb_cover.h",))
    assert dry.builds(recompiled, "postfit.o", "-c postfit.cc") and dry.builds(recompiled, "learner.o", "-c learner.cc")
    assert dry.host_all_builds("../cover_test", "tests/cpp/cover_test.cc")
    assert dry.host_all_builds("../quality_test", "tests/cpp/quality_test.cc")
    assert os.path.exists(os.path.join(ROOT, "tests", "cpp", "cover_test.cc"))
    run_asan = open(os.path.join(ROOT, "tools", "run_asan.sh")).read()
    assert "tests/test_cover_host.py" in run_asan and "tests/test_quality_host.py" in run_asan
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "cover_test" in ignored and "quality_test" in ignored


def test_the_text_loader_keeps_the_original_ids_and_the_cpp_reader_maps_them(cv, tmp_path):
    """GetUniqueEdgesFromFile's overload: the same edges and the same rand() draws as the existing one, and the file's
    id of every dense id; mcmc::ReadCover equals _cover.read_cover, with and without the id map"""
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    rng = np.random.default_rng(5)
    orig = rng.choice(10**6, 300, replace=False) * 7 + 11          # ids that are not dense
    pairs = rng.integers(0, 300, (2000, 2))
    pairs = pairs[pairs[:, 0] != pairs[:, 1]]
    g = tmp_path / "g.txt"
    g.write_text("# a\n# b\n# c\n# d\n" + "".join("%d\t%d\n" % (orig[a], orig[b]) for a, b in pairs))
    libc = C.CDLL(None)
    libc.srand(77)
    N1, e1 = hostlib.load_snap(str(g))
    after1 = libc.rand()
    libc.srand(77)
    N2, e2, ids = hostlib.load_snap_ids(str(g))
    after2 = libc.rand()
    assert N1 == N2 == ids.size and np.array_equal(e1, e2) and after1 == after2
    assert ids.dtype == np.uint32 and sorted(ids.tolist()) == sorted(set(orig[pairs].reshape(-1).tolist()))
    a, b = ids[(e2 >> np.uint64(32)).astype(np.int64)], ids[(e2 & np.uint64(0xFFFFFFFF)).astype(np.int64)]
    want = {(min(x, y), max(x, y)) for x, y in orig[pairs].tolist()}
    assert {(min(x, y), max(x, y)) for x, y in zip(a.tolist(), b.tolist())} == want
    # the cover: comments, blank lines, duplicates, ids the graph never mentions
    t = tmp_path / "t.txt"
    known = ids.tolist()
    t.write_text("# truth\n%d %d\t%d %d\n\n   \n%d 5 %d 99999999999\n3\n" % (known[4], known[1], known[4], known[9], known[0], known[2]))
    off, mem, dropped = hostlib.read_cover(str(t), ids)
    o2, m2, d2 = cv.read_cover(str(t), {int(v): i for i, v in enumerate(known)})
    assert np.array_equal(off, o2) and np.array_equal(mem, m2) and dropped == d2 == 3
    assert off.tolist() == [0, 3, 5, 5] and mem.tolist() == [1, 4, 9, 0, 2]
    d = tmp_path / "d.txt"
    d.write_text("7 3 3 1\n# x\n2\n")
    off, mem, dropped = hostlib.read_cover(str(d))
    o2, m2, d2 = cv.read_cover(str(d))
    assert off.tolist() == o2.tolist() == [0, 3, 4] and mem.tolist() == m2.tolist() == [1, 3, 7, 2] and dropped == d2 == 0
    for bad in ("1 2 x\n", "1 -2\n", "4294967296\n", "1 2.5\n"):
        d.write_text(bad)
        with pytest.raises(AmmsbError):
            hostlib.read_cover(str(d))
        with pytest.raises(AmmsbError):
            cv.read_cover(str(d))
    with pytest.raises(AmmsbError):
        hostlib.read_cover(str(tmp_path / "missing.txt"))
