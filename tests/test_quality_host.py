"""Host half of the community-quality read-out (include/ammsb_quality.h), no GPU: the drop-in boundary of the new
library (header == exports == signature table, and the existing library's yardsticks untouched), argument errors
returned before anything is launched, the derived measures on hand-worked cases, the community-quality file written and
parsed back byte for byte, and that no layer has a CPU path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL
EXE = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "ammsb_main")
FORM_RE = r'"(quality_(?:mask|edges)_[a-z0-9_]+)"'


@pytest.fixture(scope="module")
def q():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _quality
    _quality.load()
    return _quality


def test_header_exports_and_signature_table_agree(q):
    hdr = open(os.path.join(ROOT, "include", "ammsb_quality.h")).read()
    declared = set(re.findall(r"\b(ammsb_quality_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(q.SIGNATURES), declared ^ set(q.SIGNATURES)
    lib = C.CDLL(q.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(q.LIB_PATH)
    assert own == declared, own ^ declared
    assert q.MAX_COLS == int(re.search(r"#define AMMSB_QUALITY_MAX_COLS (\d+)u", hdr).group(1)) == 8192
    # the kernel forms: the names in the source are the names the signature module lists and the header describes
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_quality.hip")).read()
    assert set(re.findall(FORM_RE, src)) == set(q.KERNEL_FORMS)
    for form in q.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form


def test_the_kernels_did_not_land_in_the_existing_library(q):
    """libammsb_hip.so and its header are what the kernel census and the symbol test pin: no quality name in either;
    the new library holds gfx950 code under the form names"""
    from mcmc_ammsb_gpu_amd import _capi
    assert not [n for n in _capi.SIGNATURES if "quality" in n]
    assert "quality" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    assert b"quality" not in open(_capi.LIB_PATH, "rb").read()
    raw = open(q.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in q.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    import make_dry_run as dry
    assert dry.csrc_all_builds("../libammsb_quality.so", "ammsb_quality.o") and dry.csrc_all_builds("ammsb_quality.o", "-c ammsb_quality.hip")
    assert "ammsb_quality" not in dry.hip_library_link()   # not part of libammsb_hip.so


def _rpm(rows, cols, rows_in_block=0, blocks=1, ptr=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for i in range(blocks):
        d.blocks[i] = ptr
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows_in_block or rows, rows, cols, blocks
    return d


def test_argument_errors_are_returned_before_anything_is_launched(q):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    lib = q.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments
    good = _rpm(100, 64)

    def mask(d=good, thr=0.05, out=p):
        return lib.ammsb_quality_mask(C.byref(d) if d is not None else None, thr, out, None)

    assert mask(d=None) == EINVAL and mask(out=None) == EINVAL
    for thr in (-1e-30, -1.0, float("nan"), float("inf"), -float("inf")):
        assert mask(thr=thr) == EINVAL
        assert b"thr" in lib.ammsb_quality_last_error()
    assert mask(d=_rpm(100, 0)) == EINVAL and mask(d=_rpm(100, 8193)) == EINVAL
    assert b"num_cols" in lib.ammsb_quality_last_error()
    assert mask(d=_rpm(2**32, 64)) == EINVAL
    assert mask(d=_rpm(100, 64, rows_in_block=10, blocks=9)) == EINVAL      # 90 rows of blocks for 100 rows
    assert b"do not cover" in lib.ammsb_quality_last_error()
    assert mask(d=_rpm(100, 64, ptr=0)) == EINVAL and mask(d=_rpm(100, 64, blocks=0)) == EINVAL

    def edges(m=p, rows=100, cols=64, e=p, n=8, counts=p, shared=p):
        return lib.ammsb_quality_edges(m, rows, cols, e, n, counts, shared, None)

    assert edges(m=None) == EINVAL and edges(e=None) == EINVAL
    assert edges(counts=None, shared=None) == EINVAL
    assert b"no output" in lib.ammsb_quality_last_error()
    assert edges(cols=0) == EINVAL and edges(cols=8193) == EINVAL and edges(rows=2**32) == EINVAL
    # n == 0 is a valid no-op, also without a device: nothing has been launched
    assert edges(n=0) == 0 and edges(n=0, m=None, e=None) == 0 and edges(n=0, counts=None) == 0 and edges(n=0, shared=None) == 0
    assert edges(n=0, counts=None, shared=None) == EINVAL and edges(n=0, cols=0) == EINVAL
    assert lib.ammsb_quality_last_kernel_name() == b""
    # the workspace: 8 ceil(K / 64) bytes per row, a function of the shape alone; 0 for a shape the library refuses
    mb = lib.ammsb_quality_mask_bytes
    assert [mb(10, k) for k in (1, 64, 65, 256, 260, 8192)] == [80, 80, 160, 320, 400, 10240]
    assert mb(0, 64) == 0 and mb(10, 0) == 0 and mb(10, 8193) == 0 and mb(2**32, 64) == 0
    assert mb(2**32 - 1, 8192) == (2**32 - 1) * 1024
    for thr in (-1e-9, float("nan"), float("inf"), 1e39):
        with pytest.raises(AmmsbError):
            q.check_threshold(thr)
    assert q.check_threshold(0.05) == float(np.float32(0.05)) and q.check_threshold(0) == 0.0


def test_derived_measures_on_hand_worked_cases(q):
    # a path 0-1-2-3-4 and the cover {0, 1, 2}, {2, 3}, {4}, {} : 4 links
    #   k   size internal boundary vol  min(vol, 8 - vol)  conductance  density
    #   0    3      2        1      5          3               1/3      2 / 3
    #   1    2      1        2      4          4               1/2      1 / 1
    #   2    1      0        1      1          1                1        -1
    #   3    0      0        0      0          0               -1        -1
    size, internal, boundary = [3, 2, 1, 0], [2, 1, 0, 0], [1, 2, 1, 0]
    assert np.array_equal(q.conductance(internal, boundary, 4), [1 / 3, 0.5, 1.0, -1.0])
    assert np.array_equal(q.density(size, internal), [2 / 3, 1.0, -1.0, -1.0])
    assert q.coverage(1, 4) == 0.75 and q.coverage(0, 4) == 1.0 and q.coverage(0, 0) == -1.0
    # a community that holds every link's both ends: vol = 2 links, the complement's volume is 0 -> -1
    assert np.array_equal(q.conductance([4], [0], 4), [-1.0])
    # more than half of the volume: the complement's volume is the denominator
    assert np.array_equal(q.conductance([3], [1], 4), [1.0])
    r = q.Quality(0.05, size, internal, boundary, 4, 1, 2)
    assert (r.links, r.uncovered, r.skipped, r.coverage) == (4, 1, 2, 0.75)
    assert r.size.dtype == r.internal.dtype == r.boundary.dtype == np.int64
    assert r.conductance.dtype == r.density.dtype == np.float64
    assert np.array_equal(r.conductance, [1 / 3, 0.5, 1.0, -1.0]) and np.array_equal(r.density, [2 / 3, 1.0, -1.0, -1.0])
    # large counts stay exact in the integer part of the formulas: size (size - 1) / 2 at size = 10^6
    assert q.density([10**6], [499999500000])[0] == 1.0
    empty = q.Quality(0.0, [5], [0], [0], 0, 0, 3)
    assert empty.coverage == -1.0 and empty.conductance[0] == -1.0 and empty.density[0] == 0.0


def test_file_round_trip_is_byte_exact(q, tmp_path):
    rng = np.random.default_rng(11)
    K, N, E = 300, 5000, 40000
    size = rng.integers(0, N, K)
    size[:3] = [0, 1, 2]
    internal = rng.integers(0, E // 2, K)
    boundary = rng.integers(0, E // 2, K)
    internal[5], boundary[5] = 0, 0          # vol 0: conductance -1
    internal[6], boundary[6] = E, 0          # every link inside: the complement's volume is 0
    thr = np.float32(0.05)
    f = str(tmp_path / "q.txt")
    q.write_community_quality(f, N, thr, size, internal, boundary, E, 17)
    lines = open(f).read().splitlines()
    assert lines[0] == "# 5000 300 40000 0.0500000007 17" and len(lines) == K + 1
    assert lines[1].split()[:2] == ["0", "0"] and lines[1].split()[5] == "-1" and lines[2].split()[5] == "-1"
    assert lines[6].split()[4] == "-1" and lines[7].split()[4] == "-1"
    N2, K2, E2, thr2, unc2, size2, in2, out2, cond2, dens2 = q.read_community_quality(f)
    assert (N2, K2, E2, unc2) == (N, K, E, 17) and np.float32(thr2) == thr
    assert np.array_equal(size2, size) and np.array_equal(in2, internal) and np.array_equal(out2, boundary)
    assert size2.dtype == np.int64 and cond2.dtype == np.float64
    # the floats of the file are %.9g of the float64 measures; written again from the counts, the bytes are the same
    assert np.allclose(cond2, q.conductance(internal, boundary, E), rtol=1e-8, atol=0)
    assert np.allclose(dens2, q.density(size, internal), rtol=1e-8, atol=0)
    g = str(tmp_path / "again.txt")
    q.write_community_quality(g, N2, thr2, size2, in2, out2, E2, unc2)
    assert open(g, "rb").read() == open(f, "rb").read()
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    for text in ("# 5 2 1 0.05\n0 1 0 0 -1 -1\n1 1 0 0 -1 -1\n",           # a short header
                 "5 2 1 0.05 0\n",                                          # no header
                 "# 5 2 1 0.05 0\n0 1 0 0 -1 -1\n",                         # a line short
                 "# 5 2 1 0.05 0\n0 1 0 0 -1 -1\n1 1 0 0 -1\n",             # a field short
                 "# 5 2 1 0.05 0\n0 1 0 0 -1 -1\n0 1 0 0 -1 -1\n",          # the community ids do not count up
                 "# 5 2 1 0.05 0\n0 1 0 0 -1 -1\n1 x 0 0 -1 -1\n"):
        bad = tmp_path / "bad.txt"
        bad.write_text(text)
        with pytest.raises(AmmsbError):
            q.read_community_quality(str(bad))


def test_no_cpu_path_without_a_gpu(q, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.CommunityQuality(), lambda: lrn.CommunityQuality(0.01, np.zeros(3, np.uint64)),
                 lambda: lrn.SharedCommunities(np.zeros(3, np.uint64), 0.05)):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    with pytest.raises(AmmsbError):
        lrn.CommunityQuality(threshold=-1.0)
    with pytest.raises(AmmsbError):
        lrn.SharedCommunities(np.zeros(3, np.uint64), float("nan"))
    assert hasattr(ops, "CommunityQuality")


def test_command_line_refuses_the_bad_combinations():
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(EXE)
    cases = [(["--community-quality-threshold", "0.1"], "needs --community-quality-out"),
             (["--community-quality-out", "x.txt", "--community-quality-threshold", "-0.5"], "--community-quality-threshold must be"),
             (["--community-quality-out", "x.txt", "--community-quality-threshold", "inf"], ""),
             (["--community-quality-out", "x.txt", "--community-quality-threshold", "1e39"], ""),
             (["--community-quality-out", "x.txt", "--community-quality-threshold", "nan"], ""),
             (["--community-quality-out", "x.txt", "--community-quality-threshold", "0.1x"], "")]
    for args, msg in cases:
        r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stderr[-500:])
        assert any(ln.startswith("F ") and msg in ln for ln in r.stderr.splitlines()), (args, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, args
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    for flag, default in (("community-quality-out", None), ("community-quality-threshold", "0.05")):
        assert re.search(r"--%s arg%s" % (flag, r" \(=%s " % re.escape(default) if default else ""), r.stdout), flag
    # a good combination gets past the flag checks (and stops at the missing file, like any run)
    r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt", "--community-quality-out", "x.txt",
                        "--community-quality-threshold", "0.01"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Failed to detect file" in r.stderr


def test_build_and_link_lines_carry_the_new_library():
    import make_dry_run as dry
    links = dry.host_links()   # (every one of them carries every device library)
    assert len(links) >= 10 and all("-lammsb_linkcomm" in ln and "-lammsb_quality" in ln for ln in links)   # the ASan variants included
    assert dry.host_all_builds("../quality_test", "tests/cpp/quality_test.cc")
    assert dry.host_all_builds("../linkcomm_test", "tests/cpp/linkcomm_test.cc")
    asan = open(os.path.join(ROOT, "tools", "run_asan.sh")).read()
    assert "tests/test_quality_host.py" in asan and "tests/test_linkcomm_host.py" in asan
    ignored = open(os.path.join(ROOT, ".gitignore")).read().split()
    assert "quality_test" in ignored and "linkcomm_test" in ignored
