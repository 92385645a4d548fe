"""Host half of the link-community read-out (include/ammsb_linkcomm.h), no GPU: the drop-in boundary of the new
library (header == exports == signature table, and the existing library's yardsticks untouched), argument errors
returned before anything is launched, the link-communities file written and parsed back bit for bit, and that no layer
has a CPU path."""
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
FORM_RE = r'"(linkcomm_(?:fast|generic)[a-z0-9_]*)"'


@pytest.fixture(scope="module")
def lc():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _linkcomm
    _linkcomm.load()
    return _linkcomm


def test_header_exports_and_signature_table_agree(lc):
    hdr = open(os.path.join(ROOT, "include", "ammsb_linkcomm.h")).read()
    declared = set(re.findall(r"\b(ammsb_linkcomm_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(lc.SIGNATURES), declared ^ set(lc.SIGNATURES)
    lib = C.CDLL(lc.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(lc.LIB_PATH)
    assert own == declared, own ^ declared
    assert (lc.MAX_TOP, lc.MAX_COLS) == tuple(int(re.search(r"#define %s (\d+)u" % n, hdr).group(1))
                                              for n in ("AMMSB_LINKCOMM_MAX_TOP", "AMMSB_LINKCOMM_MAX_COLS"))
    assert (lc.MAX_TOP, lc.MAX_COLS) == (16, 8192)
    assert lc.NONE == int(re.search(r"#define AMMSB_LINKCOMM_NONE (0x[0-9A-F]+)u", hdr).group(1), 16) == 0xFFFFFFFF
    # the kernel forms: the names in the source are the names the signature module lists
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_linkcomm.hip")).read()
    assert set(re.findall(FORM_RE, src)) == set(lc.KERNEL_FORMS)


def test_the_kernels_did_not_land_in_the_existing_library(lc):
    """libammsb_hip.so and its header are what the kernel census and the symbol test pin: no linkcomm name in either;
    the new library holds gfx950 code under the form names"""
    from mcmc_ammsb_gpu_amd import _capi
    assert not [n for n in _capi.SIGNATURES if "linkcomm" in n]
    assert "linkcomm" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    assert b"linkcomm" not in open(_capi.LIB_PATH, "rb").read()
    raw = open(lc.LIB_PATH, "rb").read()
    assert b"gfx950" in raw and b"linkcomm_fast" in raw and b"linkcomm_generic" in raw
    for form in lc.KERNEL_FORMS:
        assert form.encode() in raw, form
    import make_dry_run as dry
    assert dry.csrc_all_builds("../libammsb_linkcomm.so", "ammsb_linkcomm.o") and dry.csrc_all_builds("ammsb_linkcomm.o", "-c ammsb_linkcomm.hip")
    assert "ammsb_linkcomm" not in dry.hip_library_link()   # not part of libammsb_hip.so


def _rpm(rows, cols, rows_in_block=0, blocks=1, ptr=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for i in range(blocks):
        d.blocks[i] = ptr
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows_in_block or rows, rows, cols, blocks
    return d


def test_argument_errors_are_returned_before_anything_is_launched(lc):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    lib = lc.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments
    good = _rpm(100, 64)

    def call(d=good, beta=p, eps=1e-7, edges=p, n=8, T=4, min_term=0.0, ids=p, terms=p, prob=p, sizes=p):
        return lib.ammsb_linkcomm_edges(C.byref(d) if d is not None else None, beta, eps, edges, n, T, min_term, ids,
                                        terms, prob, sizes, None)

    assert call(d=None) == EINVAL and call(beta=None) == EINVAL and call(edges=None) == EINVAL
    assert call(ids=None, terms=None, prob=None, sizes=None) == EINVAL
    assert b"no output" in lib.ammsb_linkcomm_last_error()
    assert call(ids=None) == EINVAL and call(terms=None) == EINVAL
    assert call(ids=None, prob=None, sizes=None) == EINVAL and call(terms=None, sizes=None) == EINVAL
    for T in (0, 17, 1 << 20):
        assert call(T=T) == EINVAL
        assert b"T outside" in lib.ammsb_linkcomm_last_error()
    for min_term in (-1e-30, -1.0, float("nan"), float("inf"), -float("inf")):
        assert call(min_term=min_term) == EINVAL
        assert b"min_term" in lib.ammsb_linkcomm_last_error()
    for eps in (-1e-30, -1.0, float("nan"), 1.0, 2.0, float("inf")):
        assert call(eps=eps) == EINVAL
    assert call(d=_rpm(100, 0)) == EINVAL and call(d=_rpm(100, 8193)) == EINVAL
    assert call(d=_rpm(100, 64, rows_in_block=10, blocks=9)) == EINVAL      # 90 rows of blocks for 100 rows
    assert call(d=_rpm(100, 64, ptr=0)) == EINVAL and call(d=_rpm(2**32, 64)) == EINVAL
    # the same refusals in the sizes-only pass, where T is ignored
    assert call(ids=None, terms=None, prob=None, min_term=-1.0) == EINVAL
    assert call(ids=None, terms=None, prob=None, d=_rpm(100, 8193)) == EINVAL
    # n == 0 is a valid no-op, also without a device: nothing has been launched
    assert call(n=0) == 0 and call(n=0, edges=None) == 0 and call(n=0, ids=None, terms=None, prob=None, T=0) == 0
    assert call(n=0, T=0) == EINVAL and call(n=0, min_term=-1.0) == EINVAL and call(n=0, d=_rpm(100, 0)) == EINVAL
    assert lib.ammsb_linkcomm_last_kernel_name() == b""
    for top, min_term in ((0, 0.0), (17, 0.0), (-1, 0.0), (1, -1e-9), (1, float("nan")), (1, float("inf")), (1, 1e39)):
        with pytest.raises(AmmsbError):
            lc.check_args(top, min_term)
    assert lc.check_args(16, 0.1) == (16, float(np.float32(0.1))) and lc.check_args(1, 0) == (1, 0.0)


def test_file_round_trip_is_bit_exact(lc, tmp_path):
    rng = np.random.default_rng(10)
    E, T, N, K = 400, 16, 5000, 300
    ids = rng.integers(0, K, (E, T)).astype(np.uint32)
    bits = rng.integers(0x00000001, 0x3F800000, (E, T)).astype(np.uint32)   # every positive binary32 up to 1, subnormals too
    bits[0, :4] = [0x00000001, 0x007FFFFF, 0x00800000, 0x3F7FFFFF]
    terms = bits.view(np.float32).copy()
    fill = rng.integers(0, T + 1, E)
    fill[1] = 0      # a link no community explains: an "empty" line `a b p 0`
    for i in range(E):
        ids[i, fill[i]:], terms[i, fill[i]:] = lc.NONE, 0.0
    prob = rng.integers(0x00000001, 0x3F800000, E).astype(np.uint32).view(np.float32).copy()
    prob[2] = np.float32(-1.0)
    u, v = rng.integers(0, N, E).astype(np.uint64), rng.integers(0, N, E).astype(np.uint64)
    edges = np.sort((np.minimum(u, v) << np.uint64(32)) | np.maximum(u, v))
    min_term = np.uint32(0x00000003).view(np.float32)                        # a subnormal floor
    f = str(tmp_path / "lc.txt")
    lc.write_link_communities(f, N, K, T, min_term, edges, prob, ids.view(np.int32), terms)   # int32 ids as torch hands them over
    lines = open(f).read().splitlines()
    assert lines[0] == "# 5000 300 400 16 %s" % ("%.9g" % float(min_term)) and len(lines) == E + 1
    assert lines[2] == "%d %d %s 0" % (int(edges[1]) >> 32, int(edges[1]) & 0xFFFFFFFF, "%.9g" % float(prob[1]))
    N2, K2, T2, m2, edges2, prob2, ids2, terms2 = lc.read_link_communities(f)
    assert (N2, K2, T2) == (N, K, T) and np.float32(m2).view(np.uint32) == min_term.view(np.uint32)
    assert np.array_equal(edges2, edges) and np.array_equal(ids2, ids)
    assert np.array_equal(terms2.view(np.uint32), terms.view(np.uint32))
    assert np.array_equal(prob2.view(np.uint32), prob.view(np.uint32))
    # no links at all
    g = str(tmp_path / "none.txt")
    lc.write_link_communities(g, N, K, 1, 0.0, np.zeros(0, np.uint64), np.zeros(0, np.float32),
                              np.zeros((0, 1), np.int32), np.zeros((0, 1), np.float32))
    assert open(g).read() == "# 5000 300 0 1 0\n"
    got = lc.read_link_communities(g)
    assert got[:4] == (N, K, 1, 0.0) and got[4].size == 0 and got[6].shape == (0, 1) and got[7].shape == (0, 1)
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    bad = tmp_path / "bad.txt"
    bad.write_text("# 5 2 1 1 0\n0 1 0.5 2 0 0.25\n")
    with pytest.raises(AmmsbError):
        lc.read_link_communities(str(bad))


def test_no_cpu_path_without_a_gpu(lc, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.LinkCommunities(), lambda: lrn.LinkCommunities(np.zeros(3, np.uint64), top=4, min_term=0.1),
                 lambda: lrn.LinkCommunitySizes(), lambda: lrn.TrainingLinks()):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    with pytest.raises(AmmsbError):
        lrn.LinkCommunities(top=17)
    with pytest.raises(AmmsbError):
        lrn.LinkCommunitySizes(min_term=-1.0)
    assert hasattr(ops, "LinkCommunities")


def test_command_line_refuses_the_bad_combinations():
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(EXE)
    cases = [(["--link-communities-top", "3"], "need --link-communities-out"),
             (["--link-communities-min-term", "0.1"], "need --link-communities-out"),
             (["--link-communities-out", "x.txt", "--link-communities-top", "0"], "--link-communities-top must be in 1..16"),
             (["--link-communities-out", "x.txt", "--link-communities-top", "17"], "--link-communities-top must be in 1..16"),
             (["--link-communities-out", "x.txt", "--link-communities-min-term", "-0.5"], "--link-communities-min-term must be"),
             (["--link-communities-out", "x.txt", "--link-communities-min-term", "nan"], "")]
    for args, msg in cases:
        r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stderr[-500:])
        assert any(ln.startswith("F ") and msg in ln for ln in r.stderr.splitlines()), (args, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, args
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    for flag, default in (("link-communities-out", None), ("link-communities-top", "1"), ("link-communities-min-term", "0")):
        assert re.search(r"--%s arg%s" % (flag, r" \(=%s " % default if default else ""), r.stdout), flag
    # a good combination gets past the flag checks (and stops at the missing file, like any run)
    r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt", "--link-communities-out", "x.txt", "--link-communities-top", "16",
                        "--link-communities-min-term", "0.001"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Failed to detect file" in r.stderr


def test_build_and_link_lines_carry_the_new_library():
    import make_dry_run as dry
    links = dry.host_links()   # (every one of them carries every device library)
    assert len(links) >= 9 and all("-lammsb_linkcomm" in ln for ln in links)     # the ASan variants included
    assert dry.host_all_builds("../linkcomm_test", "tests/cpp/linkcomm_test.cc")
    asan = open(os.path.join(ROOT, "tools", "run_asan.sh")).read()
    assert "tests/test_linkcomm_host.py" in asan
    assert "linkcomm_test" in open(os.path.join(ROOT, ".gitignore")).read().split()
