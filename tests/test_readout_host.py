"""Host half of the read-out (include/ammsb_readout.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, and the existing library's yardsticks untouched), argument errors returned before anything
is launched, the community CSR builder against a numpy statement, the communities file written and parsed back, the
refused command-line combinations, and that no layer has a CPU path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EXE = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "ammsb_main")
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def ro():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _readout
    _readout.load()
    return _readout


def test_header_exports_and_signature_table_agree(ro):
    hdr = open(os.path.join(ROOT, "include", "ammsb_readout.h")).read()
    declared = set(re.findall(r"\b(ammsb_readout_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(ro.SIGNATURES), declared ^ set(ro.SIGNATURES)
    lib = C.CDLL(ro.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    # the library exports no other function of its own (kernel stubs are local: anonymous namespace)
    own = exported_symbols(ro.LIB_PATH)
    assert own == declared, own ^ declared
    assert (ro.MAX_TOP, ro.MAX_COLS) == tuple(int(re.search(r"#define %s (\d+)u" % n, hdr).group(1))
                                              for n in ("AMMSB_READOUT_MAX_TOP", "AMMSB_READOUT_MAX_COLS"))


def test_the_kernels_did_not_land_in_the_existing_library(ro):
    """libammsb_hip.so and its header are what the kernel census and the symbol test pin: no read-out name in either"""
    from mcmc_ammsb_gpu_amd import _capi
    assert not [n for n in _capi.SIGNATURES if "readout" in n]
    assert "readout" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    raw = open(_capi.LIB_PATH, "rb").read()
    assert b"readout_fast" not in raw and b"readout_generic" not in raw
    raw = open(ro.LIB_PATH, "rb").read()
    assert b"readout_fast" in raw and b"readout_generic" in raw and b"gfx950" in raw


def _rpm(rows, cols, rows_in_block=0, blocks=1, ptr=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for i in range(blocks):
        d.blocks[i] = ptr
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows_in_block or rows, rows, cols, blocks
    return d


def test_argument_errors_are_returned_before_anything_is_launched(ro):
    lib = ro.load()
    out = 0x2000   # never dereferenced: every call below is refused on its arguments

    def call(d, T=4, thr=0.0, lo=0, n=10, nodes=None, ids=out, weights=out, count=out, sizes=None):
        return lib.ammsb_readout_top(C.byref(d) if d is not None else None, nodes, lo, n, T, thr, ids, weights, count,
                                     sizes, None)
    good = _rpm(100, 64)
    for T in (0, 17, 1 << 20):
        assert call(good, T=T) == EINVAL
        assert b"T outside" in lib.ammsb_readout_last_error()
    for thr in (-1e-30, -1.0, float("nan"), float("-inf")):
        assert call(good, thr=thr) == EINVAL
    assert call(good, lo=91, n=10) == EINVAL and call(good, lo=101, n=0) == EINVAL and call(good, lo=0, n=101) == EINVAL
    assert call(good, lo=2**63, n=2**63) == EINVAL                       # the sum wraps; still past num_rows
    assert call(good, ids=None) == EINVAL and call(good, weights=None) == EINVAL and call(good, count=None) == EINVAL
    assert call(good, ids=None, weights=None, count=None, sizes=None) == EINVAL   # nothing to write
    assert call(_rpm(100, 0)) == EINVAL and call(_rpm(100, 8193)) == EINVAL
    assert call(good, nodes=out, lo=1) == EINVAL
    assert call(None) == EINVAL
    assert call(_rpm(100, 64, rows_in_block=10, blocks=9)) == EINVAL      # 90 rows of blocks for 100 rows
    assert call(_rpm(100, 64, ptr=0)) == EINVAL
    assert call(_rpm(2**32, 64)) == EINVAL
    # n_rows == 0 is a valid no-op, also without a device
    assert call(good, n=0) == 0 and call(good, lo=100, n=0) == 0
    assert lib.ammsb_readout_last_kernel_name() == b""
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    for top, thr in ((0, 0.0), (17, 0.0), (4, -0.5), (4, float("nan"))):
        with pytest.raises(AmmsbError):
            ro.check_args(top, thr)
    assert ro.check_args(16, 0.0) == (16, 0.0)


def _numpy_csr(ids, K, nodes=None):
    """the definition: community k's members are the nodes with k in a slot, ascending, once per slot"""
    who = np.arange(ids.shape[0]) if nodes is None else np.asarray(nodes)
    members = [np.sort(np.repeat(who, (ids == k).sum(1))) for k in range(K)]
    offsets = np.concatenate([[0], np.cumsum([m.size for m in members])]).astype(np.int64)
    return offsets, np.concatenate(members).astype(np.int32)


@pytest.mark.parametrize("seed", range(6))
def test_community_csr_equals_the_numpy_statement(ro, seed):
    rng = np.random.default_rng(seed)
    n, T, K = int(rng.integers(1, 400)), int(rng.integers(1, 17)), int(rng.integers(1, 70))
    ids = rng.integers(0, K, (n, T)).astype(np.uint32)
    ids[rng.random((n, T)) < 0.4] = ro.NONE                      # sentinels, anywhere
    ids[ids == (seed % K)] = ro.NONE                             # an empty community
    ids[1:][rng.random(n - 1) < 0.3] = ids[0]                    # duplicates across rows
    off, mem = ro.communities_csr(ids, K)
    woff, wmem = _numpy_csr(ids, K)
    assert off.dtype == np.int64 and mem.dtype == np.int32 and off.shape == (K + 1,)
    assert np.array_equal(off, woff) and np.array_equal(mem, wmem)
    assert off[seed % K] == off[seed % K + 1]
    # int32 ids as torch hands them over (-1 = empty), and a node list
    off2, mem2 = ro.communities_csr(ids.view(np.int32), K)
    assert np.array_equal(off2, off) and np.array_equal(mem2, mem)
    nodes = rng.permutation(10 * n)[:n]
    off3, mem3 = ro.communities_csr(ids, K, nodes=nodes)
    woff3, wmem3 = _numpy_csr(ids, K, nodes)
    assert np.array_equal(off3, woff3) and np.array_equal(mem3, wmem3)
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    with pytest.raises(AmmsbError):
        ro.communities_csr(np.array([[K]], dtype=np.uint32), K)


def test_communities_file_round_trip(ro, tmp_path):
    rng = np.random.default_rng(9)
    n, T, K = 300, 3, 20
    ids = rng.integers(0, K, (n, T)).astype(np.uint32)
    ids[rng.random((n, T)) < 0.5] = ro.NONE
    ids[ids == 7] = ro.NONE
    off, mem = ro.communities_csr(ids, K)
    sizes = np.diff(off) + rng.integers(0, 5, K)
    f = str(tmp_path / "c.txt")
    ro.write_communities(f, n, K, T, np.float32(0.05), sizes, off, mem)
    lines = open(f).read().splitlines()
    assert lines[0] == "# 300 20 3 0.0500000007" and len(lines) == K + 1 and lines[8] == "7 %d" % sizes[7]
    N2, K2, T2, thr, sizes2, off2, mem2 = ro.read_communities(f)
    assert (N2, K2, T2) == (n, K, T) and np.float32(thr) == np.float32(0.05)
    assert np.array_equal(sizes2, sizes) and np.array_equal(off2, off) and np.array_equal(mem2, mem)


def test_command_line_refuses_the_bad_combinations():
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(EXE)
    cases = [(["--membership-top", "3"], "need --communities-out"),
             (["--membership-threshold", "0.1"], "need --communities-out"),
             (["--communities-out", "x.txt", "--membership-top", "0"], "--membership-top must be in 1..16"),
             (["--communities-out", "x.txt", "--membership-top", "17"], "--membership-top must be in 1..16"),
             (["--communities-out", "x.txt", "--membership-threshold", "-0.25"], "--membership-threshold must be >= 0")]
    for args, msg in cases:
        r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stderr[-500:])
        assert any(ln.startswith("F ") and msg in ln for ln in r.stderr.splitlines())
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    for flag, default in (("communities-out", None), ("membership-top", "4"), ("membership-threshold", "0")):
        assert re.search(r"--%s arg%s" % (flag, r" \(=%s " % default if default else ""), r.stdout), flag
    # a good combination gets past the flag checks (and stops at the missing file, like any run)
    r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt", "--communities-out", "x.txt", "--membership-top", "16",
                        "--membership-threshold", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Failed to detect file" in r.stderr


def test_no_cpu_path_without_a_gpu(ro, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.Memberships(4, 0.0), lambda: lrn.CommunitySizes(0.1), lambda: lrn.Communities()):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    with pytest.raises(AmmsbError):
        lrn.Memberships(17, 0.0)
    with pytest.raises(AmmsbError, match="no HIP device"):
        ops.Context(ops.make_params(100, 8, E=100))
    assert hasattr(ops, "CommunityReadout")


def test_build_and_link_lines_carry_the_new_library():
    import make_dry_run as dry
    links = [ln for ln in dry.commands("host", "all", "asan") if "-lammsb_refsample" in ln]
    assert links and all("-lammsb_readout" in ln for ln in links)     # the ASan variants included
    assert dry.csrc_all_builds("../libammsb_readout.so", "ammsb_readout.o") and dry.csrc_all_builds("ammsb_readout.o", "-c ammsb_readout.hip")
    assert "ammsb_readout" not in dry.hip_library_link()   # not part of libammsb_hip.so
