"""Host half of link prediction (include/ammsb_linkpred.h), no GPU: the drop-in boundary of the new library (header ==
exports == signature table, and the existing library's yardsticks untouched), argument errors returned before anything
is launched, the AUC helper against a brute-force count over all (link, non-link) pairs, the links file written and
parsed back bit for bit, and that no layer has a CPU path."""
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
ERANGE = -5  # AMMSB_ERANGE
EXE = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "ammsb_main")


@pytest.fixture(scope="module")
def lp():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _linkpred
    _linkpred.load()
    return _linkpred


def test_header_exports_and_signature_table_agree(lp):
    hdr = open(os.path.join(ROOT, "include", "ammsb_linkpred.h")).read()
    declared = set(re.findall(r"\b(ammsb_linkpred_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(lp.SIGNATURES), declared ^ set(lp.SIGNATURES)
    lib = C.CDLL(lp.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(lp.LIB_PATH)
    assert own == declared, own ^ declared
    assert (lp.MAX_TOP, lp.MAX_COLS) == tuple(int(re.search(r"#define %s (\d+)u" % n, hdr).group(1))
                                              for n in ("AMMSB_LINKPRED_MAX_TOP", "AMMSB_LINKPRED_MAX_COLS"))
    assert lp.NONE == int(re.search(r"#define AMMSB_LINKPRED_NONE (0x[0-9A-F]+)u", hdr).group(1), 16)
    # the kernel forms: the names in the source are the names the signature module lists
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_linkpred.hip")).read()
    assert set(re.findall(r'"(linkpred_(?:block|top|pairs)_[a-z0-9_]+)"', src)) == set(lp.KERNEL_FORMS)


def test_the_kernels_did_not_land_in_the_existing_library(lp):
    """libammsb_hip.so and its header are what the kernel census and the symbol test pin: no linkpred name in either;
    the new library holds gfx950 code, on the matrix core"""
    from mcmc_ammsb_gpu_amd import _capi
    assert not [n for n in _capi.SIGNATURES if "linkpred" in n]
    assert "linkpred" not in open(os.path.join(ROOT, "include", "ammsb.h")).read()
    assert b"linkpred" not in open(_capi.LIB_PATH, "rb").read()
    raw = open(lp.LIB_PATH, "rb").read()
    assert b"gfx950" in raw and b"linkpred_top_mfma_q128_v4" in raw and b"linkpred_tile" in raw
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_linkpred.hip")).read()
    assert "__builtin_amdgcn_mfma_f32_32x32x2f32" in src
    import make_dry_run as dry
    assert dry.csrc_all_builds("../libammsb_linkpred.so", "ammsb_linkpred.o") and dry.csrc_all_builds("ammsb_linkpred.o", "-c ammsb_linkpred.hip")
    assert "ammsb_linkpred" not in dry.hip_library_link()   # not part of libammsb_hip.so


def test_the_matrix_core_instruction_is_in_the_code_object(lp, tmp_path):
    """the f32-input MFMA is what the device code executes, not only what the source names"""
    tool = next((p for p in ("/opt/rocm/llvm/bin/clang-offload-bundler", "/opt/rocm/lib/llvm/bin/clang-offload-bundler")
                 if os.path.exists(p)), None)
    objdump = next((p for p in ("/opt/rocm/llvm/bin/llvm-objdump", "/opt/rocm/lib/llvm/bin/llvm-objdump")
                    if os.path.exists(p)), None)
    if not (tool and objdump):
        pytest.fail("no clang-offload-bundler / llvm-objdump next to hipcc")
    raw = open(lp.LIB_PATH, "rb").read()
    at = raw.find(b"__CLANG_OFFLOAD_BUNDLE__")
    assert at >= 0
    bundle = tmp_path / "bundle.bin"
    bundle.write_bytes(raw[at:])
    co = tmp_path / "gfx950.co"
    r = subprocess.run([tool, "--unbundle", "--type=o", "--input=%s" % bundle, "--output=%s" % co,
                        "--targets=hipv4-amdgcn-amd-amdhsa--gfx950"], capture_output=True, text=True)
    assert r.returncode == 0 and co.exists(), r.stderr[-2000:]
    dis = subprocess.run([objdump, "-d", str(co)], capture_output=True, text=True, check=True).stdout
    assert dis.count("v_mfma_f32_32x32x2_f32") >= 8 * 32   # 8 instances of the tile kernel, 32 per chunk each


def _rpm(rows, cols, rows_in_block=0, blocks=1, ptr=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for i in range(blocks):
        d.blocks[i] = ptr
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rows_in_block or rows, rows, cols, blocks
    return d


def test_argument_errors_are_returned_before_anything_is_launched(lp):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError, SetDesc
    lib = lp.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments
    good = _rpm(100, 64)
    big_ws = 1 << 40

    def top(d=good, beta=p, eps=1e-7, q=p, Q=8, T=10, e0=None, e1=None, lo=0, n=100, ids=p, scores=p, ws=p, ws_bytes=big_ws):
        return lib.ammsb_linkpred_top(C.byref(d) if d is not None else None, beta, eps, q, Q, T, e0, e1, lo, n, ids,
                                      scores, ws, ws_bytes, None)

    def block(d=good, beta=p, eps=1e-7, q=p, Q=8, lo=0, n=100, out=p):
        return lib.ammsb_linkpred_block(C.byref(d) if d is not None else None, beta, eps, q, Q, lo, n, out, None)

    def pairs(d=good, beta=p, eps=1e-7, edges=p, n=8, out=p):
        return lib.ammsb_linkpred_pairs(C.byref(d) if d is not None else None, beta, eps, edges, n, out, None)

    for T in (0, 65, 1 << 20):
        assert top(T=T) == EINVAL
        assert b"T outside" in lib.ammsb_linkpred_last_error()
    for eps in (-1e-30, -1.0, float("nan"), 1.0, 2.0, float("inf")):
        assert top(eps=eps) == EINVAL and block(eps=eps) == EINVAL and pairs(eps=eps) == EINVAL
    for call in (top, block):
        assert call(lo=91, n=10) == EINVAL and call(lo=101, n=0) == EINVAL and call(lo=0, n=101) == EINVAL
        assert call(lo=2**63, n=2**63) == EINVAL and call(lo=2**64 - 1, n=2) == EINVAL   # the sum wraps
    for call in (top, block, pairs):
        assert call(d=_rpm(100, 0)) == EINVAL and call(d=_rpm(100, 8193)) == EINVAL
        assert call(d=_rpm(100, 64, rows_in_block=10, blocks=9)) == EINVAL      # 90 rows of blocks for 100 rows
        assert call(d=_rpm(100, 64, ptr=0)) == EINVAL and call(d=_rpm(2**32, 64)) == EINVAL
        assert call(d=None) == EINVAL and call(beta=None) == EINVAL
    assert top(ids=None) == EINVAL and top(scores=None) == EINVAL and top(q=None) == EINVAL
    assert block(out=None) == EINVAL and block(q=None) == EINVAL
    assert pairs(out=None) == EINVAL and pairs(edges=None) == EINVAL
    # candidate indices are 32-bit inside a tile: a range within 256 of 2^32 is refused, not wrapped
    huge = _rpm(2**32 - 1, 1)
    assert top(d=huge, n=2**32 - 256) == ERANGE and block(d=huge, n=2**32 - 1) == ERANGE
    # the workspace: NULL, misaligned, one byte short of what the library asks for
    need = lib.ammsb_linkpred_top_workspace_bytes(8, 10, 100, 64)
    assert need >= 8 * 10 * 8
    assert top(ws=None) == EINVAL and top(ws=0x2008) == EINVAL and top(ws_bytes=need - 1) == EINVAL
    assert b"workspace" in lib.ammsb_linkpred_last_error()
    assert lib.ammsb_linkpred_top_workspace_bytes(1024, 64, 10**6, 1024) <= 192 << 20   # bounded: a fixed grid of lists
    assert lib.ammsb_linkpred_top_workspace_bytes(200, 10, 5000, 64) > lib.ammsb_linkpred_top_workspace_bytes(1, 10, 5000, 64)
    bad_set = SetDesc(None, 10, 0)
    assert top(e0=C.byref(bad_set)) == EINVAL and top(e1=C.byref(SetDesc(p, 0, 0))) == EINVAL
    # empty calls are valid no-ops, also without a device
    assert top(Q=0) == 0 and block(Q=0) == 0 and block(n=0) == 0 and pairs(n=0) == 0
    assert lib.ammsb_linkpred_last_kernel_name() == b""
    for T in (0, 65, -1):
        with pytest.raises(AmmsbError):
            lp.check_top(T)
    assert lp.check_top(64) == 64
    assert lp.check_exclude(("heldout", "training")) == ("training", "heldout") and lp.check_exclude(()) == ()
    assert lp.check_exclude("training") == ("training",)
    with pytest.raises(AmmsbError):
        lp.check_exclude(("training", "test"))


def _brute_auc(scores, labels):
    """the definition: the fraction of (link, non-link) pairs ordered correctly, a tie counting one half"""
    s = np.asarray(scores, dtype=np.float64)
    pos, neg = s[labels], s[~labels]
    d = pos[:, None] - neg[None, :]
    return ((d > 0).sum() + 0.5 * (d == 0).sum()) / float(pos.size * neg.size)


@pytest.mark.parametrize("seed", range(6))
def test_auc_equals_the_count_over_all_pairs(lp, seed):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    rng = np.random.default_rng(seed)
    n = int(rng.integers(2, 700))
    labels = rng.random(n) < rng.uniform(0.05, 0.95)
    labels[0], labels[1] = True, False
    levels = int(rng.integers(1, 40)) if seed % 2 else 10**6        # odd seeds: heavy ties, within and across classes
    scores = (rng.integers(0, levels, n) / levels + labels * rng.uniform(0, 0.3)).astype(np.float32)
    if seed % 2:
        scores = np.round(scores, 1)
    got = lp.auc(scores, labels)
    assert abs(got - _brute_auc(scores, labels)) <= 1e-12
    assert abs(lp.auc(scores, ~labels) - (1.0 - got)) <= 1e-12
    assert lp.auc(np.where(labels, 2.0, 1.0), labels) == 1.0 and lp.auc(np.where(labels, 1.0, 2.0), labels) == 0.0
    assert lp.auc(np.ones(n), labels) == 0.5
    for bad in (np.ones(n, bool), np.zeros(n, bool)):
        with pytest.raises(AmmsbError, match="links and non-links"):
            lp.auc(scores, bad)


def test_links_file_round_trip_is_bit_exact(lp, tmp_path):
    rng = np.random.default_rng(9)
    Q, T, N, K = 300, 10, 5000, 20
    ids = rng.integers(0, N, (Q, T)).astype(np.uint32)
    bits = rng.integers(0x00000001, 0x3F800000, (Q, T)).astype(np.uint32)   # every positive binary32 up to 1, subnormals too
    bits[0, :4] = [0x00000001, 0x007FFFFF, 0x00800000, 0x3F7FFFFF]
    scores = bits.view(np.float32).copy()
    fill = rng.integers(0, T + 1, Q)
    fill[1] = 0
    for i in range(Q):
        ids[i, fill[i]:], scores[i, fill[i]:] = lp.NONE, 0.0
    nodes = rng.integers(0, N, Q).astype(np.uint32)
    f = str(tmp_path / "links.txt")
    lp.write_links(f, N, K, T, "all", nodes, ids.view(np.int32), scores)   # int32 ids as torch hands them over
    lines = open(f).read().splitlines()
    assert lines[0] == "# 5000 20 10 all" and len(lines) == Q + 1 and lines[2] == "%d 0" % nodes[1]
    N2, K2, T2, ex, nodes2, ids2, scores2 = lp.read_links(f)
    assert (N2, K2, T2, ex) == (N, K, T, "all")
    assert np.array_equal(nodes2, nodes) and np.array_equal(ids2, ids)
    assert np.array_equal(scores2.view(np.uint32), scores.view(np.uint32))


def test_no_cpu_path_without_a_gpu(lp, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    for call in (lambda: lrn.PredictLinks([1, 2, 3]), lambda: lrn.LinkProbabilities(np.zeros(3, np.uint64)),
                 lambda: lrn.HeldoutAUC()):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    with pytest.raises(AmmsbError):
        lrn.PredictLinks([1], top=65)
    with pytest.raises(AmmsbError):
        lrn.PredictLinks([1], exclude=("everything",))
    assert hasattr(ops, "LinkPredictor")


def test_command_line_refuses_the_bad_combinations(tmp_path):
    import __graft_entry__ as ge
    ge.build()
    assert os.path.exists(EXE)
    nodes = tmp_path / "nodes.txt"
    nodes.write_text("1\n2\n3\n")
    junk = tmp_path / "junk.txt"
    junk.write_text("1\ntwo\n")
    big = tmp_path / "big.txt"
    big.write_text("1\n4294967296\n")
    cases = [(["--links-top", "3"], "need --links-out"),
             (["--links-nodes", str(nodes)], "need --links-out"),
             (["--links-exclude", "none"], "need --links-out"),
             (["--links-out", "x.txt", "--links-top", "0"], "--links-top must be in 1..64"),
             (["--links-out", "x.txt", "--links-top", "65"], "--links-top must be in 1..64"),
             (["--links-out", "x.txt", "--links-exclude", "heldout-only"], "--links-exclude must be none, training or all"),
             (["--links-out", "x.txt", "--links-nodes", str(tmp_path / "missing.txt")], "cannot read --links-nodes"),
             (["--links-out", "x.txt", "--links-nodes", str(junk)], "not a node id"),
             (["--links-out", "x.txt", "--links-nodes", str(big)], "not a node id")]
    for args, msg in cases:
        r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt"] + args, capture_output=True, text=True, timeout=60)
        assert r.returncode == 2, (args, r.stderr[-500:])
        assert any(ln.startswith("F ") and msg in ln for ln in r.stderr.splitlines()), (args, r.stderr[-500:])
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True, timeout=60)
    for flag, default in (("links-out", None), ("links-top", "10"), ("links-nodes", None), ("links-exclude", None)):
        assert re.search(r"--%s arg%s" % (flag, r" \(=%s " % default if default else ""), r.stdout), flag
    # a good combination gets past the flag checks (and stops at the missing file, like any run)
    r = subprocess.run([EXE, "-f", "/nonexistent/graph.txt", "--links-out", "x.txt", "--links-top", "64", "--links-nodes",
                        str(nodes), "--links-exclude", "training"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "Failed to detect file" in r.stderr
    # an id >= N is refused once N is known (a real run: the GPU group `cpp` of tests/test_gpu_linkpred.py)


def test_build_and_link_lines_carry_the_new_library():
    import make_dry_run as dry
    links = [ln for ln in dry.commands("host", "all", "asan") if "-lammsb_refsample" in ln]
    assert links and all("-lammsb_linkpred" in ln for ln in links)     # the ASan variants included
    asan = open(os.path.join(ROOT, "tools", "run_asan.sh")).read()
    assert "tests/test_linkpred_host.py" in asan
