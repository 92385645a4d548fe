"""Host half of the triangles inside the detected communities (include/ammsb_triangles.h), no GPU: the statement the GPU
tests compare against (triangles_statement.py) checked against powers of the dense adjacency, the derived measures from
hand-made integers, the simplification of an adjacency, the triangles file written and parsed back byte for byte, argument
errors returned before anything is launched, the drop-in boundary of the new library (header == exports == signature
table, built by build()), the command line's flag rules, and that no layer has a CPU path."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import triangles_statement as ts
from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
PKG = os.path.join(ROOT, "mcmc-ammsb-gpu_amd")
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def tr():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _triangles
    _triangles.load()
    return _triangles


def test_the_statement_equals_the_powers_of_the_dense_adjacency():
    rng = np.random.default_rng(5)
    for N, K, p, q in ((1, 1, 0.5, 0.5), (7, 3, 0.6, 0.6), (40, 5, 0.2, 0.4), (60, 70, 0.15, 0.2), (55, 64, 0.3, 1.0), (30, 65, 0.9, 0.5)):
        pairs = np.argwhere(np.triu(rng.random((N, N)) < p, 1))
        off, tgt = ts.csr_of_pairs(pairs, N, lead=3)
        M = rng.random((N, K)) < q
        if N > 5:
            M[5] = False   # a node without a community
        s = ts.statement(M, off, tgt)
        A = ts.dense(off, tgt, N)
        assert (A == A.T).all() and not np.diagonal(A).any() and A.sum() == 2 * len(pairs)
        cube = np.linalg.matrix_power(A, 3)
        assert np.array_equal(s["tri"], np.diagonal(cube) // 2) and s["counts"] == [int(np.trace(cube)) // 2, 0]
        assert np.array_equal(s["degree"], A.sum(1))
        tk = np.zeros((N, K), np.int64)
        for k in range(K):
            Ak = A * np.outer(M[:, k], M[:, k])
            ck = np.linalg.matrix_power(Ak, 3)
            tk[:, k] = np.diagonal(ck) // 2
            assert s["ktri3"][k] == int(np.trace(ck)) // 2 and s["ktri3"][k] % 3 == 0, (N, K, k)
            assert s["kpart"][k] == int((np.diagonal(ck) > 0).sum()), (N, K, k)
            c = Ak.sum(1)   # neighbours in k of the members of k
            assert s["wedges"][k] == int((c * (c - 1) // 2).sum()) and s["kmembers"][k] == int(M[:, k].sum())
        assert np.array_equal(s["tri_comms"], (tk > 0).sum(1))
        # tri_in: the triangles at a with a shared community, counted pair by pair
        for a in range(N):
            nb = np.flatnonzero(A[a])
            want = sum(1 for i, b in enumerate(nb) for c in nb[i + 1:] if A[b, c] and (M[a] & M[b] & M[c]).any())
            assert s["tri_in"][a] == want, (N, K, a)
        # a range of nodes: its entries, and the sums over it
        if N > 10:
            part = ts.statement(M, off, tgt, 4, N - 9)
            assert all(np.array_equal(part[n], s[n][4:N - 5]) for n in ts.NODE + ("degree",))
            assert part["ktri3"] == tk[4:N - 5].sum(0).tolist() and part["kpart"] == (tk[4:N - 5] > 0).sum(0).tolist()


def test_derived_measures_on_hand_made_integers(tr):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    # a triangle 0 1 2 with a tail 3 at node 2, all in community 0; node 4 alone; community 1 is a chain of three, 2 empty
    r = tr.Triangles(0.05, [2, 2, 3, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [3, 0, 0], [3, 0, 0], [4, 3, 0],
                     [5, 1, 0], 8, 1, 2, N=5)
    assert r.tpr.tolist() == [0.75, 0.0, -1.0] and r.clustering.tolist() == [3.0 / 5.0, 0.0, -1.0]
    assert r.triangles.tolist() == [1, 0, 0] and r.triangles.dtype == np.uint64 and r.total == 1 and r.whole
    assert r.local_clustering.tolist() == [1.0, 1.0, 1.0 / 3.0, -1.0, -1.0] and r.inside.tolist() == [1.0, 1.0, 1.0, -1.0, -1.0]
    assert r.transitivity == 3.0 / 5.0 and r.avg_clustering == (1.0 + 1.0 + 1.0 / 3.0) / 3.0
    assert r.without_triangles().tolist() == [1] and r.without_triangles(4).tolist() == [] and r.without_triangles(0).tolist() == [1, 2]
    assert all(x.dtype == np.float64 for x in (r.tpr, r.clustering, r.local_clustering, r.inside)) and "Triangles" in repr(r)
    # no node with two neighbours, no wedge, no triangle: every -1
    e = tr.Triangles(0.0, [1, 1], [0, 0], [0, 0], [0, 0], [0], [0], [0], [0], 2, 0, 0, N=2)
    assert e.transitivity == -1.0 and e.avg_clustering == -1.0 and e.tpr.tolist() == [-1.0] and e.total == 0
    assert e.local_clustering.tolist() == [-1.0, -1.0] and e.inside.tolist() == [-1.0, -1.0]
    # a triangle outside every shared community: inside is 0, not -1
    assert tr.Triangles(0.0, [2, 2, 2], [1, 1, 1], [0, 0, 0], [0, 0, 0], [0], [0], [1], [0], 6, 0, 0, N=3).inside.tolist() == [0.0] * 3
    # over all nodes 3 divides ktri3 and the sum of tri; over a range it need not
    for bad in (lambda: tr.Triangles(0.0, [2, 2, 2], [1, 1, 1], [1, 1, 1], [1, 1, 1], [4], [3], [3], [3], 6, 0, 0, N=3),
                lambda: tr.Triangles(0.0, [2, 2, 2], [1, 1, 0], [1, 1, 0], [1, 1, 0], [3], [3], [3], [3], 6, 0, 0, N=3),
                lambda: tr.derive([2], [1], [1], [2], [1], [1], [1])):
        with pytest.raises(AmmsbError, match="multiple of 3"):
            bad()
    part = tr.Triangles(0.0, [2, 2], [1, 1], [1, 1], [1, 1], [2], [2], [2], [2], 6, 0, 0, N=3, first=1)
    assert not part.whole and part.triangles.tolist() == [0] and part.total == 0 and part.tpr.tolist() == [1.0]
    for bad in (lambda: tr.Triangles(0.0, [2], [1, 1], [1], [1], [3], [1], [1], [1], 2, 0, 0),
                lambda: tr.Triangles(0.0, [2], [1], [2], [1], [3], [1], [1], [1], 2, 0, 0),     # tri_in > tri
                lambda: tr.Triangles(0.0, [2], [1], [1], [1], [3], [2], [1], [1], 2, 0, 0),     # kpart > kmembers
                lambda: tr.Triangles(0.0, [2], [1], [1], [1], [3], [1], [1, 1], [1], 2, 0, 0),
                lambda: tr.Triangles(0.0, [2], [1], [1], [1], [3], [1], [1], [1], -2, 0, 0),
                lambda: tr.Triangles(0.0, [2 ** 32], [1], [1], [1], [3], [1], [1], [1], 2, 0, 0)):
        with pytest.raises(AmmsbError):
            bad()
    assert tr.check_nodes(None, 7) == (0, 7) and tr.check_nodes((2, 5), 7) == (2, 5) and tr.check_nodes((7, 0), 7) == (7, 0)
    assert tr.check_rows(65535) == 65535 and tr.check_threshold(0) == 0.0 and tr.check_threshold(0.05) == float(np.float32(0.05))
    for bad in (lambda: tr.check_nodes((2, 6), 7), lambda: tr.check_nodes((-1, 2), 7), lambda: tr.check_nodes(3, 7),
                lambda: tr.check_rows(65536), lambda: tr.check_threshold(-1e-9), lambda: tr.check_threshold(float("nan")),
                lambda: tr.check_threshold(float("inf")), lambda: tr.check_threshold(1e39)):
        with pytest.raises(AmmsbError):
            bad()


def test_the_simplification_handles_repeats_loops_both_orders_and_ends_past_n(tr):
    key = lambda a, b: (a << 32) | b   # noqa: E731
    keys = np.array([key(0, 1), key(1, 0), key(2, 1), key(2, 1), key(3, 3), key(4, 0), key(0, 5), key(9, 9), key(2 ** 32 - 1, 1), key(0, 2)],
                    dtype=np.uint64)
    off, tgt, skipped, dropped = tr.simple_csr_of_keys(keys, 5)
    assert off.dtype == np.uint64 and tgt.dtype == np.uint32
    assert off.tolist() == [0, 3, 5, 7, 7, 8] and tgt.tolist() == [1, 2, 4, 0, 2, 0, 1, 0]
    assert (skipped, dropped) == (3, 3)   # 0-5, 9-9 and the end 2^32 - 1; 1-0 again, 2-1 again, the loop 3-3
    # the same graph as a CSR with unsorted rows, a repeat, a loop and a target >= N, offsets[0] > 0
    o2, t2, s2, d2 = tr.simple_csr_host([2, 6, 7, 9, 10, 11], [77, 77, 4, 2, 1, 1, 2, 1, 0, 3, 0, 99], 5)
    assert o2.tolist() == off.tolist() and t2.tolist() == tgt.tolist() and s2 == 0 and d2 == 9 - 4
    o3, t3, s3, d3 = tr.simple_csr_host([0, 1, 1], [7], 2)
    assert o3.tolist() == [0, 0, 0] and t3.size == 0 and (s3, d3) == (1, 0)
    # what it gives is what the statement takes: a triangle 0 1 2 and the pendant 4
    s = ts.statement(np.ones((5, 1), bool), off, tgt)
    assert s["tri"].tolist() == [1, 1, 1, 0, 0] and s["ktri3"] == [3] and s["kpart"] == [3] and s["wedges"] == [3 + 1 + 1 + 0 + 0]
    e = tr.simple_csr_of_keys(np.zeros(0, np.uint64), 3)
    assert e[0].tolist() == [0, 0, 0, 0] and e[1].size == 0 and e[2:] == (0, 0)


def _hand(tr):
    return tr.Triangles(0.05, [2, 2, 3, 1, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [1, 1, 1, 0, 0], [3, 0], [3, 0], [4, 3], [5, 1], 8, 1, 2, N=5)


def test_the_triangles_file_round_trips_byte_for_byte(tr, tmp_path):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    r = _hand(tr)
    path, again = str(tmp_path / "triangles.txt"), str(tmp_path / "again.txt")
    tr.write_triangles(path, 5, r)
    lines = open(path).read().splitlines()
    assert lines[0] == "# 5 2 8 0.0500000007 1 2 1" and len(lines) == 1 + 2 + 5
    assert lines[1] == "c 0 4 3 3 5" and lines[2] == "c 1 3 0 0 1" and lines[5] == "n 2 3 1 1 1" and lines[7] == "n 4 0 0 0 0"
    N, back = tr.read_triangles(path)
    assert N == 5 and (back.M, back.skipped, back.dropped, back.total, back.first) == (8, 1, 2, 1, 0)
    assert back.threshold == float(np.float32(0.05)) and np.array_equal(back.tri_in, r.tri_in) and np.array_equal(back.wedges, r.wedges)
    assert back.tpr.tobytes() == r.tpr.tobytes() and back.local_clustering.tobytes() == r.local_clustering.tobytes()
    tr.write_triangles(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    # a range of nodes, sums past 2^32
    part = tr.Triangles(0.0, [3, 0], [2, 0], [1, 0], [1, 0], [2 ** 63], [5], [5_000_000_000], [2 ** 64 - 1], 2 ** 40, 0, 7,
                        N=5_000_000_000, first=4_999_999_998)
    tr.write_triangles(path, 5_000_000_000, part)
    assert open(path).read() == ("# 5000000000 1 %d 0 0 7 0\nc 0 5000000000 5 %d %d\nn 4999999998 3 2 1 1\nn 4999999999 0 0 0 0\n"
                                 % (2 ** 40, 2 ** 63, 2 ** 64 - 1))
    N, back = tr.read_triangles(path)
    assert N == 5_000_000_000 and back.first == 4_999_999_998 and back.wedges.tolist() == [2 ** 64 - 1]
    tr.write_triangles(again, N, back)
    assert open(again, "rb").read() == open(path, "rb").read()
    tr.write_triangles(path, 5, r)
    good = open(path).read()
    for bad in ("", "# 1 2\n", good.replace("# 5 2", "# five 2"), good.replace("# 5 2 8", "# 5 3 8"), good.replace(" 1 2 1\n", " 1 2 2\n"),
                good.replace("\nc 1 ", "\nc 2 "), good.replace("c 0 4 3 3 5", "c 0 4 3 3"), good.replace("c 0 4 3 3 5", "c 0 4 3 3 5 1"),
                good.replace("c 0 4 3 3 5", "c 0 4 3 3 5x"), good.replace("c 0 4 3 3 5", "c 0 4 3 4 5"), good.replace("\nn 3 ", "\nn 4 "),
                good.replace("n 2 3 1 1 1", "n 2 3 1 2 1"), good.replace("n 2 3 1 1 1", "n 2 3 1 1"), good + "c 2 0 0 0 0\n",
                good + "n 5 0 0 0 0\n", good.replace("n 4 0 0 0 0", "m 4 0 0 0 0"), good.replace("n 4 0 0 0 0", "n 4 %d 0 0 0" % 2 ** 32),
                good.replace("n 4 0 0 0 0", "n 4 -1 0 0 0")):
        open(path, "w").write(bad)
        with pytest.raises(AmmsbError):
            tr.read_triangles(path)


def test_argument_errors_are_returned_before_anything_is_launched(tr):
    lib = tr.load()
    p = 0x2000   # never dereferenced: every call below is refused on its arguments, or is the no-op
    err = lib.ammsb_triangles_last_error
    names = ("mask", "offsets", "targets", "tri", "tri_in", "tri_comms", "ktri3", "kpart", "counts")

    def nodes(rows=1000, K=64, first=0, n=10, **ptrs):
        a = {name: p for name in names}
        a.update(ptrs)
        return lib.ammsb_triangles_nodes(a["mask"], rows, K, a["offsets"], a["targets"], first, n, a["tri"], a["tri_in"],
                                         a["tri_comms"], a["ktri3"], a["kpart"], a["counts"], None)

    for name in names:
        assert nodes(**{name: None}) == EINVAL and b"NULL" in err(), name
        assert nodes(**{name: None}, n=0) == EINVAL, name
    for K in (0, 8193, 2 ** 32 - 1):
        assert nodes(K=K) == EINVAL and b"num_cols" in err(), K
        assert nodes(K=K, n=0) == EINVAL and b"num_cols" in err(), K
    assert nodes(rows=2 ** 32) == EINVAL and b"2^32" in err()
    for first, n in ((991, 10), (1001, 0), (0, 1001), (2 ** 64 - 1, 2), (5, 2 ** 64 - 1)):
        assert nodes(first=first, n=n) == EINVAL and b"past num_rows" in err(), (first, n)
    for name in names:
        by = 4 if name in ("mask", "offsets", "ktri3", "kpart", "counts") else 2
        assert nodes(**{name: p + by}) == EINVAL and b"aligned" in err(), name
        assert nodes(**{name: p + by}, n=0) == EINVAL, name
        assert nodes(**{name: p + 1}) == EINVAL and b"aligned" in err(), name
    # n_rows == 0 needs no device, at either end of the range
    assert nodes(n=0) == 0 and nodes(first=1000, n=0) == 0 and nodes(rows=0, n=0) == 0 and nodes(K=8192, n=0) == 0
    assert lib.ammsb_triangles_last_kernel_name() == b""


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(tr):
    from mcmc_ammsb_gpu_amd import _capi, _connect, _modularity, _quality, _roles
    hdr = open(os.path.join(ROOT, "include", "ammsb_triangles.h")).read()
    declared = set(re.findall(r"\b(ammsb_triangles_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 3 and declared == set(tr.SIGNATURES), declared ^ set(tr.SIGNATURES)
    assert os.path.exists(tr.LIB_PATH) and os.path.basename(tr.LIB_PATH) == "libammsb_triangles.so"
    lib = C.CDLL(tr.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    own = exported_symbols(tr.LIB_PATH)
    assert own == declared, own ^ declared
    # the arguments of the one call, counted in the header's declaration
    decl = re.search(r"int ammsb_triangles_nodes\(([^;]*)\);", hdr).group(1)
    assert len(decl.split(",")) == len(tr.SIGNATURES["ammsb_triangles_nodes"][1]) == 14
    for macro, value in (("MAX_COLS", tr.MAX_COLS), ("W1_MAX_COLS", tr.W1_MAX_COLS), ("MAX_ROW", tr.MAX_ROW), ("ROW_LDS", tr.ROW_LDS)):
        assert value == int(re.search(r"#define AMMSB_TRIANGLES_%s (\d+)u" % macro, hdr).group(1)), macro
    assert (tr.MAX_COLS, tr.W1_MAX_COLS, tr.MAX_ROW) == (8192, 4096, 65535) and 64 <= tr.ROW_LDS <= tr.MAX_ROW
    src = open(os.path.join(PKG, "csrc", "ammsb_triangles.hip")).read()
    assert set(re.findall(r'"(triangles_[a-z0-9_]+)"', src)) == set(tr.KERNEL_FORMS) == {"triangles_nodes_w1", "triangles_nodes_w2"}
    for form in tr.KERNEL_FORMS:
        assert re.search(r"\b%s\b" % form, hdr), form
    assert hdr.index("Definitions (the contract)") < hdr.index("#ifndef") and "AMMSB_EINVAL" in hdr
    assert "asm" not in src   # plain HIP
    assert '#include "ammsb_postfit.h"' in src
    # a library of its own: the existing ones do not know it, it does not name them, and its kernels are gfx950 code objects
    for other in (_capi, _quality, _connect, _modularity, _roles):
        assert not [n for n in other.SIGNATURES if "triangles" in n]
        assert b"ammsb_triangles" not in open(other.LIB_PATH, "rb").read()
    for name in os.listdir(os.path.join(ROOT, "include")):
        if name.endswith(".h") and name != "ammsb_triangles.h":
            assert "ammsb_triangles" not in open(os.path.join(ROOT, "include", name)).read(), name
    for name in os.listdir(PKG):
        if name.startswith("libammsb_") and name.endswith(".so") and name not in ("libammsb_triangles.so", "libammsb_host.so"):
            assert b"ammsb_triangles" not in open(os.path.join(PKG, name), "rb").read(), name
    raw = open(tr.LIB_PATH, "rb").read()
    assert b"gfx950" in raw
    for form in tr.KERNEL_FORMS:   # as a kernel's (mangled) symbol and descriptor, not only as the dispatcher's string
        assert re.search(rb"_ZN[0-9A-Za-z_]*\d+" + form.encode() + rb"E[0-9A-Za-z_]*\.kd", raw), form
    for prefix in ("ammsb_roles", "ammsb_connect", "ammsb_modularity", "ammsb_quality", "ammsb_relate", "ammsb_readout"):
        assert prefix not in src and prefix not in hdr and prefix.encode() not in raw, prefix
    import make_dry_run as dry
    assert dry.header_rebuilds_object("triangles") and dry.csrc_all_builds("../libammsb_triangles.so", "ammsb_triangles.o")
    assert "ammsb_triangles" not in dry.hip_library_link()   # not part of libammsb_hip.so
    assert dry.host_all_builds("../triangles_test", "tests/cpp/triangles_test.cc", "-lammsb_triangles")
    for exe in ("triangles_test", "ammsb_main"):
        assert os.access(os.path.join(PKG, exe), os.X_OK), exe


def test_no_cpu_path_without_a_gpu(tr, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)   # (what a box without a device answers)
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner

    class Cfg:
        N, K = 50, 8
    lrn = object.__new__(Learner)   # a Learner cannot be built without a device either (ops.Context raises)
    lrn.cfg = Cfg()
    for call in (lambda: lrn.Triangles(), lambda: lrn.Triangles(0.01, edges=[1, 2]), lambda: lrn.Triangles(nodes=(3, 10))):
        with pytest.raises(AmmsbError, match="no CPU path"):
            call()
    # the arguments are checked on the host, before a device is asked for
    for bad in (lambda: lrn.Triangles(-1.0), lambda: lrn.Triangles(float("nan")), lambda: lrn.Triangles(nodes=(45, 6))):
        with pytest.raises(AmmsbError) as e:
            bad()
        assert "no CPU path" not in str(e.value)
    assert hasattr(ops, "Triangles")


def _main(*args):
    exe = os.environ.get("AMMSB_MAIN_EXE") or os.path.join(PKG, "ammsb_main")
    return subprocess.run([exe] + list(args), capture_output=True, text=True, timeout=60)


def test_flag_rules_end_with_status_2_before_the_graph_is_read(tr, tmp_path):
    missing = str(tmp_path / "no-such-graph.txt")     # reading it would be another failure, with another message
    out = str(tmp_path / "out.txt")
    base = ["-f", missing, "-k", "8"]
    o = ["--triangles-out", out]
    for extra in (["--triangles-threshold", "0.1"],                         # the modifier without -out
                  o + ["--triangles-threshold", "-0.1"], o + ["--triangles-threshold", "inf"],
                  o + ["--triangles-threshold", "1e39"],                    # not finite as a binary32
                  o + ["--triangles-threshold", "nan"], o + ["--triangles-threshold", "half"],
                  o + ["--triangles-threshold", "0.1x"]):
        r = _main(*(base + extra))
        assert r.returncode == 2, (extra, r.stderr[-500:])
        assert "Failed to detect file" not in r.stderr, (extra, r.stderr[-500:])
        assert "need" in r.stderr or "must be" in r.stderr or "is invalid" in r.stderr, r.stderr[-500:]
        assert not os.path.exists(out)
    # the accepted combinations get as far as the graph file
    for extra in (o, o + ["--triangles-threshold", "0"], o + ["--triangles-threshold", "0.2", "--node-roles-out", out + "2"]):
        r = _main(*(base + extra))
        assert r.returncode == 2 and "Failed to detect file" in r.stderr, (extra, r.stderr[-500:])
