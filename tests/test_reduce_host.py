"""The host side of merging and dropping communities (include/ammsb_reduce.h, _reduce.py): the numpy statement the device
tests compare against, checked here against the dense float64 definition; what must come out bit for bit; the plan and its
text form; the refusals; the built library against its header.  No test here needs a GPU.

The bound between the statement and the dense definition, per entry and relative: (n_j + 3) * 2^-24, n_j the sources of j --
n_j - 1 binary32 additions of non-negative terms, the rounding of s to binary32, one division (each at most 2^-24 relative,
the binary64 sum of s far below that), with one more for the products of the error terms."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import reduce_statement as st
from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def rd():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _reduce
    _reduce.load()
    return _reduce


def random_rows(rng, n, K):
    p = rng.random((n, K)).astype(np.float32) ** 8 + np.float32(1e-6)
    return (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def random_map(rng, K, drop):
    """groups of 1..7 sources scattered over the columns; a fraction `drop` of the columns dropped (never all)"""
    m = np.full(K, -1, np.int64)
    cols = rng.permutation(K)
    kept = cols[:max(1, int(round(K * (1 - drop))))]
    j = at = 0
    while at < kept.size:
        n = int(rng.integers(1, 8))
        m[kept[at:at + n]] = j
        at += n
        j += 1
    return m


@pytest.mark.parametrize("K", [5, 64, 65, 1024])
@pytest.mark.parametrize("drop", [0.0, 0.3])
def test_the_statement_is_the_dense_float64_definition(rd, K, drop):
    rng = np.random.default_rng(10 * K + int(10 * drop))
    pi, phi = random_rows(rng, 40, K), (rng.random(40) * 50 + 1).astype(np.float32)
    m = random_map(rng, K, drop)
    # the statement's CSR is the one the hosts hand to the device
    plan = rd.Plan(m)
    assert all(np.array_equal(x, y) for x, y in zip(st.csr(m), plan.csr())) and plan.drops == bool(drop)
    got, got_phi, emptied = st.rows(pi, phi, m)
    want, n_src = st.dense(pi, m)
    assert got.dtype == np.float32 and got.shape == want.shape and not emptied.any()
    rel = np.abs(got.astype(np.float64) - want) / want
    assert (rel <= (n_src + 3) * st.ULP24).all(), rel.max()
    if drop:
        kept_mass = pi.astype(np.float64)[:, m >= 0].sum(1)
        assert np.abs(got_phi / (phi.astype(np.float64) * kept_mass) - 1).max() <= (K + 3) * st.ULP24
        assert np.abs(got.astype(np.float64).sum(1) - 1).max() <= got.shape[1] * 2.0 ** -23
    else:
        assert got_phi.tobytes() == phi.tobytes()


@pytest.mark.parametrize("K", [1, 5, 64, 65, 1024])
def test_the_identity_and_a_permutation_come_out_bit_for_bit(K):
    rng = np.random.default_rng(K)
    pi, phi = random_rows(rng, 17, K), rng.random(17).astype(np.float32)
    pi[3, :] = 0
    pi[4, 0] = np.float32(-0.0)
    pi[5, K // 2] = np.nan
    pi[6, :] = np.float32(1e-42)      # subnormals
    th = rng.gamma(1.0, 1.0, (K, 2)).astype(np.float32)
    got, got_phi, emptied = st.rows(pi, phi, np.arange(K))
    assert got.tobytes() == pi.tobytes() and got_phi.tobytes() == phi.tobytes() and not emptied.any()
    assert st.theta(th, np.arange(K)).tobytes() == th.tobytes()
    perm = rng.permutation(K)         # map[k] = perm[k]: column k lands in perm[k]
    got, got_phi, _ = st.rows(pi, phi, perm)
    assert got[:, perm].tobytes() == pi.tobytes() and got_phi.tobytes() == phi.tobytes()
    assert st.theta(th, perm)[perm].tobytes() == th.tobytes()


def test_rows_sum_to_one_after_a_dropping_plan():
    rng = np.random.default_rng(3)
    for K in (13, 300, 4096):
        pi = random_rows(rng, 25, K)
        m = random_map(rng, K, 0.5)
        got, _, emptied = st.rows(pi, np.ones(25, np.float32), m)
        assert not emptied.any() and np.abs(got.astype(np.float64).sum(1) - 1).max() <= got.shape[1] * 2.0 ** -23


def test_a_row_whose_whole_mass_was_dropped_is_uniform_and_counted_once():
    rng = np.random.default_rng(4)
    K = 70
    pi, phi = random_rows(rng, 9, K), np.arange(1, 10, dtype=np.float32)
    m = np.arange(K) - 10            # the first ten columns are dropped (-10 .. -1 -> -1)
    m[m < 0] = -1
    pi[2, 10:] = 0                   # all its mass sits in dropped columns
    pi[5, :] = 0
    pi[7, 30] = np.nan
    got, got_phi, emptied = st.rows(pi, phi, m)
    assert emptied.tolist() == [False, False, True, False, False, True, False, True, False] and int(emptied.sum()) == 3
    assert (got[emptied] == np.float32(1.0) / np.float32(60)).all() and got_phi[emptied].tobytes() == phi[emptied].tobytes()
    assert not np.isnan(got).any() and np.abs(got[~emptied].astype(np.float64).sum(1) - 1).max() <= 60 * 2.0 ** -23
    # theta: the pseudo-counts of the dropped communities are discarded, the others copied
    th = rng.gamma(1.0, 1.0, (K, 2)).astype(np.float32)
    assert st.theta(th, m).tobytes() == th[10:].tobytes()
    m2 = np.zeros(K, np.int64)       # all into one: the left-to-right sums
    want = th[0].copy()
    for k in range(1, K):
        want = want + th[k]
    assert st.theta(th, m2).tobytes() == want.reshape(1, 2).tobytes()


def test_the_lane_sum_is_the_headers_order():
    rng = np.random.default_rng(5)
    t = (rng.random((3, 200)) ** 20).astype(np.float32)
    x = [[np.float64(0.0)] * 64 for _ in range(3)]
    for r in range(3):
        for j in range(200):
            x[r][j % 64] = x[r][j % 64] + np.float64(t[r, j])
        for d in (32, 16, 8, 4, 2, 1):
            x[r] = [x[r][v] + x[r][v ^ d] for v in range(64)]      # the butterfly: every lane ends with the same sum
        assert len(set(x[r])) == 1
    assert st.lane_sum(t).tolist() == [x[r][0] for r in range(3)]


# ---------------------------------------------------------------------------------------------------------------- Plan
def test_plan_merge_drop_compact(rd):
    P = rd.Plan
    p = P.identity(10)
    assert p.K == p.new_K == 10 and not p.drops and p.selects and p.map.tolist() == list(range(10))
    # chained pairs are one group; numbering by smallest source
    q = p.merge([(7, 3), (3, 9), (1, 2)])
    assert q.map.tolist() == [0, 1, 1, 2, 3, 4, 5, 2, 6, 2] and q.new_K == 7 and not q.selects
    assert q.sources(2).tolist() == [3, 7, 9] and q.sources(1).tolist() == [1, 2]
    assert q.merge([(9, 1)]).map.tolist() == [0, 1, 1, 1, 2, 3, 4, 1, 5, 1]        # merging merges whole groups
    assert q.merge([]) == q and p.merge([]) == p
    d = q.drop([0, 7])
    assert d.map.tolist() == [-1, 0, 0, 1, 2, 3, 4, -1, 5, 1] and d.drops and d.dropped.tolist() == [0, 7] and d.new_K == 6
    off, src = d.csr()
    assert off.dtype == src.dtype == np.uint32 and off.tolist() == [0, 2, 4, 5, 6, 7, 8] and src.tolist() == [1, 2, 3, 9, 4, 5, 6, 8]
    assert all((np.diff(src[off[j]:off[j + 1]].astype(np.int64)) > 0).all() for j in range(d.new_K))
    # compact: any numbering -> by smallest source
    c = P([3, -1, 0, 3, 1, 2, 0]).compact()
    assert c.map.tolist() == [0, -1, 1, 0, 2, 3, 1]
    assert P([2, 1, 0]).compact() == P.identity(3) and not P([2, 1, 0]) == P.identity(3)
    # drop_smaller: a group goes when its sources' sizes add up to less than min_size
    sizes = np.array([0, 1, 0, 5, 1, 0, 2, 0, 0, 9])
    s = q.drop_smaller(sizes, 2)
    assert s.dropped.tolist() == [0, 1, 2, 4, 5, 8] and s.map.tolist() == [-1, -1, -1, 0, -1, -1, 1, 0, -1, 0]
    assert p.drop_smaller(sizes, 1).dropped.tolist() == [0, 2, 5, 7, 8] and p.drop_smaller(sizes, 0) == p
    import torch
    assert p.drop_smaller(torch.from_numpy(sizes), 1) == p.drop_smaller(sizes, 1)
    assert not p.map.flags.writeable


def test_plan_refusals_name_the_offending_id(rd):
    P = rd.Plan
    for bad, word in (([0, 2, 2], "new community 1"), ([0, 5], "community 1 "), ([-2, 0], "community 0 "), ([-1, -1], "every"),
                      ([], "1..8192"), (np.zeros(8193, int), "1..8192"), ([0.5, 1.0], "integer"), ([[0, 1]], "1-D")):
        with pytest.raises(ValueError, match=word):
            P(bad)
    p = P.identity(6).drop([4])
    for call, word in ((lambda: p.merge([(1, 6)]), "community 6"), (lambda: p.merge([(-1, 2)]), "community -1"),
                       (lambda: p.merge([(1, 4)]), "community 4 is dropped"), (lambda: p.merge([1, 2, 3]), "pairs"),
                       (lambda: p.drop([9]), "community 9"), (lambda: p.drop(range(6)), "last one"),
                       (lambda: p.drop_smaller([1] * 5, 1), "5 sizes"), (lambda: p.drop_smaller([1] * 6, 2), "every community"),
                       (lambda: p.sources(5), "new community 5")):
        with pytest.raises(ValueError, match=word):
            call()


def test_the_text_form_round_trips_to_the_same_bytes(rd, tmp_path):
    p = rd.Plan.identity(12).merge([(0, 11), (11, 5), (2, 3)]).drop([7, 1])
    text = rd.plan_text(p)
    assert text == "# 12 7 2\n0 3 0 5 11\n1 2 2 3\n2 1 4\n3 1 6\n4 1 8\n5 1 9\n6 1 10\nx 1\nx 7\n"
    a, b = str(tmp_path / "a.plan"), str(tmp_path / "b.plan")
    rd.write_plan(a, p)
    q = rd.read_plan(a)
    rd.write_plan(b, q)
    assert q == p and open(a, "rb").read() == open(b, "rb").read() == text.encode()
    odd = rd.Plan([2, 0, 0, -1, 1])           # not numbered by smallest source: the file keeps the numbering
    rd.write_plan(a, odd)
    assert rd.read_plan(a) == odd and open(a).read() == "# 5 3 1\n0 2 1 2\n1 1 4\n2 1 0\nx 3\n"
    for bad in ("", "# 3 2\n", "# 3 2 0\n0 2 0 1\n", "# 3 2 0\n0 2 0 1\n1 1 1\n", "# 3 2 0\n0 2 0 1\n1 1 3\n", "# 3 2 0\n1 2 0 1\n0 1 2\n",
                "# 3 2 1\n0 1 0\n1 1 1\nx 2\nx 2\n", "# 3 1 0\n0 3 0 1\n", "# 3 2 0\n0 2 0 one\n1 1 2\n"):
        open(a, "w").write(bad)
        with pytest.raises(ValueError, match="line"):
            rd.read_plan(a)


# ---------------------------------------------------------------------------------------------------------------- library
def _rpm(rows, cols, rib, blocks, base=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for b in range(blocks):
        d.blocks[b] = base + b * 0x100000
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rib, rows, cols, blocks
    return d


def test_bad_arguments_are_refused_without_a_device(rd):
    lib = rd.load()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    pi, out = _rpm(100, 8, 40, 3), _rpm(100, 5, 50, 2, base=0x9000000)
    err = lib.ammsb_reduce_last_error

    def rows(pi=pi, phi=p, off=p, src=p, new=5, drops=0, out=out, ophi=p, emptied=p, first=0, count=4):
        return lib.ammsb_reduce_rows(C.byref(pi) if pi is not None else None, phi, off, src, new, drops,
                                     C.byref(out) if out is not None else None, ophi, emptied, first, count, None)
    assert rows(pi=None) == EINVAL and b"NULL" in err() and rows(out=None) == EINVAL
    assert rows(phi=None) == EINVAL and b"phi_sum" in err() and rows(ophi=None) == EINVAL
    assert rows(src=None) == EINVAL and b"src" in err()
    assert rows(drops=1, emptied=None) == EINVAL and b"emptied" in err()
    assert rows(emptied=p + 4, drops=1) == EINVAL and b"aligned" in err() and rows(src=p + 2) == EINVAL and rows(off=p + 1) == EINVAL
    for bad in (_rpm(100, 0, 40, 3), _rpm(100, 8193, 40, 3), _rpm(100, 8, 40, 2), _rpm(100, 8, 0, 3)):
        assert rows(pi=bad) == EINVAL
    for bad, new in ((_rpm(100, 0, 50, 2, 0x9000000), 0), (_rpm(100, 8193, 50, 2, 0x9000000), 8193), (_rpm(100, 5, 50, 1, 0x9000000), 5)):
        assert rows(out=bad, new=new) == EINVAL
    assert rows(out=_rpm(100, 9, 50, 2, 0x9000000), new=9) == EINVAL and b"more new" in err()        # K' > K
    assert rows(new=4) == EINVAL and b"new_cols" in err()
    assert rows(out=_rpm(101, 5, 50, 3, 0x9000000)) == EINVAL and b"rows" in err()
    share = _rpm(100, 5, 50, 2, base=0x9000000)
    share.blocks[1] = pi.blocks[2]
    assert rows(out=share) == EINVAL and b"share" in err()
    assert rows(first=97, count=4) == EINVAL and b"range" in err() and rows(first=101, count=0) == EINVAL
    assert rows(count=1 << 32) == EINVAL
    hole = _rpm(100, 8, 40, 3)
    hole.blocks[1] = 0
    assert rows(pi=hole) == EINVAL and b"NULL" in err()
    th = lambda *a: lib.ammsb_reduce_theta(*a, None)   # noqa: E731
    assert th(None, p, p, 8, 5, p + 64) == EINVAL and th(p, p, None, 8, 5, p + 64) == EINVAL and th(p, p, p, 8, 5, None) == EINVAL
    assert th(p, p, p, 0, 0, p + 64) == EINVAL and th(p, p, p, 8193, 5, p + 64) == EINVAL and th(p, p, p, 8, 0, p + 64) == EINVAL
    assert th(p, p, p, 5, 8, p + 64) == EINVAL and b"more new" in err()
    assert th(p, p, p, 8, 5, p) == EINVAL and b"same" in err() and th(p, p, p + 2, 8, 5, p + 64) == EINVAL
    # the valid no-op needs no device either; src_off == NULL is the select form, not an error
    assert rows(count=0) == 0 and rows(first=100, count=0) == 0 and rows(off=None, count=0) == 0


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(rd):
    hdr = open(os.path.join(ROOT, "include", "ammsb_reduce.h")).read()
    declared = set(re.findall(r"\b(ammsb_reduce_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 4 and declared == set(rd.SIGNATURES), declared ^ set(rd.SIGNATURES)
    assert os.path.exists(rd.LIB_PATH) and os.path.basename(rd.LIB_PATH) == "libammsb_reduce.so"
    assert exported_symbols(rd.LIB_PATH) == declared
    for name in ("rows", "theta"):
        decl = re.search(r"int ammsb_reduce_%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(rd.SIGNATURES["ammsb_reduce_" + name][1]), name
    assert rd.MAX_COLS == int(re.search(r"#define AMMSB_REDUCE_MAX_COLS (\d+)u", hdr).group(1))
    assert [rd.group_lanes(K) for K in (1, 4, 5, 13, 30, 64, 65, 256, 8192)] == [1, 1, 2, 4, 8, 16, 32, 64, 64]
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_reduce.hip")).read()
    assert set(re.findall(r"__global__ [^\n]*void (reduce_[a-z0-9_]+)\(", src)) == set(rd.KERNEL_FORMS)
    makefile = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "Makefile")).read()
    assert "reduce" in re.search(r"^ONE\s*=\s*(.+)$", makefile, re.M).group(1).split()
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd.learner import Learner
    assert all(hasattr(ops.ModelReducer, m) for m in ("rows", "theta", "run", "kernel_name"))
    assert hasattr(Learner, "Reduce")


def test_without_a_device_reduce_raises(rd, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = Learner.__new__(Learner)
    lrn.sharded = False
    with pytest.raises(AmmsbError, match="no HIP device"):
        lrn.Reduce(rd.Plan.identity(4))
