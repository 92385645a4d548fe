"""The host side of the chain spread (include/ammsb_spread.h, _spread.py): the lazy statement the device tests compare
against, checked here against the dense float64 variance of every sample within the bound the header derives; its mean
against average_statement's, bit for bit; the invariants (var >= 0 on adversarial inputs, a row never touched, a first flush
that reads nothing); Welford for beta; the bound; the refusals; the built library against its header.  No test here needs a
GPU.

The bound, per entry and for n <= 2^24 (the derivation is in the header): |var - dense| <= 13 F 2^-24 + F^2 2^-43, F the
flushes that wrote the row.  One flush is eps' = (1 - r) eps + r D + 3 h with h = 2^-25 and D = 2 mu + (mu + h)^2 + 7 h, mu
the mean's error (<= F 2^-22): a convex combination of the old error and D, so the mean's error enters once, not per flush."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import average_statement as avs
import spread_statement as st
from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL
F32 = np.float32


@pytest.fixture(scope="module")
def sp():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _spread
    _spread.load()
    return _spread


def random_rows(rng, n, K):
    p = rng.random((n, K)).astype(np.float32) ** 8 + np.float32(1e-6)
    return (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def random_chain(rng, N, K, steps, batch, untouched=(), always=()):
    """-> (lazy spread, lazy average, dense, pi, the rows some mini-batch held): `steps` iterations, each overwriting the
    rows of a random mini-batch that names one node twice and one id >= N; the rows `untouched` are in none, the rows
    `always` in every one"""
    pi = random_rows(rng, N, K)
    lazy, mean_only, dense = st.Lazy(N, K, 2 * K), avs.Lazy(N, K, 2 * K), st.Dense()
    free = np.setdiff1d(np.arange(N), np.concatenate([np.asarray(untouched, np.int64), np.asarray(always, np.int64)]))
    held = np.zeros(N, bool)
    for _ in range(steps):
        nodes = rng.choice(free, size=min(batch, free.size), replace=False).astype(np.uint32)
        nodes = np.concatenate([nodes, nodes[:1], np.asarray(always, np.uint32), [np.uint32(N + rng.integers(0, 5))]]).astype(np.uint32)
        rng.shuffle(nodes)
        lazy.before(pi, nodes)
        mean_only.before(pi, nodes)
        ids = st.claimed(nodes, N)
        pi[ids] = random_rows(rng, ids.size, K)
        held[ids] = True
        beta = rng.random(2 * K).astype(np.float32)
        lazy.after(beta)
        mean_only.after(beta)
        dense.after(pi, beta)
    return lazy, mean_only, dense, pi, held


CHAINS = [(1, 1, 3, 1), (7, 1, 20, 2), (40, 5, 60, 6), (64, 5, 200, 9), (33, 64, 41, 33), (48, 64, 60, 1)]


@pytest.mark.parametrize("N,K,steps,batch", CHAINS)
def test_the_lazy_variance_is_the_dense_variance_of_every_sample(N, K, steps, batch):
    rng = np.random.default_rng(1000 * N + K)
    always = (N - 1,) if N > 4 else ()
    untouched = (0, N // 2) if N > 4 else ()
    lazy, mean_only, dense, pi, held = random_chain(rng, N, K, steps, batch, untouched, always)
    assert lazy.n == steps
    never = lazy.last == 0
    assert np.isnan(lazy.var[never]).all() and not np.isnan(lazy.var[~never]).any()
    for slabs in (1, 3):
        copy = st.Lazy(N, K, 2 * K)
        copy.mean, copy.var, copy.last, copy.n, copy.flushes = (lazy.mean.copy(), lazy.var.copy(), lazy.last.copy(), lazy.n,
                                                                lazy.flushes.copy())
        mean, var = copy.read(pi, slabs)
        _, want_var, _, _ = dense.read()
        assert (copy.last == steps).all() and not np.isnan(var).any() and (var >= 0).all()
        F = copy.flushes[:, None]
        err = np.abs(var.astype(np.float64) - want_var)
        assert (F >= 1).all() and (err <= st.bound_var(F)).all(), (err.max(), st.bound_var(F.max()))
        if always:
            assert copy.flushes[N - 1] == steps          # flushed before every iteration but the first, and for the read
        # the mean beside it is the plain average's, bit for bit
        m2 = avs.Lazy(N, K, 2 * K)
        m2.mean, m2.last, m2.beta64, m2.n, m2.flushes = (mean_only.mean.copy(), mean_only.last.copy(), mean_only.beta64.copy(),
                                                         mean_only.n, mean_only.flushes.copy())
        want_mean, _ = m2.read(pi, slabs)
        assert mean.tobytes() == want_mean.tobytes() and np.array_equal(copy.last, m2.last)
        assert np.array_equal(copy.flushes, m2.flushes)
        # a second read at the same n writes nothing
        assert st.rows(pi, mean, var, copy.last, copy.n, first=0, count=N).size == 0
    assert lazy.beta64.tobytes() == mean_only.beta64.tobytes()


def test_the_bound_constrains_something():
    # values of var are at most 1/4: a bound of 1e-3 after 200 flushes still tells a spread from none
    assert st.bound_var(200) < 1e-3
    assert st.bound_var(1) >= 13 * 2.0 ** -24


def test_var_stays_non_negative_on_adversarial_inputs():
    one_below = np.nextafter(F32(1), F32(0))
    tiny = np.nextafter(F32(0), F32(1))                # the smallest subnormal
    cases = []
    for n, old in ((1 << 24, 1), (0xFFFFFFFF, 1), (3, 2), (1 << 24, (1 << 24) - 1), (2, 1), (0xFFFFFFFF, 0xFFFFFFFE)):
        for p, m in ((0.5, 0.5), (0.0, 0.0), (1.0, 1.0), (0.0, 1.0), (1.0, 0.0), (float(one_below), 1.0), (0.3, 0.30000001)):
            for v in (0.0, float(tiny), float(tiny) * 3, 2.0 ** -126, 1e-30, 0.25, float(np.nextafter(F32(0.25), F32(0)))):
                cases.append((n, old, p, m, v))
    for n, old, p, m, v in cases:
        pi, mean, var = np.array([[p]], F32), np.array([[m]], F32), np.array([[v]], F32)
        last = np.array([old], np.uint32)
        assert st.rows(pi, mean, var, last, n, nodes=np.array([0], np.uint32)).tolist() == [0]
        assert var[0, 0] >= 0, (n, old, p, m, v, var)
        assert 0 <= mean[0, 0] <= 1 and last[0] == n
        if p == m:                                     # d = 0: the variance only shrinks
            assert var[0, 0] <= F32(v)
    # r within an ulp of 1 really occurs, and d = 0 with a subnormal var ends at a non-negative subnormal or 0
    r = F32((1 << 24) - 1) / F32(1 << 24)
    assert r == one_below
    rng = np.random.default_rng(11)
    pi, mean = random_rows(rng, 300, 7), random_rows(rng, 300, 7)
    var = (rng.random((300, 7)) * 0.25).astype(F32)
    var[::3] = tiny
    mean[::5] = pi[::5]
    last = rng.integers(1, 50, 300).astype(np.uint32)
    st.rows(pi, mean, var, last, 50, first=0, count=300)
    assert (var >= 0).all() and (last == 50).all()


def test_a_row_no_mini_batch_held_has_var_zero_and_its_pi_row_as_mean():
    rng = np.random.default_rng(5)
    lazy, _, dense, pi, held = random_chain(rng, 50, 9, 40, 7, untouched=(0, 13, 49))
    assert not held[[0, 13, 49]].any() and held.sum() > 30
    mean, var = lazy.read(pi)
    assert mean[~held].tobytes() == pi[~held].tobytes()
    assert var[~held].tobytes() == np.zeros_like(var[~held]).tobytes()       # +0.0, every bit
    assert (lazy.flushes[~held] == 1).all()


def test_a_first_flush_reads_neither_buffer():
    rng = np.random.default_rng(6)
    N, K = 20, 6
    pi = random_rows(rng, N, K)
    for n in (1, 2, 77, (1 << 24) + 1, 0xFFFFFFFF):
        mean, var, last = np.full((N, K), np.nan, F32), np.full((N, K), np.nan, F32), np.zeros(N, np.uint32)
        nodes = np.array([3, 3, 19, N, 0xFFFFFFFF, 0], np.uint32)
        wrote = st.rows(pi, mean, var, last, n, nodes=nodes)
        assert sorted(wrote.tolist()) == [0, 3, 19]
        assert mean[[0, 3, 19]].tobytes() == pi[[0, 3, 19]].tobytes() and np.isnan(np.delete(mean, [0, 3, 19], 0)).all()
        assert var[[0, 3, 19]].tobytes() == bytes(3 * K * 4) and np.isnan(np.delete(var, [0, 3, 19], 0)).all()
        assert last[[0, 3, 19]].tolist() == [n] * 3 and last.sum() == 3 * n
        # the same list again at the same n: w == 0, nothing is written although NaNs are planted behind last == n
        var[3] = np.nan
        assert st.rows(pi, mean, var, last, n, nodes=nodes).size == 0 and np.isnan(var[3]).all()


def test_one_merge_is_the_nine_operations_of_the_header():
    pi = np.array([[0.25, 0.75]], F32)
    mean, var, last = np.array([[0.5, 0.5]], F32), np.array([[0.01, 0.0]], F32), np.array([2], np.uint32)
    st.rows(pi, mean, var, last, 3, nodes=np.array([0], np.uint32))
    r = F32(1) / F32(3)
    s = F32(1) - r
    for k, (p, m, v) in enumerate(((0.25, 0.5, 0.01), (0.75, 0.5, 0.0))):
        d = F32(p) - F32(m)
        e = d * d
        e = e * s
        e = e - F32(v)
        e = r * e
        assert mean[0, k] == F32(m) + r * d and var[0, k] == F32(v) + e
    # the exact merge: two samples 0.5 (var 0.01 is not theirs; the formula does not care) and one 0.25
    assert abs(float(var[0, 0]) - ((1 - 1 / 3) * 0.01 + (1 / 3) * (2 / 3) * 0.0625)) < 1e-8


@pytest.mark.parametrize("B,steps", [(2, 2), (10, 50), (128, 300)])
def test_welford_for_beta_against_the_float64_variance(B, steps):
    rng = np.random.default_rng(B)
    mean64, m2, plain = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan)
    xs = []
    for n in range(1, steps + 1):
        x = (rng.random(B) * (0.01 if n % 2 else 1.0)).astype(F32)
        xs.append(x.astype(np.float64))
        st.vector(x, mean64, m2, n)
        avs.vector(x, plain, n)
        assert mean64.tobytes() == plain.tobytes()
        if n == 1:
            assert m2.tobytes() == bytes(8 * B)
    want = np.var(np.stack(xs), axis=0)
    assert (m2 >= 0).all() and np.abs(m2 / steps - want).max() <= 1e-12 * want.max()


def test_the_bound_clamps_and_a_nan_is_never_a_member():
    rng = np.random.default_rng(9)
    mean = random_rows(rng, 40, 11)
    var = (rng.random((40, 11)) ** 4 * 0.25).astype(F32)
    zero = st.bound(mean, var, 0.0)
    assert zero.tobytes() == np.clip(mean, 0, 1).tobytes() and zero.dtype == F32
    for z in (-0.5, -2.0, -1e30):
        lower = st.bound(mean, var, z)
        assert (lower <= zero).all() and (lower >= 0).all()
    upper = st.bound(mean, var, 3.0)
    assert (upper >= zero).all() and (upper <= 1).all() and (upper == 1).any()
    assert (st.bound(mean, var, -1e30)[var > 0] == 0).all()
    # the operations: a correctly rounded square root, a product, a sum
    want = mean + F32(-2) * np.sqrt(var.astype(np.float64)).astype(F32)
    assert st.bound(mean, var, -2.0).tobytes() == np.where(want > 0, np.minimum(want, F32(1)), F32(0)).astype(F32).tobytes()
    m, v = mean.copy(), var.copy()
    m[0, 0], v[1, 1], v[2, 2] = np.nan, np.nan, -1.0
    for z in (-2.0, 0.0, 2.0):
        out = st.bound(m, v, z)
        assert out[0, 0] == 0 and out[1, 1] == 0 and out[2, 2] == 0 and not np.isnan(out).any()


def test_the_row_sum_is_the_order_of_the_reduce_statement():
    import reduce_statement as rs
    rng = np.random.default_rng(4)
    for K in (1, 5, 13, 30, 64, 65, 129, 1000):
        var = (rng.random((9, K)) ** 6 * 0.25).astype(F32)
        got = st.rowsum(var)
        assert got.dtype == np.float64 and got.tobytes() == rs.lane_sum(var).tobytes()
        assert np.abs(got - var.astype(np.float64).sum(1)).max() <= K * 2.0 ** -53


def _rpm(rows, cols, rib, blocks, base=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for b in range(blocks):
        d.blocks[b] = base + b * 0x100000
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rib, rows, cols, blocks
    return d


def test_bad_arguments_are_refused_without_a_device(sp):
    lib = sp.load()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    pi, mean, var = _rpm(100, 8, 40, 3), _rpm(100, 8, 40, 3, base=0x9000000), _rpm(100, 8, 40, 3, base=0x19000000)
    B = C.byref
    rows = lambda *a: lib.ammsb_spread_rows(*a, None)   # noqa: E731
    err = lib.ammsb_spread_last_error
    assert rows(None, B(mean), B(var), p, p, 0, 4, 1) == EINVAL and b"NULL" in err()
    assert rows(B(pi), None, B(var), p, p, 0, 4, 1) == EINVAL and rows(B(pi), B(mean), None, p, p, 0, 4, 1) == EINVAL
    assert rows(B(pi), B(mean), B(var), None, p, 0, 4, 1) == EINVAL and b"last" in err()
    assert rows(B(pi), B(mean), B(var), None, None, 0, 4, 1) == EINVAL
    assert rows(B(pi), B(mean), B(var), p + 2, p, 0, 4, 1) == EINVAL and b"aligned" in err()
    assert rows(B(pi), B(mean), B(var), p, p + 1, 0, 4, 1) == EINVAL and b"aligned" in err()
    for other in (_rpm(101, 8, 40, 3), _rpm(100, 9, 40, 3), _rpm(100, 8, 50, 2), _rpm(100, 8, 50, 3)):
        other.blocks[0] = 0x29000000
        assert rows(B(pi), B(other), B(var), p, p, 0, 4, 1) == EINVAL and b"geometry" in err()
        assert rows(B(pi), B(mean), B(other), p, p, 0, 4, 1) == EINVAL and b"geometry" in err()
    for x, y, z in ((pi, pi, var), (pi, mean, pi), (pi, mean, mean)):
        assert rows(B(x), B(y), B(z), p, p, 0, 4, 1) == EINVAL and b"share" in err()
    assert rows(B(pi), B(mean), B(var), p, p, 0, 4, 0) == EINVAL and b"n == 0" in err()       # n = 0 with a node list
    assert rows(B(pi), B(mean), B(var), p, p, 1, 4, 1) == EINVAL and b"first" in err()
    assert rows(B(pi), B(mean), B(var), p, None, 97, 4, 1) == EINVAL and b"range" in err()    # count past N
    assert rows(B(pi), B(mean), B(var), p, None, 101, 0, 1) == EINVAL
    assert rows(B(pi), B(mean), B(var), p, p, 0, 1 << 32, 1) == EINVAL
    for bad in (_rpm(100, 0, 40, 3), _rpm(100, 8193, 40, 3), _rpm(100, 8, 40, 2), _rpm(100, 8, 0, 3)):
        assert rows(B(bad), B(bad), B(bad), p, p, 0, 4, 1) == EINVAL
    hole = _rpm(100, 8, 40, 3, base=0x39000000)
    hole.blocks[1] = 0
    assert rows(B(pi), B(mean), B(hole), p, p, 0, 4, 1) == EINVAL and b"NULL" in err()

    vec = lambda *a: lib.ammsb_spread_vector(*a, None)   # noqa: E731
    q = p + 8
    assert vec(p, p, q, 4, 0) == EINVAL and b"n == 0" in err()
    assert vec(None, p, q, 4, 1) == EINVAL and vec(p, None, q, 4, 1) == EINVAL and vec(p, p, None, 4, 1) == EINVAL
    assert vec(p, p + 4, q, 4, 1) == EINVAL and vec(p, p, q + 4, 4, 1) == EINVAL and vec(p + 2, p, q, 4, 1) == EINVAL
    assert vec(p, q, q, 4, 1) == EINVAL and b"same" in err()
    assert vec(p, p, q, 1 << 32, 1) == EINVAL

    out = _rpm(100, 8, 40, 3, base=0x49000000)
    bnd = lambda *a: lib.ammsb_spread_bound(*a, None)   # noqa: E731
    assert bnd(None, B(var), B(out), -2.0, 0, 4) == EINVAL and bnd(B(mean), None, B(out), -2.0, 0, 4) == EINVAL
    assert bnd(B(mean), B(var), None, -2.0, 0, 4) == EINVAL and b"NULL" in err()
    assert bnd(B(mean), B(var), B(mean), -2.0, 0, 4) == EINVAL and b"share" in err()
    assert bnd(B(mean), B(var), B(var), -2.0, 0, 4) == EINVAL and b"share" in err()
    assert bnd(B(mean), B(var), B(_rpm(100, 9, 40, 3, base=0x49000000)), -2.0, 0, 4) == EINVAL and b"geometry" in err()
    for z in (float("nan"), float("inf"), float("-inf")):
        assert bnd(B(mean), B(var), B(out), z, 0, 4) == EINVAL and b"finite" in err()
    assert bnd(B(mean), B(var), B(out), -2.0, 97, 4) == EINVAL and b"range" in err()
    assert bnd(B(mean), B(var), B(out), -2.0, 0, 1 << 32) == EINVAL
    bad = _rpm(100, 8193, 40, 3)
    assert bnd(B(bad), B(bad), B(bad), -2.0, 0, 4) == EINVAL

    rsum = lambda *a: lib.ammsb_spread_rowsum(*a, None)   # noqa: E731
    assert rsum(None, p, 0, 4) == EINVAL and rsum(B(var), None, 0, 4) == EINVAL and b"out" in err()
    assert rsum(B(var), p + 4, 0, 4) == EINVAL and b"aligned" in err()
    assert rsum(B(var), p, 97, 4) == EINVAL and b"range" in err()
    assert rsum(B(var), p, 0, 1 << 32) == EINVAL and rsum(B(bad), p, 0, 4) == EINVAL

    # the valid no-ops need no device either
    assert rows(B(pi), B(mean), B(var), None, p, 0, 0, 1) == 0
    assert rows(B(pi), B(mean), B(var), None, None, 100, 0, 1) == 0
    assert rows(B(pi), B(mean), B(var), None, None, 0, 100, 0) == 0     # a range at n == 0: nothing has been sampled
    assert vec(None, None, None, 0, 1) == 0
    assert bnd(B(mean), B(var), B(out), -2.0, 100, 0) == 0 and rsum(B(var), None, 100, 0) == 0


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(sp):
    hdr = open(os.path.join(ROOT, "include", "ammsb_spread.h")).read()
    declared = set(re.findall(r"\b(ammsb_spread_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 6 and declared == set(sp.SIGNATURES), declared ^ set(sp.SIGNATURES)
    assert os.path.exists(sp.LIB_PATH) and os.path.basename(sp.LIB_PATH) == "libammsb_spread.so"
    assert exported_symbols(sp.LIB_PATH) == declared
    for name in ("rows", "vector", "bound", "rowsum"):
        decl = re.search(r"int ammsb_spread_%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(sp.SIGNATURES["ammsb_spread_" + name][1]), name
    assert sp.MAX_COLS == int(re.search(r"#define AMMSB_SPREAD_MAX_COLS (\d+)u", hdr).group(1))
    assert [sp.group_lanes(K) for K in (1, 4, 5, 13, 30, 64, 65, 256, 8192)] == [1, 1, 2, 4, 8, 16, 32, 64, 64]
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_spread.hip")).read()
    assert set(re.findall(r"__global__ [^\n]*void (spread_[a-z0-9_]+)\(", src)) == set(sp.KERNEL_FORMS)
    makefile = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "Makefile")).read()
    assert "spread" in re.search(r"^ONE\s*=\s*(.+)$", makefile, re.M).group(1).split()
    # the header's bound is the statement's
    assert "13 F 2^-24 + F^2 2^-43" in hdr
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd.learner import AveragedModel, BoundedModel, Learner
    from mcmc_ammsb_gpu_amd.postfit import PostFit
    assert issubclass(ops.ChainSpread, ops.ChainAverage)
    assert all(hasattr(ops.ChainSpread, m) for m in ("rows", "vector", "round", "flush", "reset", "kernel_name", "bound", "rowsum"))
    assert all(hasattr(AveragedModel, m) for m in ("has_spread", "BetaStd", "MembershipSpread", "Unsettled", "Bound"))
    assert issubclass(BoundedModel, PostFit) and not issubclass(BoundedModel, Learner)
    assert "not probabilities" in BoundedModel.__doc__.lower().replace("\n", " ")


def test_without_a_device_the_spread_raises(sp, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import AveragedModel, Learner
    lrn = Learner.__new__(Learner)
    lrn.loop, lrn.sharded, lrn._average = None, False, None
    with pytest.raises(AmmsbError, match="no HIP device"):
        lrn.StartAverage(spread=True)
    assert lrn._average is None and lrn.AverageSamples == 0


def test_an_average_without_a_spread_names_the_way_to_get_one():
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import AveragedModel

    class MeanOnly:      # what ops.ChainAverage is to a view: no var
        n = 3

    view = AveragedModel.__new__(AveragedModel)
    view._avg = MeanOnly()
    assert view.has_spread is False
    for call in (lambda: view.Bound(-2), view.BetaStd, view.MembershipSpread, view.Unsettled):
        with pytest.raises(AmmsbError, match=r"StartAverage\(spread=True\)"):
            call()
