"""The host side of the chain average (include/ammsb_average.h, _average.py): the lazy statement the device tests compare
against, checked here against the dense float64 mean of every sample; what a row's first flush and a row that is never
flushed must equal bit for bit; the refusals; the built library against its header.  No test here needs a GPU.

The bound between the lazy mean and the dense one, per entry: F * 2^-22, F the flushes that wrote the row.  A flush is
e' = (1 - r) e + delta for the error e against the exact recurrence, and delta is at most the four roundings of the update
(the ratio, the difference, the product, the sum), each at most half an ulp of a value <= 1, 2^-25: |delta| <= 4 * 2^-24
with room to spare; 0 <= 1 - r <= 1 never grows an earlier error."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import average_statement as st
from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1  # AMMSB_EINVAL


@pytest.fixture(scope="module")
def av():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _average
    _average.load()
    return _average


def random_rows(rng, n, K):
    p = rng.random((n, K)).astype(np.float32) ** 8 + np.float32(1e-6)
    return (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


def random_chain(rng, N, K, steps, batch, untouched=()):
    """-> (lazy, dense, pi, the rows some mini-batch held): `steps` iterations, each overwriting the rows of a random
    mini-batch that names one node twice and one id >= N; the rows `untouched` are in none"""
    pi = random_rows(rng, N, K)
    beta = rng.random(2 * K).astype(np.float32)
    lazy, dense = st.Lazy(N, K, 2 * K), st.Dense(N, K, 2 * K)
    free = np.setdiff1d(np.arange(N), np.asarray(untouched, dtype=np.int64))
    held = np.zeros(N, bool)
    for _ in range(steps):
        nodes = rng.choice(free, size=min(batch, free.size), replace=False).astype(np.uint32)
        nodes = np.concatenate([nodes, nodes[:1], [np.uint32(N + rng.integers(0, 5))]]).astype(np.uint32)
        rng.shuffle(nodes)
        lazy.before(pi, nodes)
        ids = st.claimed(nodes, N)
        pi[ids] = random_rows(rng, ids.size, K)
        held[ids] = True
        beta = rng.random(2 * K).astype(np.float32)
        lazy.after(beta)
        dense.after(pi, beta)
    return lazy, dense, pi, held


@pytest.mark.parametrize("N,K,steps,batch", [(1, 1, 3, 1), (7, 3, 20, 2), (40, 5, 60, 6), (64, 17, 60, 9), (33, 16, 41, 33),
                                             (64, 4, 60, 1)])
def test_the_lazy_mean_is_the_dense_mean_of_every_sample(N, K, steps, batch):
    rng = np.random.default_rng(1000 * N + K)
    lazy, dense, pi, _ = random_chain(rng, N, K, steps, batch)
    assert lazy.n == dense.n == steps
    # the invariant before the read: flushed rows hold the mean of their first last[a] samples; nothing is NaN but the
    # rows that were never flushed
    never = lazy.last == 0
    assert np.isnan(lazy.mean[never]).all() and not np.isnan(lazy.mean[~never]).any()
    for slabs in (1, 3):
        copy = st.Lazy(N, K, 2 * K)
        copy.mean, copy.last, copy.beta64, copy.n, copy.flushes = (lazy.mean.copy(), lazy.last.copy(), lazy.beta64.copy(),
                                                                  lazy.n, lazy.flushes.copy())
        mean, beta32 = copy.read(pi, slabs)
        want_pi, want_beta = dense.read()
        assert (copy.last == steps).all() and not np.isnan(mean).any()
        F = copy.flushes[:, None]
        assert (F >= 1).all() and (np.abs(mean.astype(np.float64) - want_pi) <= F * st.ULP22).all(), \
            np.abs(mean.astype(np.float64) - want_pi).max()
        # beta: n binary64 folds, each within a few ulps of a value <= 1
        assert np.abs(copy.beta64 - want_beta).max() <= 4 * steps * 2.0 ** -53
        assert np.array_equal(beta32, copy.beta64.astype(np.float32))
        # a second read at the same n changes nothing and writes nothing
        again = mean.copy()
        assert st.rows(pi, mean, copy.last, copy.n, first=0, count=N).size == 0 and np.array_equal(again, mean)


def test_a_row_no_mini_batch_held_equals_its_pi_row_bit_for_bit():
    rng = np.random.default_rng(5)
    lazy, dense, pi, held = random_chain(rng, 50, 9, 40, 7, untouched=(0, 13, 49))
    assert not held[[0, 13, 49]].any() and held.sum() > 30
    mean, _ = lazy.read(pi)
    assert mean[~held].tobytes() == pi[~held].tobytes()
    assert (lazy.flushes[~held] == 1).all()


def test_a_first_flush_copies_pi_and_never_reads_the_mean():
    rng = np.random.default_rng(6)
    N, K = 20, 6
    pi = random_rows(rng, N, K)
    for n in (1, 2, 77, (1 << 24) + 1, 0xFFFFFFFF):
        mean, last = np.full((N, K), np.nan, np.float32), np.zeros(N, np.uint32)
        nodes = np.array([3, 3, 19, N, 0xFFFFFFFF, 0], np.uint32)
        wrote = st.rows(pi, mean, last, n, nodes=nodes)
        assert sorted(wrote.tolist()) == [0, 3, 19]
        assert mean[[0, 3, 19]].tobytes() == pi[[0, 3, 19]].tobytes() and np.isnan(np.delete(mean, [0, 3, 19], 0)).all()
        assert last[[0, 3, 19]].tolist() == [n] * 3 and last.sum() == 3 * n
        # the same list again at the same n: w == 0, nothing is written although NaNs are planted behind last == n
        mean[3] = np.nan
        assert st.rows(pi, mean, last, n, nodes=nodes).size == 0 and np.isnan(mean[3]).all()


def test_one_fold_is_the_four_operations_of_the_header():
    pi = np.array([[0.25, 0.75]], np.float32)
    mean, last = np.array([[0.5, 0.5]], np.float32), np.array([2], np.uint32)
    st.rows(pi, mean, last, 3, nodes=np.array([0], np.uint32))
    r = np.float32(1) / np.float32(3)
    want = [np.float32(0.5) + r * (np.float32(0.25) - np.float32(0.5)), np.float32(0.5) + r * (np.float32(0.75) - np.float32(0.5))]
    assert mean[0].tolist() == [float(w) for w in want] and last[0] == 3
    m64 = np.array([np.nan, np.nan])
    st.vector(np.array([0.1, 0.7], np.float32), m64, 1)
    assert m64.tolist() == [float(np.float32(0.1)), float(np.float32(0.7))]
    st.vector(np.array([0.3, 0.7], np.float32), m64, 2)
    assert m64[0] == np.float64(np.float32(0.1)) + (np.float64(np.float32(0.3)) - np.float64(np.float32(0.1))) / 2.0 and m64[1] == m64[1]
    assert st.rounded(m64).dtype == np.float32


def _rpm(av, rows, cols, rib, blocks, base=0x1000):
    from mcmc_ammsb_gpu_amd._capi import Rpm
    d = Rpm()
    for b in range(blocks):
        d.blocks[b] = base + b * 0x100000
    d.rows_in_block, d.num_rows, d.num_cols, d.num_blocks = rib, rows, cols, blocks
    return d


def test_bad_arguments_are_refused_without_a_device(av):
    lib = av.load()
    word = (C.c_uint64 * 4)()
    p = C.addressof(word)
    pi, mean = _rpm(av, 100, 8, 40, 3), _rpm(av, 100, 8, 40, 3, base=0x9000000)
    rows = lambda *a: lib.ammsb_average_rows(*a, None)   # noqa: E731
    err = lib.ammsb_average_last_error
    assert rows(None, C.byref(mean), p, p, 0, 4, 1) == EINVAL and b"NULL" in err()
    assert rows(C.byref(pi), None, p, p, 0, 4, 1) == EINVAL
    assert rows(C.byref(pi), C.byref(mean), None, p, 0, 4, 1) == EINVAL and b"last" in err()
    assert rows(C.byref(pi), C.byref(mean), None, None, 0, 4, 1) == EINVAL
    assert rows(C.byref(pi), C.byref(mean), p + 2, p, 0, 4, 1) == EINVAL and b"aligned" in err()
    for other in (_rpm(av, 101, 8, 40, 3), _rpm(av, 100, 9, 40, 3), _rpm(av, 100, 8, 50, 2), _rpm(av, 100, 8, 50, 3)):
        other.blocks[0] = 0x9000000
        assert rows(C.byref(pi), C.byref(other), p, p, 0, 4, 1) == EINVAL and b"geometry" in err()
    assert rows(C.byref(pi), C.byref(pi), p, p, 0, 4, 1) == EINVAL and b"share" in err()
    assert rows(C.byref(pi), C.byref(mean), p, p, 0, 4, 0) == EINVAL and b"n == 0" in err()       # n = 0 with a node list
    assert rows(C.byref(pi), C.byref(mean), p, p, 1, 4, 1) == EINVAL and b"first" in err()
    assert rows(C.byref(pi), C.byref(mean), p, None, 97, 4, 1) == EINVAL and b"range" in err()    # count past N
    assert rows(C.byref(pi), C.byref(mean), p, None, 101, 0, 1) == EINVAL
    assert rows(C.byref(pi), C.byref(mean), p, p, 0, 1 << 32, 1) == EINVAL
    for bad in (_rpm(av, 100, 0, 40, 3), _rpm(av, 100, 8193, 40, 3), _rpm(av, 100, 8, 40, 2), _rpm(av, 100, 8, 0, 3)):
        assert rows(C.byref(bad), C.byref(bad), p, p, 0, 4, 1) == EINVAL
    hole = _rpm(av, 100, 8, 40, 3)
    hole.blocks[1] = 0
    assert rows(C.byref(hole), C.byref(mean), p, p, 0, 4, 1) == EINVAL and b"NULL" in err()
    vec = lambda *a: lib.ammsb_average_vector(*a, None)   # noqa: E731
    assert vec(p, p, 4, 0) == EINVAL and b"n == 0" in err()
    assert vec(None, p, 4, 1) == EINVAL and vec(p, None, 4, 1) == EINVAL and vec(p, p + 4, 4, 1) == EINVAL
    assert vec(p, p, 1 << 32, 1) == EINVAL
    rnd = lambda *a: lib.ammsb_average_round(*a, None)   # noqa: E731
    assert rnd(None, p, 4) == EINVAL and rnd(p, None, 4) == EINVAL and rnd(p + 4, p, 4) == EINVAL and rnd(p, p + 2, 4) == EINVAL
    # the valid no-ops need no device either
    assert rows(C.byref(pi), C.byref(mean), None, p, 0, 0, 1) == 0
    assert rows(C.byref(pi), C.byref(mean), None, None, 100, 0, 1) == 0
    assert rows(C.byref(pi), C.byref(mean), None, None, 0, 100, 0) == 0     # a range at n == 0: nothing has been sampled
    assert vec(None, None, 0, 1) == 0 and rnd(None, None, 0) == 0


def test_the_library_is_built_by_build_and_exports_what_its_header_declares(av):
    hdr = open(os.path.join(ROOT, "include", "ammsb_average.h")).read()
    declared = set(re.findall(r"\b(ammsb_average_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) == 5 and declared == set(av.SIGNATURES), declared ^ set(av.SIGNATURES)
    assert os.path.exists(av.LIB_PATH) and os.path.basename(av.LIB_PATH) == "libammsb_average.so"
    assert exported_symbols(av.LIB_PATH) == declared
    for name in ("rows", "vector", "round"):
        decl = re.search(r"int ammsb_average_%s\(([^;]*)\);" % name, hdr).group(1)
        assert len(decl.split(",")) == len(av.SIGNATURES["ammsb_average_" + name][1]), name
    assert av.MAX_COLS == int(re.search(r"#define AMMSB_AVERAGE_MAX_COLS (\d+)u", hdr).group(1))
    assert [av.group_lanes(K) for K in (1, 4, 5, 13, 30, 64, 65, 256, 8192)] == [1, 1, 2, 4, 8, 16, 32, 64, 64]
    src = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "ammsb_average.hip")).read()
    assert set(re.findall(r"__global__ [^\n]*void (average_[a-z0-9_]+)\(", src)) == set(av.KERNEL_FORMS)
    makefile = open(os.path.join(ROOT, "mcmc-ammsb-gpu_amd", "csrc", "Makefile")).read()
    assert "average" in re.search(r"^ONE\s*=\s*(.+)$", makefile, re.M).group(1).split()
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd.learner import AveragedModel, Learner
    from mcmc_ammsb_gpu_amd.postfit import PostFit
    assert all(hasattr(ops.ChainAverage, m) for m in ("rows", "vector", "round", "flush", "reset", "kernel_name"))
    assert all(hasattr(Learner, m) for m in ("StartAverage", "StopAverage", "AverageSamples", "Averaged"))
    assert issubclass(AveragedModel, PostFit) and not issubclass(AveragedModel, Learner)


def test_without_a_device_the_average_raises(av, monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd.learner import Learner
    lrn = Learner.__new__(Learner)
    lrn.loop, lrn.sharded, lrn._average = None, False, None
    with pytest.raises(AmmsbError, match="no HIP device"):
        lrn.StartAverage()
    with pytest.raises(AmmsbError, match="no sample"):
        lrn.Averaged()
    assert lrn.AverageSamples == 0
