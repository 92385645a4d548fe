"""Host half of the reference-stream device sampler (include/ammsb_refsample.h), no GPU: rand_r jump-ahead against
libc, the unordered_set epoch table against a real std::unordered_set's bucket_count() history, the epoch procedure
(the library's host form and a plain numpy restatement) against the oracle's uset_order, the host's share of a
mini-batch (coin, u, seed) against host/sample.cc, the refused Config combinations, and the drop-in boundary of the new
library (header == exports == signature table; the existing library's yardsticks are untouched)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from postfit_support import exported_symbols

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def rs():
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _refsample
    _refsample.load()
    return _refsample


@pytest.fixture(scope="module")
def libc():
    L = C.CDLL("libc.so.6")
    L.rand_r.argtypes = [C.POINTER(C.c_uint)]
    L.rand_r.restype = C.c_int
    return L


def test_header_exports_and_signature_table_agree(rs):
    hdr = open(os.path.join(ROOT, "include", "ammsb_refsample.h")).read()
    declared = set(re.findall(r"\b(ammsb_refsample_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(rs.SIGNATURES), declared ^ set(rs.SIGNATURES)
    lib = C.CDLL(rs.LIB_PATH)
    for name in declared:
        assert hasattr(lib, name), name
    # ... and the library exports no other function of its own (kernel stubs are local: anonymous namespace)
    own = exported_symbols(rs.LIB_PATH)
    assert own == declared, own ^ declared


@pytest.mark.parametrize("seed", [0, 1, 42, 1804289383, 846930886, 0xFFFFFFFF])
def test_rand_r_jump_ahead_equals_libc(rs, libc, seed):
    """value and state at call j, by jump-ahead, equal libc's rand_r by stepping: every j up to 2000, then a stride,
    around every multiple of 2^16 up to 2 * 10^5"""
    top = 200001
    s = C.c_uint(seed)
    states, values = np.zeros(top + 1, dtype=np.uint64), np.zeros(top, dtype=np.int64)
    for j in range(top):
        states[j] = s.value
        values[j] = libc.rand_r(C.byref(s))
    states[top] = s.value
    js = set(range(0, 2000)) | set(range(2000, top, 97)) | {top - 1, top}
    for k in (1, 2, 3):
        js |= set(range(k * 65536 - 3, k * 65536 + 4))
    for j in sorted(js):
        st = rs.jump(seed, j)
        assert st == states[j], j
        if j < top:
            v, nxt = rs.rand_r(st)
            assert v == values[j] and nxt == states[j + 1], j


def _real_buckets(tmp, keys):
    so = os.path.join(tmp, "libusetb.so")
    if not os.path.exists(so):
        subprocess.check_call(["g++", "-O1", "-shared", "-fPIC", "-o", so, os.path.join(HERE, "cpp", "uset_buckets.cc")])
    L = C.CDLL(so)
    L.real_uset_bucket_history.restype = C.c_uint64
    L.real_uset_bucket_history.argtypes = [np.ctypeslib.ndpointer(np.uint64), C.c_uint64, np.ctypeslib.ndpointer(np.uint64)]
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(max(keys.size, 1), dtype=np.uint64)
    n = L.real_uset_bucket_history(keys, keys.size, out)
    return out[:n]


def _table_as_history(table, n):
    hist, start = np.zeros(n, dtype=np.uint64), 0
    for end, nb in table:
        hist[start:min(end, n)] = nb
        start = end
    assert start >= n
    return hist


def test_epoch_table_is_the_real_bucket_count_history(rs, tmp_path):
    rng = np.random.default_rng(3)
    n = 200000
    for keys in (np.arange(n, dtype=np.uint64), rng.integers(0, 2**62, n, dtype=np.uint64),
                 (np.uint64(77) << np.uint64(32)) | rng.integers(0, 10**6, n, dtype=np.uint64)):   # with duplicates
        hist = _real_buckets(str(tmp_path), keys)
        table = rs.epochs(hist.size)
        assert table[-1][0] == hist.size and all(a[0] < b[0] for a, b in zip(table, table[1:]))
        assert np.array_equal(_table_as_history(table, hist.size), hist)  # key-independent, rehash BEFORE the insert
    assert len(rs.epochs(65536)) == len(rs.epochs(65537)) == 13
    assert rs.epochs(13) == [(13, 13)] and rs.epochs(14)[0] == (13, 13) and len(rs.epochs(14)) == 2
    assert rs.epochs(0) == []


def _numpy_epoch_procedure(rs, keys):
    """the epoch procedure restated: per epoch, (list so far) ++ (new keys) ordered by (first position of the key's
    bucket, descending; own position, descending)"""
    keys = np.asarray(keys, dtype=np.uint64)
    _, idx = np.unique(keys, return_index=True)
    uniq = keys[np.sort(idx)]
    lst, start = np.zeros(0, dtype=np.uint64), 0
    for end, nb in rs.epochs(uniq.size):
        seq = np.concatenate([lst, uniq[start:end]])
        b = (seq % np.uint64(nb)).astype(np.int64)
        pos = np.arange(seq.size)
        first = np.full(nb, -1, dtype=np.int64)
        first[b[::-1]] = pos[::-1]   # the smallest position wins
        lst = seq[np.argsort(-(first[b] * seq.size + pos), kind="stable")]
        start = end
    return lst


@pytest.mark.parametrize("n", [1, 11, 12, 13, 14, 29, 30, 65536, 65537])
def test_epoch_procedure_equals_the_oracle_order(rs, orc, n):
    rng = np.random.default_rng(n)
    for keys in (rng.integers(0, max(3, 2 * n), 3 * n, dtype=np.uint64),                              # duplicates
                 (np.uint64(12345) << np.uint64(32)) | rng.integers(0, 4 * n, n + n // 2 + 2, dtype=np.uint64),
                 np.arange(n, dtype=np.uint64)):
        # exactly n unique keys where the draw allows it, so that the sizes named are the set's sizes
        _, idx = np.unique(keys, return_index=True)
        first = np.sort(idx)
        if first.size > n:
            keys = keys[:first[n]]
        want = orc.uset_order(keys)
        assert np.array_equal(rs.host_order(keys), want), "library host form"
        assert np.array_equal(_numpy_epoch_procedure(rs, keys), want), "numpy restatement"


def test_host_share_of_a_minibatch_follows_the_host_sampler(rs, libc):
    """coin, u and the link retry loop consume rand_r exactly as host/sample.cc does: for a link mini-batch the seed
    afterwards and the edge set's end point equal hostlib.Dataset.sample's"""
    from mcmc_ammsb_gpu_amd import hostlib
    N = 3000
    edges = hostlib.generate_graph(N, 8, 3.0, seed=5)   # sparse: many vertices without a training edge
    ds = hostlib.Dataset.robust(N, edges, heldout_ratio=0.02, rand_seed=3)
    off, _ = ds.training_csr()
    degree = np.ascontiguousarray(np.diff(off.astype(np.int64)), dtype=np.uint32)
    assert (degree == 0).sum() > N // 50
    lib = rs.load()
    seed, links, retried = 4242, 0, 0
    for it in range(400):
        strategy = ("Node", "NodeLink")[it % 2]
        e, v, w, after = ds.sample(64, strategy, seed)
        s, link, u = C.c_uint32(seed), C.c_uint32(0), C.c_uint32(0)
        assert lib.ammsb_refsample_choose(rs.STRATEGIES[strategy], N, degree.ctypes.data, C.byref(s), C.byref(link),
                                          C.byref(u)) == 0
        if link.value:
            links += 1
            assert w == float(N) and e.size == degree[u.value] and s.value == after
            assert all(u.value in (int(x >> np.uint64(32)), int(x & np.uint64(0xFFFFFFFF))) for x in e)
            plain = C.c_uint(seed)
            if strategy == "Node":
                libc.rand_r(C.byref(plain))
            libc.rand_r(C.byref(plain))
            retried += plain.value != after
        else:
            assert w != float(N) and e.size == 64
            assert all(u.value in (int(x >> np.uint64(32)), int(x & np.uint64(0xFFFFFFFF))) for x in e)
        seed = after
    assert links > 200 and retried > 0


def test_refused_combinations():
    from mcmc_ammsb_gpu_amd import learner
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    ok = learner.Config(device_sampling=True, sampling_stream="reference")
    assert learner._check_sampling_stream(ok) is True and ok.graph_launch == "auto"
    assert learner._check_sampling_stream(learner.Config()) is False
    assert learner.Config().sampling_stream == "own"
    assert learner._check_sampling_stream(learner.Config(sampling_stream="reference")) is False  # host sampling: no effect
    with pytest.raises(AmmsbError, match="graph_launch does not cover"):
        learner._check_sampling_stream(learner.Config(device_sampling=True, sampling_stream="reference", graph_launch=True))
    for bf in ("BF", "BFLink", "BFNonLink"):
        with pytest.raises(AmmsbError, match="device sampling implements Node / NodeLink / NodeNonLink only"):
            learner._check_sampling_stream(learner.Config(device_sampling=True, sampling_stream="reference", strategy=bf))
    with pytest.raises(AmmsbError, match="sampling_stream must be"):
        learner._check_sampling_stream(learner.Config(sampling_stream="host"))


def test_learner_refuses_before_it_allocates():
    """the same refusals through Learner(...): they come before the device context is created"""
    from mcmc_ammsb_gpu_amd import hostlib, learner
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    ds = hostlib.Dataset.robust(2000, hostlib.generate_graph(2000, 8, 8.0, seed=5), heldout_ratio=0.02, rand_seed=3)
    with pytest.raises(AmmsbError, match="graph_launch does not cover"):
        learner.Learner(learner.Config(K=32, device_sampling=True, sampling_stream="reference", graph_launch=True), ds)
    with pytest.raises(AmmsbError, match="Node / NodeLink / NodeNonLink only"):
        learner.Learner(learner.Config(K=32, device_sampling=True, sampling_stream="reference", strategy="BF"), ds)
