"""Child process of test_gpu_average.py (one per group): the chain average (include/ammsb_average.h, ops.ChainAverage,
Learner.StartAverage / Averaged) against average_statement.py, which test_average_host.py checks on the CPU against the
dense float64 mean of every sample.  The library's results are asserted bit for bit (mean, last, beta's binary64 mean and
its rounding); the learner's mean against the float64 mean of the snapshots within (n + 1) * 2^-22 per entry: a row is
flushed at most once per iteration and once for the read, and a flush adds at most 2^-22 (the derivation is in
test_average_host.py)."""
import ctypes as C
import io
import sys

import numpy as np

import average_statement as st
import postfit_support as ps

F32 = np.float32
FILL_F, FILL_I = 12345.5, 0x5A5A5A5A   # what the words past a buffer hold
BLOCK = 256                            # csrc/ammsb_average.hip


def random_rows(rng, n, K):
    p = rng.random((n, K), dtype=np.float32) ** 8 + F32(1e-6)
    return (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)


class Blocks:
    """rows x K floats in blocks of `rib` rows, each block followed by GUARD words of FILL_F; `off` floats in front of every
    block (1: its base is 4 bytes past a 16-byte boundary)"""

    def __init__(self, b, rows, K, rib, fill, off=0):
        from mcmc_ammsb_gpu_amd._capi import Rpm
        self.b, self.rows, self.cols, self.rows_in_block = b, rows, K, rib
        sizes = [min(rib, rows - lo) for lo in range(0, rows, rib)]
        self.bufs = [b.ctx.empty((off + s * K + ps.GUARD,), b.torch.float32) for s in sizes]
        self.views = []
        self.desc = Rpm()
        for i, (buf, s) in enumerate(zip(self.bufs, sizes)):
            buf.fill_(FILL_F)
            v = buf[off:off + s * K].view(s, K)
            v.fill_(fill)
            self.views.append(v)
            self.desc.blocks[i] = buf.data_ptr() + 4 * off
            assert self.desc.blocks[i] % 16 == 4 * off
        self.desc.rows_in_block, self.desc.num_rows, self.desc.num_cols, self.desc.num_blocks = rib, rows, K, len(sizes)
        self.off = off

    def load(self, host):
        lo = 0
        for v in self.views:
            v.copy_(self.b.dev(host[lo:lo + v.shape[0]]))
            lo += v.shape[0]

    def host(self):
        return np.concatenate([v.cpu().numpy() for v in self.views], axis=0)

    def clone(self):
        c = Blocks(self.b, self.rows, self.cols, self.rows_in_block, 0.0, self.off)
        for s, d in zip(self.views, c.views):
            d.copy_(s)
        return c

    def guards_ok(self):
        return all(bool((buf[:self.off] == FILL_F).all()) and bool((buf[-ps.GUARD:] == FILL_F).all()) for buf in self.bufs)


class Bench:
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _average, ops
        self.b = ps.DeviceBench()
        self.av, self.lib, self.ops = _average, _average.load(), ops
        self.torch = self.b.torch

    def rows(self, pi, mean, last, n, nodes=None, first=0, count=None):
        """the library call itself; nodes: a device tensor -> the kernel form it took"""
        if nodes is not None:
            count = int(nodes.numel()) if count is None else count
        rc = self.lib.ammsb_average_rows(C.byref(pi.desc), C.byref(mean.desc), C.c_void_p(last.data_ptr()),
                                         C.c_void_p(nodes.data_ptr()) if nodes is not None else None, first, count, n,
                                         self.ops._stream())
        self.av.check(rc)
        return self.av.last_kernel_name()

    def vector(self, x, mean64, n):
        self.av.check(self.lib.ammsb_average_vector(C.c_void_p(x.data_ptr()), C.c_void_p(mean64.data_ptr()), x.numel(), n,
                                                    self.ops._stream()))

    def round(self, mean64, out32, n):
        self.av.check(self.lib.ammsb_average_round(C.c_void_p(mean64.data_ptr()), C.c_void_p(out32.data_ptr()), n,
                                                   self.ops._stream()))


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------------------ exact
N_EXACT, RIB, STEPS = 3000, 1100, 6     # blocks of 1100, 1100 and 800 rows
# every group width (13 and 30: 4 and 8 lanes), both forms, a ragged last trip at 4160; (64, 1): blocks 4 bytes off a 16-byte boundary -> 4-byte form
EXACT_CASES = [(1, 0), (5, 0), (64, 0), (65, 0), (256, 0), (1024, 0), (4096, 0), (4160, 0), (13, 0), (30, 0), (64, 1)]


def exact_sequence(bn, K, off, seed):
    """One chain over a pi the test mutates between calls -> everything the device holds at the end, as bytes-comparable
    host arrays, after every intermediate state was compared with the statement."""
    b, torch, N = bn.b, bn.torch, N_EXACT
    rng = np.random.default_rng(seed)
    hp = random_rows(rng, N, K)
    pi, mean = Blocks(b, N, K, RIB, 0.0, off), Blocks(b, N, K, RIB, float("nan"), off)
    pi.load(hp)
    last = b.guarded(N, torch.int32, FILL_I, zero=True)
    B = 2 * K
    beta64, beta32 = b.guarded(B, torch.float64, FILL_F), b.guarded(B, torch.float32, FILL_F)
    lazy = st.Lazy(N, K, B)
    vec = K % 4 == 0 and off == 0
    form = "average_rows_v4" if vec else "average_rows_s1"
    assert bn.av.group_lanes(K) == {1: 1, 5: 2, 13: 4, 30: 8, 64: 16, 65: 32}.get(K, 64)
    for step in range(STEPS):
        # a list that straddles the three blocks: rows near both seams, random rows, repeats, ids >= N
        ids = np.concatenate([np.arange(RIB - 3, RIB + 3), np.arange(2 * RIB - 2, 2 * RIB + 2), [0, N - 1],
                              rng.choice(N, 300, replace=False)]).astype(np.uint32)
        nodes = np.concatenate([ids, ids[:40], ids[5:6].repeat(7), np.array([N, N + 7, 0xFFFFFFFF], np.uint32)]).astype(np.uint32)
        rng.shuffle(nodes)
        d_nodes = b.dev(nodes)
        if lazy.n:
            assert bn.rows(pi, mean, last, lazy.n, nodes=d_nodes) == form + "<list>"
            lazy.before(hp, nodes)
            assert same_bits(mean.host(), lazy.mean) and same_bits(last[:N].cpu().numpy().view(np.uint32), lazy.last), (K, step)
            # w == 0 writes nothing: NaNs planted behind last == n survive the same list at the same n
            a = int(ids[step])
            blk, loc = divmod(a, RIB)
            keep = mean.views[blk][loc].clone()
            mean.views[blk][loc].fill_(float("nan"))
            bn.rows(pi, mean, last, lazy.n, nodes=d_nodes)
            assert bool(torch.isnan(mean.views[blk][loc]).all()), "a row with w == 0 was written"
            mean.views[blk][loc].copy_(keep)
            assert same_bits(last[:N].cpu().numpy().view(np.uint32), lazy.last)
        claimed = st.claimed(nodes, N)
        hp[claimed] = random_rows(rng, claimed.size, K)
        pi.load(hp)
        beta = rng.random(B, dtype=np.float32)
        lazy.n += 1
        st.vector(beta, lazy.beta64, lazy.n)
        bn.vector(b.dev(beta), beta64, lazy.n)
        assert same_bits(beta64[:B].cpu().numpy(), lazy.beta64), (K, step)
    # the read: three ragged slabs, and one slab over a copy of the same state
    mean1, last1 = mean.clone(), last.clone()
    want_mean, want_last = lazy.mean.copy(), lazy.last.copy()
    for lo, hi in ((0, 1000), (1000, 1001), (1001, N)):
        assert bn.rows(pi, mean, last, lazy.n, first=lo, count=hi - lo) == form + "<range>"
        st.rows(hp, want_mean, want_last, lazy.n, first=lo, count=hi - lo)
    bn.rows(pi, mean1, last1, lazy.n, first=0, count=N)
    got = mean.host()
    assert same_bits(got, want_mean) and not np.isnan(got).any() and same_bits(mean1.host(), got), K
    assert same_bits(last[:N].cpu().numpy().view(np.uint32), want_last) and (want_last == lazy.n).all()
    assert same_bits(last1.cpu().numpy(), last.cpu().numpy())
    # a second read writes nothing
    mean.views[2][5].fill_(float("nan"))
    bn.rows(pi, mean, last, lazy.n, first=0, count=N)
    assert bool(torch.isnan(mean.views[2][5]).all())
    mean.views[2][5].copy_(mean1.views[2][5])
    bn.round(beta64, beta32, B)
    assert same_bits(beta32[:B].cpu().numpy(), st.rounded(lazy.beta64))
    # the words past every buffer, and pi itself
    assert pi.guards_ok() and mean.guards_ok() and mean1.guards_ok() and same_bits(pi.host(), hp)
    assert bool((last[N:] == FILL_I).all()) and bool((beta64[B:] == FILL_F).all()) and bool((beta32[B:] == FILL_F).all())
    return got, last[:N].cpu().numpy(), beta64[:B].cpu().numpy(), beta32[:B].cpu().numpy()


def exact_group(which):
    bn = Bench()
    for i in which:
        K, off = EXACT_CASES[i]
        one = exact_sequence(bn, K, off, 100 + i)
        two = exact_sequence(bn, K, off, 100 + i)
        assert all(same_bits(x, y) for x, y in zip(one, two)), "two runs differ at K = %d" % K
        print("exact K=%d off=%d: %s, group of %d lanes" % (K, off, "average_rows_v4" if K % 4 == 0 and off == 0 else "average_rows_s1",
                                                             bn.av.group_lanes(K)), flush=True)
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ far
def far_group():
    """pi and mean: uninitialised one-block buffers of 2^19 + 64 rows at K = 8192 (17 GB each; nothing but the flushed
    rows is ever touched).  2^18 + 64 rows would reach element 2^31 and byte 2^33 only; element 2^32, which the header
    promises, starts at row 2^19, so the buffers take that size and the rows around 2^17 and 2^18 are among those flushed.  A short node list and 64-row ranges around the
    boundaries and at the end; the rows 0 .. 64, which a 32-bit element offset of the rows past 2^19 would hit, hold a
    sentinel in mean and 0 in last and must keep them."""
    bn = Bench()
    b, torch = bn.b, bn.torch
    K, N = 8192, (1 << 19) + 64
    rng = np.random.default_rng(3)
    pi, mean = b.ops.RowPartitionedMatrix(b.ctx, N, K), b.ops.RowPartitionedMatrix(b.ctx, N, K)
    last = b.ctx.zeros((N,), torch.int32)
    P, M = pi.blocks[0], mean.blocks[0]
    bounds = (1 << 17, 1 << 18, 1 << 19)
    listed = np.concatenate([np.arange(x - 2, x + 2) for x in bounds] + [[N - 1, N - 2, (1 << 19) + 1]]).astype(np.int64)
    ranges = [(x - 32, 64) for x in bounds] + [(N - 64, 64)]
    used = np.unique(np.concatenate([listed] + [np.arange(lo, lo + c) for lo, c in ranges]))
    pos = {int(a): i for i, a in enumerate(used)}
    hp = random_rows(rng, used.size, K)
    d_used = b.dev(used)
    P[d_used] = b.dev(hp)
    M[:64].fill_(7.0)
    want_mean, want_last = np.full((used.size, K), np.nan, F32), np.zeros(used.size, np.uint32)
    nodes = np.concatenate([listed, listed[:5], [N, 0xFFFFFFFF]]).astype(np.uint32)
    compact = np.array([pos.get(int(a), used.size) for a in nodes], np.uint32)   # ids >= N -> an id past the compact rows
    d_nodes = b.dev(nodes)
    for n in (1, 2, 3):
        assert bn.rows(pi, mean, last, n, nodes=d_nodes) == "average_rows_v4<list>"
        st.rows(hp, want_mean, want_last, n, nodes=compact)
        at = np.array([pos[int(a)] for a in listed])
        hp[at] = random_rows(rng, at.size, K)
        P[b.dev(listed)] = b.dev(hp[at])
    for lo, c in ranges:
        assert bn.rows(pi, mean, last, 4, first=lo, count=c) == "average_rows_v4<range>"
        st.rows(hp, want_mean, want_last, 4, first=pos[lo], count=c)
    got = M[d_used].cpu().numpy()
    assert same_bits(got, want_mean) and not np.isnan(got).any()
    assert same_bits(last[d_used].cpu().numpy().view(np.uint32), want_last) and (want_last == 4).all()
    assert bool((M[:64] == 7.0).all()) and int(last[:64].sum()) == 0 and int((last != 0).sum()) == used.size
    assert same_bits(P[d_used].cpu().numpy(), hp)
    print("far ok: %d rows up to element %d" % (used.size, N * K - 1), flush=True)


# ------------------------------------------------------------------------------------------------------------ contend
def contend_group():
    """one node listed 4096 times in one call is flushed once: exactly one fold, whatever the group width"""
    bn = Bench()
    b, torch = bn.b, bn.torch
    N = 512
    for K in (5, 64, 256, 4096):
        rng = np.random.default_rng(K)
        hp, hm = random_rows(rng, N, K), random_rows(rng, N, K)
        pi, mean = Blocks(b, N, K, N, 0.0), Blocks(b, N, K, N, 0.0)
        pi.load(hp)
        mean.load(hm)
        hl = np.full(N, 2, np.uint32)
        last = b.dev(hl)
        a = 77
        once = hm[a] + F32(3) / F32(5) * (hp[a] - hm[a])   # one fold of w = 5 - 2 samples; a second one would move it again
        nodes = np.concatenate([np.full(4096, a), [3, 9, a, 500], np.full(100, 9)]).astype(np.uint32)
        rng.shuffle(nodes)
        bn.rows(pi, mean, last, 5, nodes=b.dev(nodes))
        wrote = st.rows(hp, hm, hl, 5, nodes=nodes)
        assert sorted(wrote.tolist()) == [3, 9, 77, 500]
        assert same_bits(mean.host(), hm) and same_bits(last.cpu().numpy().view(np.uint32), hl) and mean.guards_ok()
        assert same_bits(hm[a], once) and not same_bits(hm[a], hp[a])
    print("contend ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def learner_group():
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    ps.rejects(AmmsbError, (lrn.Averaged,))
    assert lrn.AverageSamples == 0
    lrn.StartAverage()
    ps.rejects(AmmsbError, (lrn.Averaged,))                      # n == 0
    start = lrn.pi.host().copy()
    n, sum_pi, sum_beta, moved = 40, np.zeros((N, K)), np.zeros(2 * K), np.zeros(N, bool)
    for _ in range(n):
        lrn.Run(1)
        lrn.drain()
        snap = lrn.pi.host()
        sum_pi += snap
        sum_beta += lrn.beta.cpu().numpy()
        moved |= (snap != start).any(1)
    assert lrn.AverageSamples == n
    view = lrn.Averaged()
    got, now = view.pi.host(), lrn.pi.host()
    err = np.abs(got.astype(np.float64) - sum_pi / n)
    print("learner: max |mean - dense| = %.3g (bound %.3g), %d of %d rows never in a mini-batch"
          % (err.max(), (n + 1) * st.ULP22, int((~moved).sum()), N), flush=True)
    assert err.max() <= (n + 1) * st.ULP22
    assert 0 < (~moved).sum() < N and got[~moved].tobytes() == now[~moved].tobytes()
    assert np.array_equal(lrn._average.last.cpu().numpy(), np.full(N, n, np.int32))
    gb = view.beta.cpu().numpy()
    assert gb.dtype == np.float32 and np.abs(gb.astype(np.float64) - sum_beta / n).max() <= 2.0 ** -24
    # a view follows the chain: one more iteration, and the next analysis answers for 41 samples
    lrn.Run(1)
    view.Memberships(top=2)
    assert view.samples == n + 1 and lrn._average.flushed == n + 1
    err = np.abs(view.pi.host().astype(np.float64) - (sum_pi + lrn.pi.host()) / (n + 1))
    assert err.max() <= (n + 2) * st.ULP22
    # Parse() ends the average; the view of the ended average refuses
    ck = io.BytesIO()
    lrn.Serialize(ck)
    lrn.Parse(io.BytesIO(ck.getvalue()))
    assert lrn.AverageSamples == 0 and lrn._average is None
    ps.rejects(AmmsbError, (lrn.Averaged, view.drain, lambda: view.CommunitySizes(0.05)))
    lrn.close()

    # Run(20); StartAverage(); Run(20); Averaged() leaves the checkpoint a plain Run(40) leaves
    a, c = make(), make()
    a.Run(20)
    a.StartAverage()
    a.Run(20)
    assert a.Averaged().samples == 20
    c.Run(40)
    ca, cc = io.BytesIO(), io.BytesIO()
    a.Serialize(ca)
    c.Serialize(cc)
    assert [(s.n_edges, s.n_nodes) for s in a.samples] == [(s.n_edges, s.n_nodes) for s in c.samples]
    ps.same_buffers(ca.getvalue(), cc.getvalue(), "Run(20) + StartAverage + Run(20) + Averaged against Run(40)", ps.sample_buffers(a))
    assert a.HeldoutPerplexity() == c.HeldoutPerplexity()
    a.StopAverage()
    assert a.AverageSamples == 0
    a.close()
    c.close()

    # the descriptor loop and the multi-rank schedule are refused
    _, make_graph = ps.c1_learner(True)
    g = make_graph()
    assert g.loop is not None
    e = ps.rejects(AmmsbError, (g.StartAverage,))
    assert "graph_launch=False" in str(e[0])
    g.close()
    x = make(device_sampling=False, graph_launch=False, force_exchange=True, phi_replicate=0.0)
    ps.rejects(AmmsbError, (x.StartAverage,))
    x.close()
    print("learner ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ views
def views_group():
    """the analyses of Averaged() against their libraries called directly on the downloaded mean"""
    b = ps.DeviceBench()
    ops, torch = b.ops, b.torch
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(False)
    lrn = make()
    lrn.Run(10)
    lrn.StartAverage()
    lrn.Run(15)
    view = lrn.Averaged()
    mean, beta = view.pi.host(), view.beta.cpu().numpy()
    assert not np.array_equal(mean, lrn.pi.host()) and not np.array_equal(beta, lrn.beta.cpu().numpy())
    c = lrn.ctx
    pi2 = ops.RowPartitionedMatrix(c, N, K)
    pi2.load(mean)
    beta2 = c.from_numpy(beta)
    h = lambda t: t.cpu().numpy()   # noqa: E731
    ro = ops.CommunityReadout(c)
    for got, want in zip(view.Memberships(top=3, threshold=0.01), ro.top(pi2, 3, 0.01)):
        assert same_bits(h(got), h(want))
    assert same_bits(h(view.CommunitySizes(0.05)), h(ro.sizes(pi2, 0.05)))
    edges = lrn.heldoutEdges
    lp = ops.LinkPredictor(c)
    assert same_bits(h(view.LinkProbabilities(edges)), h(lp.pairs(pi2, beta2, lrn.params.epsilon, edges)))
    assert not same_bits(h(view.LinkProbabilities(edges)), h(lrn.LinkProbabilities(edges)))
    r = view.CommunityCores(0.05)
    offsets, targets = view._simple_csr(None, row_limit=False)[:2]
    state, base, M, slot_comm, indeg = ops.CommunityCores(c).run(pi2, 0.05, offsets, targets, 4 << 30)[:5]
    assert r.M == M and np.array_equal(r.core, h(state["deg"]).view(np.uint32)) and np.array_equal(r.indeg, h(indeg).view(np.uint32))
    assert np.array_equal(r.members, h(state["members"]).view(np.uint64)) and np.array_equal(r.degeneracy, h(state["degeneracy"]).view(np.uint32))
    assert np.array_equal(r.community, h(slot_comm).view(np.uint16))
    print("views: held-out AUC %.6f on the mean of %d samples, %.6f on the last draw" % (view.HeldoutAUC(), view.samples, lrn.HeldoutAUC()),
          flush=True)
    lrn.close()
    print("views ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def cpp_group():
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("average_test", d, 300)
    print("cpp ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "far": lambda a: far_group(),
    "contend": lambda a: contend_group(),
    "learner": lambda a: learner_group(),
    "views": lambda a: views_group(),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
