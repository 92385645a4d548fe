"""Child process of test_gpu_spread.py (one per group): the chain spread (include/ammsb_spread.h, ops.ChainSpread,
Learner.StartAverage(spread=True), AveragedModel.Bound) against spread_statement.py, which test_spread_host.py checks on
the CPU against the dense float64 variance of every sample.  The library's results are asserted bit for bit (mean, var, last,
the bound, the row sums, beta's moments); the learner's variance against the float64 variance of the recorded samples within
the header's bound at F = n + 1: a row is flushed at most once per iteration and once for the read."""
import ctypes as C
import io
import os
import sys

import numpy as np

import average_child as ac
import postfit_support as ps
import spread_statement as st
from average_child import Blocks, random_rows, same_bits

F32 = np.float32
FILL_F, FILL_I = ac.FILL_F, ac.FILL_I
ZS = (-2.0, 0.0, 1.5)


class Bench:
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _average, _spread, ops
        self.b = ps.DeviceBench()
        self.sp, self.lib, self.ops = _spread, _spread.load(), ops
        self.av, self.avlib = _average, _average.load()
        self.torch = self.b.torch

    def rows(self, pi, mean, var, last, n, nodes=None, first=0, count=None):
        """the library call itself; nodes: a device tensor -> the kernel form it took"""
        if nodes is not None:
            count = int(nodes.numel()) if count is None else count
        rc = self.lib.ammsb_spread_rows(C.byref(pi.desc), C.byref(mean.desc), C.byref(var.desc), C.c_void_p(last.data_ptr()),
                                        C.c_void_p(nodes.data_ptr()) if nodes is not None else None, first, count, n,
                                        self.ops._stream())
        self.sp.check(rc)
        return self.sp.last_kernel_name()

    def mean_rows(self, pi, mean, last, n, nodes=None, first=0, count=None):
        """ammsb_average_rows over the same arguments: what the mean must equal"""
        if nodes is not None:
            count = int(nodes.numel()) if count is None else count
        self.av.check(self.avlib.ammsb_average_rows(C.byref(pi.desc), C.byref(mean.desc), C.c_void_p(last.data_ptr()),
                                                    C.c_void_p(nodes.data_ptr()) if nodes is not None else None, first, count, n,
                                                    self.ops._stream()))

    def vector(self, x, mean64, m2, n):
        self.sp.check(self.lib.ammsb_spread_vector(C.c_void_p(x.data_ptr()), C.c_void_p(mean64.data_ptr()),
                                                   C.c_void_p(m2.data_ptr()), x.numel(), n, self.ops._stream()))

    def bound(self, mean, var, out, z, first, count):
        self.sp.check(self.lib.ammsb_spread_bound(C.byref(mean.desc), C.byref(var.desc), C.byref(out.desc), z, first, count,
                                                  self.ops._stream()))
        return self.sp.last_kernel_name()

    def rowsum(self, var, out, first, count):
        self.sp.check(self.lib.ammsb_spread_rowsum(C.byref(var.desc), C.c_void_p(out.data_ptr()), first, count, self.ops._stream()))
        return self.sp.last_kernel_name()


# ------------------------------------------------------------------------------------------------------------ exact
N_EXACT, RIB, STEPS = 3000, 1100, 12     # blocks of 1100, 1100 and 800 rows; ~12 rounds of list and range calls mixed
# every group width, both forms, a ragged last trip at 4160; (64, 1) and (1024, 1): blocks 4 bytes off -> the 4-byte form
EXACT_CASES = [(1, 0), (5, 0), (13, 0), (30, 0), (64, 0), (65, 0), (256, 0), (1024, 0), (4096, 0), (4160, 0), (8192, 0),
               (64, 1), (1024, 1)]


def exact_sequence(bn, K, off, seed):
    b, torch, N = bn.b, bn.torch, N_EXACT
    rng = np.random.default_rng(seed)
    hp = random_rows(rng, N, K)
    pi = Blocks(b, N, K, RIB, 0.0, off)
    mean, var = Blocks(b, N, K, RIB, float("nan"), off), Blocks(b, N, K, RIB, float("nan"), off)
    plain = Blocks(b, N, K, RIB, float("nan"), off)          # ammsb_average_rows over the same calls
    pi.load(hp)
    last = b.guarded(N, torch.int32, FILL_I, zero=True)
    plain_last = b.guarded(N, torch.int32, FILL_I, zero=True)
    B = 2 * K
    beta64, m2 = b.guarded(B, torch.float64, FILL_F), b.guarded(B, torch.float64, FILL_F)
    lazy = st.Lazy(N, K, B)
    vec = K % 4 == 0 and off == 0
    form = "spread_rows_v4" if vec else "spread_rows_s1"

    def check(what):
        assert same_bits(mean.host(), lazy.mean) and same_bits(var.host(), lazy.var), (K, off, what)
        assert same_bits(last[:N].cpu().numpy().view(np.uint32), lazy.last), (K, off, what)

    for step in range(STEPS):
        ids = np.concatenate([np.arange(RIB - 3, RIB + 3), np.arange(2 * RIB - 2, 2 * RIB + 2), [0, N - 1],
                              rng.choice(N, 300, replace=False)]).astype(np.uint32)
        nodes = np.concatenate([ids, ids[:40], ids[5:6].repeat(7), np.array([N, N + 7, 0xFFFFFFFF], np.uint32)]).astype(np.uint32)
        rng.shuffle(nodes)
        d_nodes = b.dev(nodes)
        if lazy.n:
            if step % 4 == 3:
                # a range call in the middle of the chain: a slab that straddles a seam is brought to n, then the list
                lo, cnt = RIB - 50 + step, 137
                assert bn.rows(pi, mean, var, last, lazy.n, first=lo, count=cnt) == form + "<range>"
                bn.mean_rows(pi, plain, plain_last, lazy.n, first=lo, count=cnt)
                lazy.flushes[st.rows(hp, lazy.mean, lazy.var, lazy.last, lazy.n, first=lo, count=cnt)] += 1
                check("range %d" % step)
            assert bn.rows(pi, mean, var, last, lazy.n, nodes=d_nodes) == form + "<list>"
            bn.mean_rows(pi, plain, plain_last, lazy.n, nodes=d_nodes)
            lazy.before(hp, nodes)
            check("list %d" % step)
            # w == 0 writes nothing: NaNs planted behind last == n survive the same list at the same n
            a = int(ids[step])
            blk, loc = divmod(a, RIB)
            keep = var.views[blk][loc].clone()
            var.views[blk][loc].fill_(float("nan"))
            bn.rows(pi, mean, var, last, lazy.n, nodes=d_nodes)
            assert bool(torch.isnan(var.views[blk][loc]).all()), "a row with w == 0 was written"
            var.views[blk][loc].copy_(keep)
        claimed = st.claimed(nodes, N)
        hp[claimed] = random_rows(rng, claimed.size, K)
        pi.load(hp)
        beta = rng.random(B, dtype=np.float32)
        lazy.n += 1
        st.vector(beta, lazy.beta64, lazy.m2, lazy.n)
        bn.vector(b.dev(beta), beta64, m2, lazy.n)
        assert same_bits(beta64[:B].cpu().numpy(), lazy.beta64) and same_bits(m2[:B].cpu().numpy(), lazy.m2), (K, step)
    # the read: three ragged slabs
    for lo, hi in ((0, 1000), (1000, 1001), (1001, N)):
        assert bn.rows(pi, mean, var, last, lazy.n, first=lo, count=hi - lo) == form + "<range>"
        bn.mean_rows(pi, plain, plain_last, lazy.n, first=lo, count=hi - lo)
    lazy.read(hp, 1)
    check("read")
    got_mean, got_var = mean.host(), var.host()
    assert not np.isnan(got_var).any() and (got_var >= 0).all() and (lazy.last == lazy.n).all()
    assert same_bits(plain.host(), got_mean), "the mean is not ammsb_average_rows' (K = %d)" % K
    # the bound at three z and the row sums, over ragged slabs
    out = Blocks(b, N, K, RIB, float("nan"), off)
    bform = "spread_bound_v4" if vec else "spread_bound_s1"
    for z in ZS:
        for lo, hi in ((0, 1099), (1099, 2201), (2201, N)):
            assert bn.bound(mean, var, out, z, lo, hi - lo) == bform
        assert same_bits(out.host(), st.bound(got_mean, got_var, z)), (K, off, z)
    sums = b.guarded(N, torch.float64, FILL_F)
    for lo, hi in ((0, 7), (7, 2200), (2200, N)):
        sl = sums[lo:]
        assert bn.rowsum(var, sl, lo, hi - lo) == "spread_rowsum"
    got_sums = sums[:N].cpu().numpy()
    assert same_bits(got_sums, st.rowsum(got_var)), (K, off)
    # the words past every buffer, and the inputs
    assert all(x.guards_ok() for x in (pi, mean, var, out)) and same_bits(pi.host(), hp)
    assert bool((last[N:] == FILL_I).all()) and bool((sums[N:] == FILL_F).all())
    assert bool((beta64[B:] == FILL_F).all()) and bool((m2[B:] == FILL_F).all())
    assert same_bits(mean.host(), got_mean) and same_bits(var.host(), got_var)     # bound and rowsum wrote neither
    return got_mean, got_var, got_sums, m2[:B].cpu().numpy()


def exact_group(which):
    bn = Bench()
    for i in which:
        K, off = EXACT_CASES[i]
        one = exact_sequence(bn, K, off, 100 + i)
        if K <= 1024:
            # (equality with the statement after every call says it already; the second run is kept where it is cheap, and
            # above K = 1024 the time goes to the twelve rounds instead)
            two = exact_sequence(bn, K, off, 100 + i)
            assert all(same_bits(x, y) for x, y in zip(one, two)), "two runs differ at K = %d" % K
        print("exact K=%d off=%d: %s, group of %d lanes" % (K, off, "spread_rows_v4" if K % 4 == 0 and off == 0 else "spread_rows_s1",
                                                             bn.sp.group_lanes(K)), flush=True)
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ far
def far_group():
    """pi, mean and var: uninitialised one-block buffers of 2^19 + 64 rows at K = 8192 (17 GB each; nothing but the flushed
    rows is ever touched), as test_gpu_average.py's far case builds them: rows around byte 2^32 (row 2^17), element 2^31
    (row 2^18) and element 2^32 (row 2^19) of a block, by a node list and by 64-row ranges.  The rows 0 .. 64, which a
    32-bit element offset of the rows past 2^19 would hit, hold a sentinel and must keep it.  Then the bound into the
    freed pi block's successor and the row sums over the same ranges."""
    bn = Bench()
    b, torch = bn.b, bn.torch
    K, N = 8192, (1 << 19) + 64
    rng = np.random.default_rng(3)
    RPM = b.ops.RowPartitionedMatrix
    pi, mean, var = RPM(b.ctx, N, K), RPM(b.ctx, N, K), RPM(b.ctx, N, K)
    last = b.ctx.zeros((N,), torch.int32)
    P, M, V = pi.blocks[0], mean.blocks[0], var.blocks[0]
    bounds = (1 << 17, 1 << 18, 1 << 19)
    listed = np.concatenate([np.arange(x - 2, x + 2) for x in bounds] + [[N - 1, N - 2, (1 << 19) + 1]]).astype(np.int64)
    ranges = [(x - 32, 64) for x in bounds] + [(N - 64, 64)]
    used = np.unique(np.concatenate([listed] + [np.arange(lo, lo + c) for lo, c in ranges]))
    pos = {int(a): i for i, a in enumerate(used)}
    hp = random_rows(rng, used.size, K)
    d_used = b.dev(used)
    P[d_used] = b.dev(hp)
    M[:64].fill_(7.0)
    V[:64].fill_(9.0)
    want_mean, want_var = np.full((used.size, K), np.nan, F32), np.full((used.size, K), np.nan, F32)
    want_last = np.zeros(used.size, np.uint32)
    nodes = np.concatenate([listed, listed[:5], [N, 0xFFFFFFFF]]).astype(np.uint32)
    compact = np.array([pos.get(int(a), used.size) for a in nodes], np.uint32)   # ids >= N -> an id past the compact rows
    d_nodes = b.dev(nodes)
    for n in (1, 2, 3):
        assert bn.rows(pi, mean, var, last, n, nodes=d_nodes) == "spread_rows_v4<list>"
        st.rows(hp, want_mean, want_var, want_last, n, nodes=compact)
        at = np.array([pos[int(a)] for a in listed])
        hp[at] = random_rows(rng, at.size, K)
        P[b.dev(listed)] = b.dev(hp[at])
    for lo, c in ranges:
        assert bn.rows(pi, mean, var, last, 4, first=lo, count=c) == "spread_rows_v4<range>"
        st.rows(hp, want_mean, want_var, want_last, 4, first=pos[lo], count=c)
    got_mean, got_var = M[d_used].cpu().numpy(), V[d_used].cpu().numpy()
    assert same_bits(got_mean, want_mean) and same_bits(got_var, want_var) and not np.isnan(got_var).any()
    assert (got_var[[pos[int(a)] for a in listed]] > 0).any()
    assert same_bits(last[d_used].cpu().numpy().view(np.uint32), want_last) and (want_last == 4).all()
    assert bool((M[:64] == 7.0).all()) and bool((V[:64] == 9.0).all())
    assert int(last[:64].sum()) == 0 and int((last != 0).sum()) == used.size
    assert same_bits(P[d_used].cpu().numpy(), hp)
    # the row sums of the same ranges; the rows 0 .. 64 would give 8192 * 9
    for lo, c in ranges:
        sums = b.guarded(c, torch.float64, FILL_F)
        assert bn.rowsum(var, sums, lo, c) == "spread_rowsum"
        assert same_bits(sums[:c].cpu().numpy(), st.rowsum(want_var[pos[lo]:pos[lo] + c])) and bool((sums[c:] == FILL_F).all())
    # the bound: pi's block is given back first, so that three blocks are alive at most
    del pi, P
    b.release()
    out = RPM(b.ctx, N, K)
    O = out.blocks[0]
    O[:64].fill_(5.0)
    for lo, c in ranges:
        assert bn.bound(mean, var, out, -2.0, lo, c) == "spread_bound_v4"
    for lo, c in ranges:
        got = O[lo:lo + c].cpu().numpy()
        assert same_bits(got, st.bound(want_mean[pos[lo]:pos[lo] + c], want_var[pos[lo]:pos[lo] + c], -2.0)), lo
    assert bool((O[:64] == 5.0).all()) and bool((M[:64] == 7.0).all()) and bool((V[:64] == 9.0).all())
    print("far ok: %d rows up to element %d" % (used.size, N * K - 1), flush=True)


# ------------------------------------------------------------------------------------------------------------ contend
def contend_group():
    """one node listed 4096 times in one call is flushed once: mean and variance move once, whatever the group width"""
    bn = Bench()
    b = bn.b
    N = 512
    for K in (5, 64, 256, 4096):
        rng = np.random.default_rng(K)
        hp, hm = random_rows(rng, N, K), random_rows(rng, N, K)
        hv = (rng.random((N, K), dtype=np.float32) * F32(0.1)).astype(F32)
        pi, mean, var = Blocks(b, N, K, N, 0.0), Blocks(b, N, K, N, 0.0), Blocks(b, N, K, N, 0.0)
        pi.load(hp)
        mean.load(hm)
        var.load(hv)
        hl = np.full(N, 2, np.uint32)
        last = b.dev(hl)
        a = 77
        one_m, one_v, one_l = hm[a:a + 1].copy(), hv[a:a + 1].copy(), hl[a:a + 1].copy()
        st.rows(hp[a:a + 1], one_m, one_v, one_l, 5, first=0, count=1)      # one merge of w = 5 - 2 samples
        twice_m, twice_v = one_m.copy(), one_v.copy()
        st.rows(hp[a:a + 1], twice_m, twice_v, np.full(1, 2, np.uint32), 5, first=0, count=1)   # what a second one would leave
        nodes = np.concatenate([np.full(4096, a), [3, 9, a, 500], np.full(100, 9)]).astype(np.uint32)
        rng.shuffle(nodes)
        bn.rows(pi, mean, var, last, 5, nodes=b.dev(nodes))
        wrote = st.rows(hp, hm, hv, hl, 5, nodes=nodes)
        assert sorted(wrote.tolist()) == [3, 9, 77, 500]
        assert same_bits(mean.host(), hm) and same_bits(var.host(), hv) and same_bits(last.cpu().numpy().view(np.uint32), hl)
        assert mean.guards_ok() and var.guards_ok()
        assert same_bits(hv[a], one_v[0]) and same_bits(hm[a], one_m[0]) and not same_bits(one_v, twice_v)
    print("contend ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def small_learner(N=2000, K=64, m=128, n=16):
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd.learner import Config, Learner
    ds = hostlib.Dataset.robust(N, hostlib.generate_graph(N, 16, 16, seed=20260101), heldout_ratio=0.01, rand_seed=1)

    def make():
        return Learner(Config.from_cli_defaults(K=K, mini_batch_size=m, num_node_sample=n, strategy="Node",
                                                device_sampling=False, graph_launch=False), ds)
    return ds, make


def replay_samples(pis, betas):
    """every sample of a chain, float32 (pi [N, K], beta [2K]) in order -> the st.Lazy a loop leaves that flushes, before
    each iteration, the rows that iteration rewrote (those whose bits changed), and every row for the read"""
    N, K = pis[0].shape
    lazy = st.Lazy(N, K, betas[0].size)
    prev = None
    for pi, beta in zip(pis, betas):
        assert pi.dtype == F32 and beta.dtype == F32
        if prev is not None:
            changed = np.flatnonzero((pi.view(np.uint32) != prev.view(np.uint32)).any(1)).astype(np.uint32)
            assert 0 < changed.size < N
            lazy.before(prev, changed)
        lazy.after(np.ascontiguousarray(beta))
        prev = pi
    lazy.read(np.ascontiguousarray(prev))
    return lazy


def learner_group():
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K, n = 2000, 64, 30
    ds, make = small_learner(N, K)
    lrn, twin = make(), make()
    lrn.Run(10)
    twin.Run(10)
    lrn.StartAverage(spread=True)
    twin.StartAverage()
    assert type(lrn._average).__name__ == "ChainSpread" and type(twin._average).__name__ == "ChainAverage"
    pis, betas = [], []
    for _ in range(n):
        lrn.Run(1)
        lrn.drain()
        pis.append(lrn.pi.host())
        betas.append(lrn.beta.cpu().numpy())
    twin.Run(n)
    replay = replay_samples(pis, betas)
    pis, betas = np.stack(pis).astype(np.float64), np.stack(betas).astype(np.float64)
    avg = lrn.Averaged()
    assert avg.has_spread and avg.samples == n and not twin.Averaged().has_spread
    sp = lrn._average
    var, mean = sp.var.host(), avg.pi.host()
    # the chain replayed through the statement: the learner's moments are its bits.  tests/cpp/spread_test.cc's two loops
    # are held to the same replay (cpp_group), which is where the two hosts meet
    assert same_bits(mean, replay.mean) and same_bits(var, replay.var), "the learner's moments are not the statement's"
    assert same_bits(sp.beta64.cpu().numpy(), replay.beta64) and same_bits(sp.beta_m2.cpu().numpy(), replay.m2)
    want = pis.var(0)
    err = np.abs(var.astype(np.float64) - want)
    bound = float(st.bound_var(n + 1))
    moved = (pis != pis[0]).any(0).any(1)
    print("learner: max |var - dense| = %.3g (bound %.3g), largest var %.3g, %d of %d rows never in a mini-batch"
          % (err.max(), bound, var.max(), int((~moved).sum()), N), flush=True)
    assert err.max() <= bound and (var >= 0).all()
    assert want.max() > 2 * bound            # (the chain does move: the bound tells its largest spread from none)
    assert 0 < (~moved).sum() < N and not var[~moved].any()
    # the mean is the plain average's of the same seed, bit for bit; so is beta's
    tw = twin.Averaged()
    assert same_bits(mean, tw.pi.host()) and same_bits(avg.beta.cpu().numpy(), tw.beta.cpu().numpy())
    assert same_bits(sp.beta64.cpu().numpy(), twin._average.beta64.cpu().numpy())
    # BetaStd
    got = avg.BetaStd()
    assert got.dtype == np.float64 and got.shape == (2 * K,) and np.abs(got - betas.std(0)).max() <= 1e-9
    # MembershipSpread gathers var at Memberships' ids
    h = lambda t: t.cpu().numpy()   # noqa: E731
    thr = float(np.median(np.sort(mean, 1)[:, -2]))     # about half the rows have one membership at most: empty slots
    for nodes in (None, np.array([5, 1999, 0, 5, 77], np.uint32)):
        ids, m, sd = (h(t) for t in avg.MembershipSpread(top=3, threshold=thr, nodes=nodes))
        wi, wm, _ = (h(t) for t in avg.Memberships(3, thr, nodes))
        assert same_bits(ids, wi) and same_bits(m, wm) and sd.dtype == np.float32 and sd.shape == ids.shape
        rows = np.arange(N) if nodes is None else nodes.astype(np.int64)
        want_sd = np.where(ids >= 0, np.sqrt(var[rows[:, None], np.maximum(ids, 0)]), F32(0)).astype(F32)
        print("MembershipSpread %s: %d slots, %d empty, %d with sd > 0, %d differ" % (
            "all" if nodes is None else "list", ids.size, int((ids < 0).sum()), int((sd > 0).sum()),
            int((sd.view(np.uint32) != want_sd.view(np.uint32)).sum())), flush=True)
        assert same_bits(sd, want_sd)
        if nodes is None:
            assert (ids < 0).any() and (sd > 0).any()
    # Unsettled: a stable argsort of the float64 row sums
    total = st.rowsum(var)
    assert same_bits(h(sp.rowsum()), total)
    who, how = avg.Unsettled(top=25)
    order = np.argsort(-total, kind="stable")[:25]
    assert who.dtype == np.int64 and np.array_equal(who, order) and same_bits(how, total[order]) and (np.diff(how) <= 0).all()
    assert avg.Unsettled(top=N + 5)[0].size == N
    # a restart with the other `spread` replaces the object; the same one only resets
    keep = lrn._average
    lrn.StartAverage(spread=True)
    assert lrn._average is keep and lrn.AverageSamples == 0
    lrn.StartAverage()
    assert type(lrn._average).__name__ == "ChainAverage" and lrn._average is not keep
    ps.rejects(AmmsbError, (avg.drain, avg.BetaStd))          # the old view's average is gone
    lrn.close()
    twin.close()

    # Run(20); StartAverage(spread=True); Run(20); Averaged() leaves the checkpoint a plain Run(40) leaves
    a, c = make(), make()
    a.Run(20)
    a.StartAverage(spread=True)
    a.Run(20)
    view = a.Averaged()
    assert view.samples == 20 and view.Bound(-2).CommunitySizes(0.05).numel() == K
    c.Run(40)
    ca, cc = io.BytesIO(), io.BytesIO()
    a.Serialize(ca)
    c.Serialize(cc)
    assert [(s.n_edges, s.n_nodes) for s in a.samples] == [(s.n_edges, s.n_nodes) for s in c.samples]
    ps.same_buffers(ca.getvalue(), cc.getvalue(), "Run(20) + StartAverage(spread=True) + Run(20) + Averaged against Run(40)",
                    ps.sample_buffers(a))
    assert a.HeldoutPerplexity() == c.HeldoutPerplexity()
    a.close()
    c.close()
    print("learner ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ views
N_INTEGERS = 21    # CommunitySizes, 4 of CommunityQuality, 3 of RelatedCommunities, 13 of NodeRoles


def _integers(view, thr):
    """the integers of four analyses of a PostFit view, as host arrays"""
    h = lambda t: t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)   # noqa: E731
    q = view.CommunityQuality(thr)
    rel = view.RelatedCommunities(thr, top=3)
    roles = view.NodeRoles(thr, top=2)
    out = [h(view.CommunitySizes(thr)), q.size, q.internal, q.boundary, np.array([q.uncovered])]
    out += [rel.size, rel.partner, rel.overlap]                       # (a field that is gone is an AttributeError here)
    out += [roles.degree, roles.own, roles.embedded, roles.reached, roles.votes, roles.squares, roles.home, roles.hcount,
            roles.hflags, roles.ksum, roles.ksq, roles.kmembers, np.array([roles.valid, roles.skipped])]
    assert len(out) == N_INTEGERS and all(isinstance(x, np.ndarray) and x.dtype.kind in "iu" for x in out)
    return out


class Plain:
    """a PostFit over a matrix of the test's own: the numpy statement of the bound, uploaded"""

    def __new__(cls, like, host_pi):
        from mcmc_ammsb_gpu_amd.postfit import PostFit

        class _View(PostFit):
            def drain(self):
                pass
        v = _View()
        for f in ("ops", "ctx", "cfg", "params", "dataset", "trainingSet", "heldoutSet", "heldoutEdges", "beta"):
            setattr(v, f, getattr(like, f))
        v.pi = like.ops.RowPartitionedMatrix(like.ctx, host_pi.shape[0], host_pi.shape[1], like.pi.rows_in_block)
        v.pi.load(host_pi)
        return v


def views_group():
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    N, K = 2000, 64
    ds, make = small_learner(N, K)
    lrn = make()
    lrn.Run(10)
    lrn.StartAverage(spread=True)
    lrn.Run(15)
    avg = lrn.Averaged()
    low, mid = avg.Bound(-2), avg.Bound(0)
    assert low.samples == 15 and low.z == -2.0
    mean, var = avg.pi.host(), lrn._average.var.host()
    want = st.bound(mean, var, -2.0)
    assert same_bits(low.pi.host(), want) and same_bits(mid.pi.host(), mean) and same_bits(low.beta.cpu().numpy(), avg.beta.cpu().numpy())
    thr = 0.05
    same = lambda xs, ys: len(xs) == len(ys) and all(np.array_equal(x, y) for x, y in zip(xs, ys))   # noqa: E731
    got, ref = _integers(low, thr), _integers(Plain(avg, want), thr)
    assert len(got) >= 10 and same(got, ref)
    assert np.array_equal(got[0], (want >= F32(thr)).sum(0))
    assert same(_integers(mid, thr), _integers(avg, thr))
    assert not np.array_equal(got[0], _integers(avg, thr)[0]) and (got[0] <= _integers(avg, thr)[0]).all()
    # the view stays valid and refreshes after a further Run(5); an unchanged chain refills nothing
    filled = low._filled
    low.CommunitySizes(thr)
    assert low._filled == filled == (lrn._average.epoch, 15)
    lrn.Run(5)
    sizes = low.CommunitySizes(thr).cpu().numpy()
    assert low.samples == 20 and low._filled == (lrn._average.epoch, 20)
    want = st.bound(avg.pi.host(), lrn._average.var.host(), -2.0)
    assert same_bits(low.pi.host(), want) and np.array_equal(sizes, (want >= F32(thr)).sum(0))
    # a restart with the same `spread` keeps the object, so the views stay valid; after as many steps as before n is what
    # it was, and the bound must still be the new chain's
    keep, old = lrn._average, want
    lrn.StartAverage(spread=True)
    assert lrn._average is keep
    ps.rejects(AmmsbError, (low.drain,))                      # no sample yet
    lrn.Run(20)
    sizes = low.CommunitySizes(thr).cpu().numpy()
    assert low.samples == 20 and avg.samples == 20
    want = st.bound(avg.pi.host(), keep.var.host(), -2.0)
    assert not same_bits(want, old), "the restarted chain left the bound of the one before: the case shows nothing"
    assert same_bits(low.pi.host(), want) and np.array_equal(sizes, (want >= F32(thr)).sum(0))
    assert same(_integers(mid, thr), _integers(avg, thr))
    ps.rejects(AmmsbError, (lambda: avg.Bound(float("nan")), lambda: avg.Bound(float("inf"))))
    lrn.StopAverage()
    ps.rejects(AmmsbError, (low.drain, lambda: low.CommunitySizes(thr), lambda: mid.CommunityQuality(thr)))
    # an average without a spread names the way to get one
    lrn.StartAverage()
    lrn.Run(2)
    e = ps.rejects(AmmsbError, (lambda: lrn.Averaged().Bound(-2), lrn.Averaged().BetaStd))
    assert all("StartAverage(spread=True)" in str(x) for x in e)
    lrn.close()
    print("views ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def cpp_group():
    """tests/cpp/spread_test.cc records every sample of its two loops; the chain is replayed here through the statement
    (replay_samples) and the C++ learner's moments must equal it bit for bit, as learner_group holds the Python learner's
    to the same replay of its own samples; its CommunityQuality under ReadBound(true, -2) against the statement over the
    bound"""
    import tempfile
    import quality_child as qc
    from mcmc_ammsb_gpu_amd import _linkcomm, _quality
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("spread_test", d, 300)
        links = _linkcomm.read_link_communities(os.path.join(d, "links.txt"))[4]
        for loop in ("sync", "async"):
            raw = open(os.path.join(d, loop + ".samples"), "rb").read()
            N, K, n = (int(x) for x in np.frombuffer(raw, np.uint32, 3))
            body = np.frombuffer(raw, np.float32, offset=12).reshape(n, N * K + 2 * K)
            lazy = replay_samples([body[t, :N * K].reshape(N, K) for t in range(n)], [body[t, N * K:] for t in range(n)])
            mean, var = lazy.mean, lazy.var
            mom = open(os.path.join(d, loop + ".moments"), "rb").read()
            got_mean = np.frombuffer(mom, np.float32, N * K).reshape(N, K)
            got_var = np.frombuffer(mom, np.float32, N * K, offset=4 * N * K).reshape(N, K)
            got_vb = np.frombuffer(mom, np.float64, 2 * K, offset=8 * N * K)
            assert same_bits(got_mean, mean) and same_bits(got_var, var), loop
            assert same_bits(got_vb, lazy.m2 / np.float64(n)), loop
            fN, fK, fE, fthr, unc, size, internal, boundary, cond, dens = _quality.read_community_quality(
                os.path.join(d, loop + ".quality"))
            assert (fN, fK) == (N, K) and F32(fthr) == F32(0.05) and fE == links.size
            qc._check_counts(st.bound(got_mean, got_var, -2.0), 0.05, links, (unc, size, internal, boundary), "spread_test " + loop)
            print("cpp %s: %d samples replayed, var and mean bit-equal, quality of Bound(-2) equal" % (loop, n), flush=True)
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
