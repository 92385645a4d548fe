"""Child process of test_gpu_refsample.py (one per group; also `cpu-check`, which needs no GPU): the reference-stream
device sampler against the reference-exact host sampler (hostlib.Dataset.sample == host/sample.cc), bit for bit."""
import ctypes as C
import io
import sys

import numpy as np

import postfit_support as ps

HUB, HUB_DEGREE = 77, 5000
U32 = np.uint64(0xFFFFFFFF)

# name -> (N, avg degree, m, heldout_ratio, [(strategy, batches, first seed)], extra)
#   extra "hub": vertex HUB gets HUB_DEGREE more edges and the first seed makes it the first u;
#   extra "self": small N, many batches: the run must contain a (u, u) edge
CASES = {
    "m32": (1 << 17, 12.0, 32, 0.02, [("Node", 200, 1804289383), ("NodeLink", 200, 846930886),
                                       ("NodeNonLink", 200, 1681692777)], None),
    "m1024": (1 << 17, 12.0, 1024, 0.02, [("Node", 200, 1714636915), ("NodeLink", 200, 1957747793),
                                          ("NodeNonLink", 200, 424238335)], None),
    "m65536": (1000000, 10.0, 65536, 0.01, [("Node", 200, 719885386), ("NodeLink", 200, 1102520059),
                                            ("NodeNonLink", 200, 1649760492)], None),
    "no-heldout": (300000, 10.0, 1024, 0.0, [("Node", 200, 596516649), ("NodeLink", 200, 2044897763),
                                             ("NodeNonLink", 200, 1189641421)], None),
    "self-edge": (4096, 8.0, 32, 0.02, [("NodeNonLink", 2000, 1025202362), ("Node", 1000, 1350490027)], "self"),
    "hub": (1 << 17, 12.0, 1024, 0.02, [("NodeNonLink", 200, None), ("NodeLink", 200, 1967513926), ("Node", 200, 783368690)], "hub"),
}


def canon(a, b):
    a, b = np.uint64(a), np.uint64(b)
    return (np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b)


def dataset(name):
    from mcmc_ammsb_gpu_amd import hostlib
    N, deg, m, hr, runs, extra = CASES[name]
    edges = hostlib.generate_graph(N, 16, deg, seed=7)
    if extra == "hub":
        others = np.arange(1000, 1000 + HUB_DEGREE, dtype=np.uint64)
        edges = np.unique(np.concatenate([edges, canon(np.full(others.size, HUB, dtype=np.uint64), others)]))
        edges = edges[np.random.default_rng(5).permutation(edges.size)]
    if hr == 0.0:
        ds = hostlib.Dataset(N, edges, heldout_ratio=0.0, rand_seed=3)
        assert ds.heldout is None or ds.heldout_edges.size == 0
    else:
        ds = hostlib.Dataset.robust(N, edges, heldout_ratio=hr, rand_seed=3)
    return ds


def heldout_degree(ds):
    he = np.ascontiguousarray(ds.heldout_edges, dtype=np.uint64)
    if ds.heldout is None or he.size == 0:
        return np.zeros(ds.N, dtype=np.int64)
    he = he[ds.heldout.Has(he)]
    ends = np.concatenate([he >> np.uint64(32), he & U32]).astype(np.int64)
    return np.bincount(ends, minlength=ds.N)[:ds.N]


def seed_that_picks(rs, N, vertex, strategy):
    """smallest seed >= 1 whose first u (after the coin of Node) is `vertex`"""
    for seed in range(1, 1 << 26):
        s = seed
        if strategy == "Node":
            _, s = rs.rand_r(s)
        v, _ = rs.rand_r(s)
        if v % N == vertex:
            return seed
    raise AssertionError("no seed found")


def runs_of(name, rs, N):
    out = []
    for strategy, batches, seed in CASES[name][4]:
        out.append((strategy, batches, seed if seed is not None else seed_that_picks(rs, N, HUB, strategy)))
    return out


def calls_between(rs, state, after, limit):
    n = 0
    while state != after:
        _, state = rs.rand_r(state)
        n += 1
        assert n <= limit, "seed afterwards not reached"
    return n


class HostSide:
    """what the host sampler says about a case, and the checks on it that need no device"""

    def __init__(self, name):
        from mcmc_ammsb_gpu_amd import _capi, _refsample as rs
        self.name, self.rs, self.ds = name, rs, dataset(name)
        ds = self.ds
        self.m = CASES[name][2]
        off, tgt = ds.training_csr()
        self.off, self.tgt = off, tgt
        self.degree = np.ascontiguousarray(np.diff(off.astype(np.int64)), dtype=np.uint32)
        self.excluded = self.degree.astype(np.int64) + 1 + heldout_degree(ds)
        self.cand_for = lambda x: int(_capi.load().ammsb_minibatch_candidates_for(ds.N, self.m, (int(x) + 31) // 32 * 32))
        self.capacity = self.cand_for(self.excluded.max())
        assert self.capacity > 0

    def csr_is_the_graphs_adjacency_order(self):
        """NeighborsOf(u) lists neighbours in the order the edges were inserted (include/mcmc/data.h): rebuild that
        from the training edge list and compare with the CSR the device reads"""
        te = self.ds.training_edges
        a, b = (te >> np.uint64(32)).astype(np.int64), (te & U32).astype(np.int64)
        src = np.stack([a, b], axis=1).reshape(-1)   # edge (a, b): a gains b, then b gains a
        dst = np.stack([b, a], axis=1).reshape(-1)
        order = np.argsort(src, kind="stable")
        assert np.array_equal(dst[order].astype(np.uint32), self.tgt)
        assert np.array_equal(np.bincount(src, minlength=self.ds.N), self.degree)

    def batches(self):
        """(strategy, index, seed, link, u, state after u, edges, nodes, weight, seed afterwards, consumed)"""
        lib, rs, ds = self.rs.load(), self.rs, self.ds
        for strategy, n, seed in runs_of(self.name, rs, ds.N):
            for it in range(n):
                e, v, w, after = ds.sample(self.m, strategy, seed)
                s, link, u = C.c_uint32(seed), C.c_uint32(0), C.c_uint32(0)
                assert lib.ammsb_refsample_choose(rs.STRATEGIES[strategy], ds.N, self.degree.ctypes.data, C.byref(s),
                                                  C.byref(link), C.byref(u)) == 0
                consumed = 0
                if not link.value:
                    consumed = calls_between(rs, s.value, after, 1 << 22)
                    cap = min(self.cand_for(self.excluded[u.value]), self.capacity)
                    assert consumed <= cap, "%s %s batch %d: the host stream needs %d candidates, the sizing rule " \
                                            "gives %d" % (self.name, strategy, it, consumed, cap)
                else:
                    assert s.value == after
                yield strategy, it, seed, bool(link.value), int(u.value), int(s.value), e, v, w, after, consumed
                seed = after


def case_facts(h, strategy, it, link, u, state, e, consumed, facts):
    """the properties a case was built for, established on the host sampler's own output"""
    if not link and (e == canon(u, u)).any():
        facts["self_edges"] = facts.get("self_edges", 0) + 1
    if not link and u == HUB and CASES[h.name][5] == "hub" and it == 0:
        s, hit = state, 0
        vs = np.zeros(consumed, dtype=np.uint64)
        for j in range(consumed):
            v, s = h.rs.rand_r(s)
            vs[j] = v % h.ds.N
        hit = int(h.ds.training.Has(canon(np.full(consumed, u, dtype=np.uint64), vs)).sum())
        assert h.degree[u] >= 0.9 * HUB_DEGREE  # (a few hub edges are held out)
        assert hit > 0 and consumed > h.m
        facts["hub_hits"] = hit


def check_facts(name, facts):
    extra = CASES[name][5]
    if extra == "self":
        assert facts.get("self_edges", 0) > 0, "the run holds no (u, u) edge: choose other seeds"
    if extra == "hub":
        assert facts.get("hub_hits", 0) > 0, "the hub was never u"


def cpu_check(names):
    for name in names:
        h = HostSide(name)
        h.csr_is_the_graphs_adjacency_order()
        facts, n, worst = {}, 0, 0.0
        for strategy, it, seed, link, u, state, e, v, w, after, consumed in h.batches():
            case_facts(h, strategy, it, link, u, state, e, consumed, facts)
            if not link:
                worst = max(worst, consumed / min(h.cand_for(h.excluded[u]), h.capacity))
            n += 1
        check_facts(name, facts)
        print("cpu-check ok %s: %d batches, capacity %d, worst consumed/candidates %.3f, %s" % (name, n, h.capacity, worst, facts),
              flush=True)


def sampler_group(name):
    import torch
    from mcmc_ammsb_gpu_amd import ops
    h = HostSide(name)
    h.csr_is_the_graphs_adjacency_order()
    ds, m = h.ds, h.m
    ctx = ops.Context(ops.make_params(ds.N, 32, E=ds.E, num_node_sample=8))
    ts = ops.DeviceSet(ctx, ds.training.Serialize(), ds.training.BinsPerBucket(), ds.training.PrimeIdx())
    hs = None
    if ds.heldout is not None and ds.heldout_edges.size:
        hs = ops.DeviceSet(ctx, ds.heldout.Serialize(), ds.heldout.BinsPerBucket(), ds.heldout.PrimeIdx())
    assert (hs is None) == (CASES[name][3] == 0.0)
    smp = ops.ReferenceStreamSampler(ctx, h.off, h.tgt, ts, hs, m, heldout_degree=heldout_degree(ds))
    assert smp.C == h.capacity
    de = ctx.zeros((ds.max_edges(m),), torch.int64)
    dv = ctx.zeros((ds.max_nodes(m),), torch.int32)
    facts, n, links = {}, 0, 0
    for strategy, it, seed, link, u, state, e, v, w, after, consumed in h.batches():
        case_facts(h, strategy, it, link, u, state, e, consumed, facts)
        ne, nv, gw, gafter = smp.enqueue(strategy, seed, de, dv)   # waits for the result bytes itself
        torch.cuda.synchronize()
        ge = de[:ne].cpu().numpy().view(np.uint64)
        gv = dv[:nv].cpu().numpy().view(np.uint32)
        where = "%s %s batch %d (seed %d, u %d, %s)" % (name, strategy, it, seed, u, "link" if link else "non-link")
        assert ne == e.size and nv == v.size, "%s: sizes %d %d, host %d %d" % (where, ne, nv, e.size, v.size)
        assert np.array_equal(ge, e), "%s: edges differ (first at %d)" % (where, int(np.flatnonzero(ge != e)[0]))
        assert np.array_equal(gv, v), "%s: nodes differ (first at %d)" % (where, int(np.flatnonzero(gv != v)[0]))
        assert gw == w, "%s: weight %r, host %r" % (where, gw, w)
        assert gafter == after, "%s: seed afterwards %d, host %d" % (where, gafter, after)
        if not link:
            assert smp.last_consumed == consumed, where
        links += link
        n += 1
    check_facts(name, facts)
    want = sum(r[1] for r in CASES[name][4])
    assert n == want
    print("sampler ok %s: %d batches (%d link), %d epochs, %s" % (name, n, links, smp.num_epochs, facts), flush=True)


def shortfall_group():
    """a candidate capacity too small for m: the call reports it (exception + sticky counter), writes inside the
    buffers only, and the sampler goes on working"""
    import torch
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    h = HostSide("m1024")
    ds, m = h.ds, h.m
    ctx = ops.Context(ops.make_params(ds.N, 32, E=ds.E, num_node_sample=8))
    ts = ops.DeviceSet(ctx, ds.training.Serialize(), ds.training.BinsPerBucket(), ds.training.PrimeIdx())
    hs = ops.DeviceSet(ctx, ds.heldout.Serialize(), ds.heldout.BinsPerBucket(), ds.heldout.PrimeIdx())
    smp = ops.ReferenceStreamSampler(ctx, h.off, h.tgt, ts, hs, m, heldout_degree=heldout_degree(ds), capacity=512)
    guard = 4096
    de = torch.full((ds.max_edges(m) + guard,), -7, dtype=torch.int64, device=ctx.device)
    dv = torch.full((ds.max_nodes(m) + guard,), -7, dtype=torch.int32, device=ctx.device)
    try:
        smp.enqueue("NodeNonLink", 12345, de, dv)
        raise AssertionError("512 candidates cannot hold 1024 edges: no error reported")
    except AmmsbError as e:
        assert "fewer than 1024 distinct non-links" in str(e), str(e)
    torch.cuda.synchronize()
    r = smp.result.contents
    assert r.shortfall == 1 and r.n_edges <= 512 and r.n_nodes <= 513 and r.consumed == 512
    assert bool((de[512:] == -7).all()) and bool((dv[513:] == -7).all()), "wrote past what it reported"
    assert smp.shortfalls == 1
    try:
        smp.check()
        raise AssertionError("sticky counter not reported")
    except AmmsbError:
        pass
    smp.check()  # cleared
    # a link mini-batch needs no candidates: the same sampler still answers, and exactly
    e, v, w, after = ds.sample(m, "NodeLink", 999)
    ne, nv, gw, gafter = smp.enqueue("NodeLink", 999, de, dv)
    torch.cuda.synchronize()
    assert np.array_equal(de[:ne].cpu().numpy().view(np.uint64), e) and np.array_equal(dv[:nv].cpu().numpy().view(np.uint32), v)
    assert (gw, gafter) == (w, after)
    print("shortfall ok", flush=True)


def _state(lrn):
    import torch
    lrn.drain()
    rows = np.unique(np.linspace(0, lrn.cfg.N - 1, 4096).astype(np.int64))
    pi = lrn.pi.host()[rows]
    return dict(pi=pi, beta=lrn.beta.cpu().numpy(), theta=lrn.theta.cpu().numpy(), phi=lrn.phi.cpu().numpy(),
                seeds=np.array([s.seed for s in lrn.samples], dtype=np.uint64), step=np.array([lrn.stepCount]))


def _same(a, b, what):
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k].view(np.uint8), b[k].view(np.uint8)), "%s: %s differs" % (what, k)


def trajectory_group(workload, parallel):
    _, learner = ps.c1_learner(False, workload)

    def make(ref):
        lrn = learner(sample_parallel=parallel, device_sampling=ref, sampling_stream="reference" if ref else "own")
        assert lrn.loop is None and (lrn.ref_sampler is not None) == ref and lrn.dev_sampler is None
        return lrn
    first, second = 30, 30
    host, ref = make(False), make(True)
    host.Run(first)
    ref.Run(first)
    _same(_state(host), _state(ref), "%s after %d steps" % (workload, first))
    ck_host, ck_ref = io.BytesIO(), io.BytesIO()
    host.Serialize(ck_host)
    ref.Serialize(ck_ref)
    assert len(ck_host.getvalue()) == len(ck_ref.getvalue())   # same records (the bytes hold wall-clock times too)
    host.Run(second)
    ref.Run(second)
    end = _state(host)
    _same(end, _state(ref), "%s after %d steps" % (workload, first + second))
    assert int(end["step"][0]) == first + second + 1
    ppx = host.HeldoutPerplexity()
    assert ref.HeldoutPerplexity() == ppx
    host.close()
    ref.close()
    for mode, blob in ((True, ck_host), (False, ck_ref)):   # resume each checkpoint in the OTHER mode
        lrn = make(mode)
        blob.seek(0)
        lrn.Parse(blob)
        lrn.Run(second)
        _same(end, _state(lrn), "%s resumed in %s mode" % (workload, "reference-stream" if mode else "host"))
        lrn.close()
    print("trajectory ok %s parallel=%s: %d steps, perplexity %.6f" % (workload, parallel, first + second, ppx), flush=True)


GROUPS = {
    "cpu-check": lambda a: cpu_check(a or sorted(CASES)),
    "sampler": lambda a: sampler_group(a[0]),
    "shortfall": lambda a: shortfall_group(),
    "trajectory": lambda a: trajectory_group(a[0], a[1] == "1"),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
