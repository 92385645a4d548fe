"""Child process of test_gpu_reduce.py (one per group): merging and dropping communities (include/ammsb_reduce.h,
ops.ModelReducer, Learner.Reduce) against reduce_statement.py, which test_reduce_host.py checks on the CPU against the dense
float64 definition.  Everything the device writes -- pi', phi_sum', theta', the count of emptied rows -- is asserted bit for
bit."""
import sys

import numpy as np

import postfit_support as ps
import reduce_statement as st
from average_child import FILL_F, Blocks, same_bits

F32 = np.float32
FILL_I = 0x5A5A5A5A5A5A5A5A


class Bench:
    def __init__(self):
        from mcmc_ammsb_gpu_amd import _reduce, ops
        self.b = ps.DeviceBench()
        self.rd, self.ops, self.torch = _reduce, ops, self.b.torch
        self.red = ops.ModelReducer(self.b.ctx)


# ------------------------------------------------------------------------------------------------------------ exact
N_EXACT, RIB, RIB_OUT = 3000, 1100, 1300     # pi in blocks of 1100, 1100, 800 rows; the outputs cut elsewhere
# every group width (13 and 30: 4 and 8 lanes), both load widths, blocks of 256 and (above 4096 columns) 128 lanes, a ragged
# last column trip at 4160; (64, 1): every block 4 bytes off a 16-byte boundary -> the 4-byte form
EXACT_CASES = [(1, 0), (5, 0), (13, 0), (30, 0), (64, 0), (65, 0), (256, 0), (1024, 0), (64, 1), (4096, 0), (4160, 0), (8192, 0)]
ZERO_ROW, NAN_ROW, DROPPED_ROW = 5, 1101, 2999   # one in every block of pi


def exact_plans(K, rng):
    """name -> map[K]; plans that coincide at a small K are listed once"""
    plans = {"identity": np.arange(K), "reversal": np.arange(K)[::-1].copy()}
    third = np.full(K, -1, np.int64)
    third[::3] = np.arange(len(third[::3]))
    plans["every third"] = third
    plans["all into one"] = np.zeros(K, np.int64)
    for name, drop in (("groups", False), ("groups, drops", True)):
        m = np.full(K, -1, np.int64)
        cols = rng.permutation(K)                       # interleaved: the sources of a group lie anywhere in the row
        kept = cols[:max(1, K - K // 4)] if drop else cols
        j = at = 0
        while at < kept.size:
            n = 1 + j % 7
            m[kept[at:at + n]] = j
            at += n
            j += 1
        plans[name] = m
    if K > 1:
        one_less = np.arange(K) - 1                     # K' = K - 1: the first two merged
        one_less[0] = 0
        plans["K - 1"] = one_less
    seen, out = set(), {}
    for name, m in plans.items():
        if m.tobytes() not in seen:
            seen.add(m.tobytes())
            out[name] = m.astype(np.int64)
    return out


def exact_rows(rng, K):
    p = rng.random((N_EXACT, K), dtype=np.float32) ** 8 + F32(1e-6)
    p = (p / p.sum(1, keepdims=True, dtype=np.float32)).astype(np.float32)
    p[rng.random((N_EXACT, K), dtype=np.float32) < 0.2] = 0   # zeros everywhere
    p[10:20] *= F32(1e-38)                              # rows of subnormals (and zeros)
    p[ZERO_ROW] = 0
    p[NAN_ROW, K // 2] = np.nan
    return p


def run_plan(bn, pi, phi, theta, plan, select, slabs, off):
    """one pass over fresh guarded outputs -> (the blocks of pi', phi', theta', emptied, the form of the row kernel)"""
    b, torch = bn.b, bn.torch
    new_K = plan.new_K
    out = Blocks(b, N_EXACT, new_K, RIB_OUT, float("nan"), off)
    ophi = b.guarded(N_EXACT, torch.float32, FILL_F)
    oth = b.guarded(2 * new_K, torch.float32, FILL_F)
    emptied = b.guarded(1, torch.int64, FILL_I, zero=True)
    dplan = bn.red.device_plan(plan, select)
    names = set()
    for lo, hi in slabs:
        bn.red.rows(pi, phi, dplan, out, ophi[:N_EXACT], emptied[:1], first=lo, count=hi - lo)
        names.add(bn.red.kernel_name())
    bn.red.theta(theta, dplan, oth[:2 * new_K])
    assert bn.red.kernel_name() == "reduce_theta" and len(names) == 1
    assert out.guards_ok() and bool((ophi[N_EXACT:] == FILL_F).all()) and bool((oth[2 * new_K:] == FILL_F).all())
    assert bool((emptied[1:] == FILL_I).all())
    return out, ophi[:N_EXACT].cpu().numpy(), oth[:2 * new_K].cpu().numpy().reshape(-1, 2), int(emptied[0]), names.pop()


def exact_case(bn, K, off, seed):
    b = bn.b
    rng = np.random.default_rng(seed)
    hp = exact_rows(rng, K)
    hphi = (rng.random(N_EXACT, dtype=np.float32) * 40 + 1).astype(np.float32)
    hth = rng.gamma(1.0, 1.0, (K, 2)).astype(np.float32)
    pi = Blocks(b, N_EXACT, K, RIB, 0.0, off)
    phi, theta = b.dev(hphi), b.dev(hth.reshape(-1))
    vec = K % 4 == 0 and off == 0
    done = []
    # pi is uploaded once and kept beside a copy on the device; a plan changes one row of both and of the host array
    pi.load(hp)
    kept = pi.clone()
    blk, loc = divmod(DROPPED_ROW, RIB)
    rows, original = hp, hp[DROPPED_ROW].copy()
    for name, m in exact_plans(K, rng).items():
        plan = bn.rd.Plan(m)
        # a dropping plan: a row whose mass sits in dropped columns alone
        rows[DROPPED_ROW] = np.where(m < 0, F32(1.0) / F32(max(1, (m < 0).sum())), F32(0)) if plan.drops else original
        for p in (pi, kept):
            p.views[blk][loc].copy_(b.dev(rows[DROPPED_ROW]))
        want_pi, want_phi, want_empty = st.rows(rows, hphi, m)
        want_th = st.theta(hth, m)
        want_dev = [b.dev(want_pi[lo:lo + RIB_OUT]).view(bn.torch.int32) for lo in range(0, N_EXACT, RIB_OUT)]   # compared on the device
        if plan.drops:
            # (the NaN row is emptied where the plan keeps the NaN's column; at a small K other rows hold zeros alone too)
            assert want_empty[[ZERO_ROW, DROPPED_ROW]].all() and want_empty[NAN_ROW] == (m[K // 2] >= 0) and not want_empty.all()
            assert not np.isnan(want_pi).any()
        else:
            assert not want_empty.any() and np.isnan(want_pi[NAN_ROW]).any()
        forms = [True, False] if plan.selects else [False]
        for select in forms:
            form = ("reduce_select_" if select else "reduce_merge_") + ("v4" if vec else "s1")
            for slabs in (((0, 1000), (1000, 1001), (1001, N_EXACT)), ((0, N_EXACT),)):
                got_pi, got_phi, got_th, got_empty, got_form = run_plan(bn, pi, phi, theta, plan, select, slabs, off)
                what = (K, off, name, form, len(slabs))
                assert got_form == form, what
                assert all(bool(bn.torch.equal(v.view(bn.torch.int32), w)) for v, w in zip(got_pi.views, want_dev)), what
                assert same_bits(got_phi, want_phi) and same_bits(got_th, want_th) and got_empty == int(want_empty.sum()), what
        if name in ("identity",):
            assert same_bits(want_pi, rows) and same_bits(want_th, hth)
        i32 = bn.torch.int32
        assert pi.guards_ok() and all(bool(bn.torch.equal(v.view(i32), w.view(i32))) for v, w in zip(pi.views, kept.views))  # only read
        done.append("%s K'=%d%s" % (name, plan.new_K, " drops" if plan.drops else ""))
    print("exact K=%d off=%d (%s, group of %d lanes): %s" % (K, off, "v4" if vec else "s1", bn.rd.group_lanes(K), "; ".join(done)),
          flush=True)


def exact_group(which):
    bn = Bench()
    for i in which:
        K, off = EXACT_CASES[i]
        exact_case(bn, K, off, 200 + i)
    print("exact ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ far
def far_group():
    """DeviceBench.big_pi: K = 8192, rows past byte 2^32, element 2^31 and element 2^32 of a block, aligned and 4 bytes
    off.  Narrow out: K' = 8 (1024 sources each, nothing dropped) over every row, and a dropping plan over the planted
    windows alone.  Wide out: a permutation at K' = 8192 into a second zeroed block of the same size, whose rows past 2^19
    lie past element 2^32 too.  One pair of big blocks alive at a time."""
    bn = Bench()
    b, torch = bn.b, bn.torch
    K, N = ps.BIG_K, ps.BIG_ROWS
    ids, wins = ps.big_ids(), ps.big_windows()
    narrow = np.arange(K) % 8
    narrow_drop = np.where(np.arange(K) % 3 == 0, -1, np.arange(K) % 8)
    perm = np.random.default_rng(9).permutation(K)
    slab = 1 << 16

    def check(blk, want, what):
        """the planted windows against the statement; every other row all-zero, on the device"""
        at = 0
        for (lo, hi), nxt in zip(wins, [w[0] for w in wins[1:]] + [N]):
            assert same_bits(blk[lo:hi].cpu().numpy(), want[at:at + hi - lo]), (what, lo)
            at += hi - lo
            assert not bool(blk[hi:nxt].any()), (what, "rows", hi, nxt)

    for mis in (False, True):
        form = "s1" if mis else "v4"
        pi, compact, _ = b.big_pi(31 + mis, mis)
        phi = b.ctx.zeros((N,), torch.float32)
        phi[b.dev(ids)] = 2.0
        ophi = b.ctx.zeros((N,), torch.float32)
        emptied = b.ctx.zeros((1,), torch.int64)
        # a kernel that kept row * K in 32 bits would read the rows [0, 128) for the rows past 2^19: other values
        wrapped = ps.big_wrapped(compact)
        for m in (narrow, narrow_drop, perm):
            a, w = st.rows(compact, np.full(ids.size, 2, F32), m)[0], st.rows(wrapped, np.full(ids.size, 2, F32), m)[0]
            assert same_bits(a[ids < (1 << 19)], w[ids < (1 << 19)]) and not (a[ids >= (1 << 19)] == w[ids >= (1 << 19)]).all(1).any()
        # narrow out, nothing dropped, every row
        out, blk = b.zeroed(N, 8, mis)
        dplan = bn.red.device_plan(bn.rd.Plan(narrow))
        for lo in range(0, N, slab):
            bn.red.rows(pi, phi, dplan, out, ophi, emptied, first=lo, count=min(slab, N - lo))
        assert bn.red.kernel_name() == "reduce_merge_" + form
        want, want_phi, _ = st.rows(compact, np.full(ids.size, 2, F32), narrow)
        check(blk, want, ("narrow", mis))
        assert same_bits(ophi[b.dev(ids)].cpu().numpy(), want_phi) and float(ophi.sum()) == 2.0 * ids.size and int(emptied[0]) == 0
        # narrow out, a third of the columns dropped, the windows alone
        out, blk = b.zeroed(N, 8, mis)
        ophi.zero_()
        dplan = bn.red.device_plan(bn.rd.Plan(narrow_drop))
        for lo, hi in wins:
            bn.red.rows(pi, phi, dplan, out, ophi, emptied, first=lo, count=hi - lo)
        want, want_phi, want_empty = st.rows(compact, np.full(ids.size, 2, F32), narrow_drop)
        check(blk, want, ("narrow, drops", mis))
        assert same_bits(ophi[b.dev(ids)].cpu().numpy(), want_phi) and int(emptied[0]) == int(want_empty.sum()) == 0
        assert int((ophi != 0).sum()) == ids.size
        del out, blk
        # wide out: a permutation into a second block of pi's size
        out, blk = b.zeroed(N, K, mis)
        dplan = bn.red.device_plan(bn.rd.Plan(perm))
        for lo in range(0, N, slab):
            bn.red.rows(pi, phi, dplan, out, ophi, emptied, first=lo, count=min(slab, N - lo))
        assert bn.red.kernel_name() == "reduce_select_" + form
        want = st.rows(compact, np.full(ids.size, 2, F32), perm)[0]
        assert same_bits(want[:, perm], compact)
        check(blk, want, ("wide", mis))
        del pi, out, blk, dplan
        b.release()
        print("far %s: %d planted rows up to element %d, in and out" % (form, ids.size, N * K - 1), flush=True)
    print("far ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ learner
def learner_state(lrn):
    lrn.drain()
    return lrn.pi.host(), lrn.phi.cpu().numpy(), lrn.theta.cpu().numpy().reshape(-1, 2), lrn.beta.cpu().numpy()


def learner_group(graph):
    from mcmc_ammsb_gpu_amd._capi import AmmsbError
    from mcmc_ammsb_gpu_amd._reduce import Plan
    graph = bool(int(graph))
    N, K = ps.WORKLOADS["C1"][:2]
    ds, make = ps.c1_learner(graph)
    lrn = make()
    assert (lrn.loop is not None) == graph
    lrn.Run(20)
    old = learner_state(lrn)
    # the identity: the same model bit for bit, at the same point of the step-size schedule
    new = lrn.Reduce(Plan.identity(K))
    assert all(same_bits(x, y) for x, y in zip(old, learner_state(new)))
    assert new.stepCount == lrn.stepCount == 21 and new.edges_done == lrn.edges_done and new.reduced_from == (K, 0)
    assert new.phiUpdater.count_calls == lrn.phiUpdater.count_calls == 20 and (new.loop is not None) == graph
    assert new.cfg.K == K and new.cfg.alpha == lrn.cfg.alpha and new.cfg is not lrn.cfg
    new.close()
    # a plan from the diagnostics (whatever they find after 20 iterations), with one merge and one drop that do not depend on them
    rel = lrn.RelatedCommunities(0.05, top=4)
    jac = np.sort(rel.jaccard[rel.partner >= 0])
    dups = rel.duplicates(float(jac[-3])) if jac.size >= 3 else []
    plan = Plan.identity(K).merge(dups).merge([(0, 1)]).drop([K - 1]).drop_smaller(lrn.CommunitySizes(0.05), 2)
    assert plan.drops and not plan.selects and plan.new_K < K - 1
    print("learner: %d duplicate pairs, %r" % (len(dups), plan), flush=True)
    before = lrn.HeldoutPerplexity()
    old = learner_state(lrn)
    new = lrn.Reduce(plan)
    want_pi, want_phi, want_empty = st.rows(old[0], old[1], plan.map)
    want_th = st.theta(old[2], plan.map)
    got = learner_state(new)
    assert same_bits(got[0], want_pi) and same_bits(got[1], want_phi) and same_bits(got[2], want_th)
    assert new.reduced_from == (K, int(want_empty.sum())) and new.cfg.K == plan.new_K == new.pi.cols
    want_beta = new.ctx.zeros((2 * plan.new_K,), new.ops.torch.float32)
    new.ops.beta_from_theta(new.ctx, new.ctx.from_numpy(want_th.reshape(-1)), want_beta)
    assert same_bits(got[3], want_beta.cpu().numpy())
    assert all(same_bits(x, y) for x, y in zip(old, learner_state(lrn)))          # the old learner's state stands
    after = new.HeldoutPerplexity()
    new.Run(5)
    trained = new.HeldoutPerplexity()
    assert new.stepCount == 26 and np.isfinite([after, trained]).all()
    ids, weights, count = new.Memberships(top=2)
    assert tuple(ids.shape) == (N, 2) and int(ids.max()) < plan.new_K
    q = new.CommunityQuality(0.05)
    assert len(q.size) == plan.new_K
    print("learner (%s): held-out perplexity %.4f at K = %d, %.4f reduced to K' = %d, %.4f after 5 more iterations"
          % ("graph" if graph else "eager", before, K, after, plan.new_K, trained), flush=True)
    new.close()
    lrn.close()
    # the old learner goes on as if nothing had happened
    fixed = Plan.identity(K).merge([(2, 9), (9, 30)]).drop([5])
    ps.unperturbed_run(make, lambda a: a.Reduce(fixed).close(), "Reduce")
    if not graph:
        x = make(device_sampling=False, graph_launch=False, force_exchange=True, phi_replicate=0.0)
        e = ps.rejects(AmmsbError, (lambda: x.Reduce(fixed),))
        assert "one rank" in str(e[0])
        x.close()
        y = make()
        e = ps.rejects(AmmsbError, (lambda: y.Reduce(Plan.identity(K + 1)), lambda: y.Reduce(Plan.identity(K - 1))))
        assert "plan over" in str(e[0])
        y.close()
    print("learner ok", flush=True)


# ------------------------------------------------------------------------------------------------------------ cpp
def cpp_group():
    """tests/cpp/reduce_test.cc: mcmc::Learner::Reduce against its own restatement in the synchronous, the async and the
    graph loop; the plan file it writes holds the bytes of Python's text form of the same plan"""
    import os
    import tempfile
    from mcmc_ammsb_gpu_amd._reduce import Plan, plan_text, read_plan
    with tempfile.TemporaryDirectory() as d:
        ps.run_cpp_test("reduce_test", d, 300)
        plan = Plan.identity(64).merge([(3, 17), (17, 40), (8, 9)]).drop([5, 63])
        path = os.path.join(d, "cpp.plan")
        assert open(path, "rb").read() == plan_text(plan).encode() and read_plan(path) == plan
    print("cpp ok", flush=True)


GROUPS = {
    "exact": lambda a: exact_group(tuple(int(i) for i in a)),
    "far": lambda a: far_group(),
    "learner": lambda a: learner_group(a[0]),
    "cpp": lambda a: cpp_group(),
}


if __name__ == "__main__":
    ps.child_main(GROUPS, sys.argv[1:])
