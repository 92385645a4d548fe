"""Runs the rows of one environment group of kernel_forms.ROWS against the oracle, in this (child) process.

    python kernel_forms_child.py GROUP REF_IN|- [REF_OUT]
    python kernel_forms_child.py GROUP edges [FIRST LAST [REF_IN]]
    python kernel_forms_child.py 0 edge-refs REF_OUT

GROUP indexes kernel_forms.groups(); the caller sets that group's environment.  REF_IN: an .npz of default-form
gradients (keyed by ref_key) that the gradient rows of this group must equal bit for bit ("-": none).  REF_OUT: where
to save, computed with this process's dispatch, the gradients of every gradient row of the OTHER groups that keeps the
slot count (the default group writes it).  Prints "row ok <index>" per row and "group ok" at the end.

`edges`: the phi, grads and fused rows of the group (those with FIRST <= index in ROWS <= LAST) on the inputs of
division_edges.py, which put every form on both sides of its exact-division branch; every comparison bit for bit
(both-NaN allowed).  REF_IN: default-form gradients of the same inputs, written by `0 edge-refs REF_OUT` in the default
environment, for the gradient rows of another group.  Prints "edge ok <index>" per row and "group ok".
"""
import contextlib
import ctypes as C
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import division_edges as de  # noqa: E402
import kernel_forms as kf  # noqa: E402

SLOT = {k: i for i, k in enumerate(("update_phi", "update_pi", "beta_grads", "perplexity", "update_phi_small",
                                    "sample_neighbors", "grads_sum"))}
MAX_PARTIALS = 4096  # ammsb_ctx.max_partials


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ref_key(row):
    return "%s_b%d" % ("_".join(str(v) for v in row.shape), row.blocks)


def keeps_slots(row):
    return "beta_slots" not in row.debug and not any(k == "AMMSB_BETA_SLOTS" for k, _ in row.env)


def raw_names(ctx):
    return {k: ctx.lib.ammsb_last_kernel_name(ctx.handle, i).decode() for k, i in SLOT.items()}


def check_names(ctx, row, what):
    got = raw_names(ctx)
    for slot, want in row.kernel.items():
        assert kf.normalize(got[slot]) == want, (what, slot, got[slot], want, row)


# ---- the edges mode: what a row runs (shared with test_division_edges_host.py, which checks the coverage on the CPU)
EDGE_NODES = 96
EDGE_DEG = 16  # both directions: about 32 graph neighbours per node, so half of any neighbour row can be links


def edge_deg(row):
    """graph density of a row's state: for the gradient a graph in which the node of largest degree has well over a
    hundred links (about 300 edges in the list), as far as N leaves as many non-neighbours"""
    return EDGE_DEG if row.op == "phi" else grad_deg(row.shape[0])


def grad_deg(N):
    return min(64, N // 4)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def edge_nodes(row):
    """mini-batch nodes of a phi row in the edges mode: its own, but 96 for a row of more than 512 whose form does not
    depend on the count (the small-launch, persistent-grid and stream rows keep theirs)"""
    nodes = row.shape[3]
    keeps = row.flags == "small" or any(k in ("AMMSB_PHI_PERSIST", "AMMSB_PHI_STREAM") for k, _ in row.env)
    return nodes if nodes <= 512 or keeps else EDGE_NODES


def edge_state_shape(row):
    """(N, K, n, mini-batch nodes) of the Problem a row's edges run builds"""
    N, K, n = row.shape[:3]
    return (N, K, n, edge_nodes(row) if row.op == "phi" else 16)


def phi_case(st, case, eps):
    """applies `case` to the state and asserts its coverage conditions; returns (classes, tally)"""
    de.apply_case(st, case, eps)
    cls = de.classify_phi(st, eps)
    return cls, de.check_phi_coverage(case, cls)


def grad_case(orc, p_orc, st, case, eps, fused, wg):
    """The pi state of `case`, its node-strategy edge list, coverage asserted.  fused: phi_vec rows are planted so that
    update_pi reproduces (up to its normalisation) the edited pi rows of u and the partners; the classes are those of
    the pi rows AFTER the oracle's update_pi, which is what the gradient of the fused launch reads."""
    rng = np.random.default_rng(17)
    {"trained": de.trained, "denormal": de.denormal}.get(case, lambda s, r: de.mixed(s, r, eps))(st, rng)
    u, partners, links = de.grad_edges(st, rng, eps)
    c = {"u": u, "partners": partners, "links": links,
         "edges": ((np.minimum(u, partners).astype(np.uint64) << np.uint64(32)) | np.maximum(u, partners).astype(np.uint64))}
    c["pi"] = st.pi_h
    if fused:
        c["nodes"] = np.concatenate([[u], partners]).astype(np.uint32)
        with np.errstate(all="ignore"):
            c["phi_vec"] = (st.pi_h[c["nodes"]] * st.phi_sum_h[c["nodes"], None]).astype(np.float32)
        c["pi"], c["phi_sum"] = st.pi_h.copy(), st.phi_sum_h.copy()
        orc.update_pi(p_orc, c["pi"].reshape(-1), c["phi_sum"], c["phi_vec"].reshape(-1), c["nodes"], wg, 1)
        after = de.State()
        after.pi_h, after.beta_h = c["pi"], st.beta_h
        st = after
    c["fast"] = de.classify_grads(st, eps, u, partners, links)
    c["count"] = de.check_grad_coverage(case, links, c["fast"])
    return c


class Runner:
    def __init__(self):
        import torch
        import ammsb_pkg
        ammsb_pkg.load()
        from mcmc_ammsb_gpu_amd import ops as hip
        import oracle_lib as orc
        orc.build()
        from test_gpu_parity import Problem
        self.torch, self.hip, self.orc, self.Problem = torch, hip, orc, Problem

    def problem(self, row, n_nodes=None, deg=16):
        N, K, n, nodes, _ = row.shape
        pr = self.Problem(self.orc, self.hip, N, K, n, nodes if n_nodes is None else n_nodes, deg=deg)
        if row.blocks == 2:  # rows of the mini-batch on both sides of a block boundary
            rib = N // 2 + 1
            if not ((pr.nodes_h < rib).any() and (pr.nodes_h >= rib).any()):
                rib = max(int(np.sort(pr.nodes_h)[pr.nodes_h.size // 2]), N // 30 + 1)
            pr.pi = self.hip.RowPartitionedMatrix(pr.ctx, N, K, rib)
            pr.pi.load(pr.pi_h)
            assert len(pr.pi.Blocks()) >= 2 and (pr.nodes_h < rib).any() and (pr.nodes_h >= rib).any()
        assert (len(pr.pi.Blocks()) == 1) == (row.blocks == 1)
        return pr

    # ---- update_phi + update_pi: noise on and off, two steps; phi_vec, streams, pi rows, phi_sum bit for bit
    def phi(self, row):
        orc, hip = self.orc, self.hip
        N, K, n, nodes, wg = row.shape
        if any(k == "AMMSB_PHI_PERSIST" for k, _ in row.env):  # more groups than any occupancy keeps resident
            assert nodes > 32 * self.torch.cuda.get_device_properties(0).multi_processor_count, row
        for noise in (False, True):
            pr = self.problem(row, deg=4 if N > 10000 else 16)
            upd = hip.PhiUpdater(pr.ctx, pr.beta, pr.pi, pr.phi_sum, pr.dset, nodes, (42, 43), wg,
                                 phi_disable_noise=not noise, streaming_only=row.flags == "streaming")
            seeds = orc.rng_init(nodes * wg, 42, 43)
            pi_h, phi_sum_h = pr.pi_h.copy(), pr.phi_sum_h.copy()
            for step in (1, 2):
                upd(pr.nodes, pr.nb, nodes)
                pr.sync()
                check_names(pr.ctx, row, "step %d" % step)
                want = orc.update_phi(pr.p_orc, pr.beta_h, pi_h.reshape(-1), phi_sum_h, pr.oset, pr.nodes_h,
                                      pr.nb_h.reshape(-1), step, seeds, wg, 1, noise)
                got = upd.phi_vec.cpu().numpy()[:nodes]
                assert np.array_equal(bits(got), bits(want)), ("phi_vec", noise, step, row)
                assert np.array_equal(upd.rand.host(), seeds), ("streams", noise, step, row)
                orc.update_pi(pr.p_orc, pi_h.reshape(-1), phi_sum_h, want.reshape(-1), pr.nodes_h, wg, 1)
                if N > 10000:  # (large N: the mini-batch rows only)
                    rows = np.unique(pr.nodes_h)
                    assert np.array_equal(bits(pr.pi.host()[rows]), bits(pi_h[rows])), ("pi", noise, step, row)
                else:
                    assert np.array_equal(bits(pr.pi.host()), bits(pi_h)), ("pi", noise, step, row)
                assert np.array_equal(bits(pr.phi_sum.cpu().numpy()), bits(phi_sum_h)), ("phi_sum", noise, step, row)
            pr.ctx.close()

    def _edges(self, pr, n_edges):
        rng = pr.rng
        N = pr.N
        non = self.orc.make_edge(rng.integers(0, N, n_edges), rng.integers(0, N, n_edges))
        mbe = np.concatenate([pr.edges[: n_edges // 3], non[: n_edges - n_edges // 3]]).astype(np.uint64)
        rng.shuffle(mbe)
        return mbe

    def gradient(self, row):
        """the gradient of row's mini-batch with this process's dispatch (no checks): what the default group saves"""
        pr = self.problem(row, n_nodes=16)
        mbe = self._edges(pr, row.shape[3])
        upd = self.hip.BetaUpdater(pr.ctx, pr.theta, pr.beta, pr.pi, pr.dset, (44, 45), row.shape[4])
        upd.count_calls += 1
        g = upd.calculate_grads(pr.ctx.from_numpy(mbe), mbe.size).cpu().numpy().copy()
        pr.ctx.close()
        return g

    # ---- gradient: 1e-5 relative of the oracle's f64 sum, theta_sum bit for bit, the default form's bits where P is kept
    def grads(self, row, ref):
        orc, hip = self.orc, self.hip
        N, K, _, n_edges, wg = row.shape
        pr = self.problem(row, n_nodes=16)
        mbe = self._edges(pr, n_edges)
        upd = hip.BetaUpdater(pr.ctx, pr.theta, pr.beta, pr.pi, pr.dset, (44, 45), wg)
        upd.count_calls += 1
        old = os.environ.get("AMMSB_BETA_SLOTS")
        if "beta_slots" in row.debug:
            os.environ["AMMSB_BETA_SLOTS"] = row.debug["beta_slots"]
        try:
            g = upd.calculate_grads(pr.ctx.from_numpy(mbe), mbe.size).cpu().numpy().copy()
        finally:
            if "beta_slots" in row.debug:
                if old is None:
                    del os.environ["AMMSB_BETA_SLOTS"]
                else:
                    os.environ["AMMSB_BETA_SLOTS"] = old
        check_names(pr.ctx, row, "grads")
        exact = orc.beta_grads(pr.p_orc, pr.theta_h, pr.beta_h, pr.pi_h.reshape(-1), pr.oset, mbe, wg, 1, order=1)
        err = np.abs(g.astype(np.float64) - exact).max() / np.abs(exact).max()
        assert err <= 1e-5, ("grads", err, row)
        ts = np.zeros(K, dtype=np.float32)
        orc.lib().orc_sum_theta(pr.theta_h, ts, K)
        assert np.array_equal(bits(upd.GetThetaSum().cpu().numpy()), bits(ts)), ("theta_sum", row)
        if ref is not None and keeps_slots(row):
            assert np.array_equal(bits(g), bits(ref)), ("grads differ from the default form", row)
        if "beta_slots" in row.debug:
            P = min(n_edges, min(max(int(row.debug["beta_slots"]), 64), MAX_PARTIALS))
            assert np.array_equal(bits(g), bits(self.summed_in_order(pr, mbe, wg, P))), ("grads: not the order of P = %d" % P, row)
        pr.ctx.close()
        return g

    def summed_in_order(self, pr, mbe, wg, P, pi_h=None):
        """the gradient as P slots sum it (test_gpu_parity.py::test_beta_gradient_association_order_is_fixed): slot s
        adds edges s, s + P, ...; sum_partials8_kernel's row-lane r adds slots r, r + 128, ..., then a halving tree
        (sum_partials_kernel, K % 4 != 0: 16 row-lanes)"""
        pi_h = pr.pi_h if pi_h is None else pi_h
        terms = np.stack([self.orc.beta_grads(pr.p_orc, pr.theta_h, pr.beta_h, pi_h.reshape(-1), pr.oset, mbe[i:i + 1],
                                              wg, 1, order=0) for i in range(mbe.size)]).astype(np.float32)
        rows = np.zeros((P, terms.shape[1]), dtype=np.float32)
        for e in range(mbe.size):
            rows[e % P] = rows[e % P] + terms[e]
        R = 128 if pr.K % 4 == 0 else 16
        lanes = np.zeros((R, terms.shape[1]), dtype=np.float32)
        for p in range(P):
            lanes[p % R] = lanes[p % R] + rows[p]
        half = R // 2
        while half > 0:
            lanes[:half] = lanes[:half] + lanes[half:2 * half]
            half //= 2
        return lanes[0]

    # ---- update_pi + gradient as one launch against update_pi then the gradient (bit for bit) and the oracle
    def fused(self, row, pi_nt=None):
        orc, hip, torch = self.orc, self.hip, self.torch
        N, K, n, n_edges, wg = row.shape
        m = n_edges + 1
        pr = self.problem(row, n_nodes=m, deg=4 if N > 10000 else 16)
        edges = orc.make_edge(np.full(n_edges, pr.nodes_h[0], dtype=np.uint32), pr.nodes_h[1:m]).astype(np.uint64)
        d_edges = pr.ctx.from_numpy(edges)
        phi = hip.PhiUpdater(pr.ctx, pr.beta, pr.pi, pr.phi_sum, pr.dset, m, (42, 43), wg, streaming_only=True)
        bu = hip.BetaUpdater(pr.ctx, pr.theta, pr.beta, pr.pi, pr.dset, (44, 45), wg)
        phi.count_calls = 1
        phi.update_phi(pr.nodes, pr.nb, m)
        pr.sync()
        seeds = orc.rng_init(m * wg, 42, 43)
        want = orc.update_phi(pr.p_orc, pr.beta_h, pr.pi_h.reshape(-1), pr.phi_sum_h, pr.oset, pr.nodes_h,
                              pr.nb_h.reshape(-1), 1, seeds, wg, 1, True)
        assert np.array_equal(bits(phi.phi_vec.cpu().numpy()[:m]), bits(want)), ("phi_vec", row)
        pi_h, phi_sum_h = pr.pi_h.copy(), pr.phi_sum_h.copy()
        orc.update_pi(pr.p_orc, pi_h.reshape(-1), phi_sum_h, want.reshape(-1), pr.nodes_h, wg, 1)
        exact = orc.beta_grads(pr.p_orc, pr.theta_h, pr.beta_h, pi_h.reshape(-1), pr.oset, edges, wg, 1, order=1)
        rows = np.unique(pr.nodes_h)
        results = []
        forms = [("separate", None)] if pi_nt is None else []
        forms += [("fused", v) for v in ([None] if pi_nt is None else pi_nt)]
        for form, nt in forms:
            pr.pi.load(pr.pi_h)
            pr.phi_sum.copy_(pr.ctx.from_numpy(pr.phi_sum_h))
            bu.count_calls = 1
            if nt is not None:
                pr.ctx.lib.ammsb_debug_beta_pi_nt(nt)
            try:
                if form == "separate":
                    phi.update_pi(pr.nodes, m)
                    g = bu.calculate_grads(d_edges, n_edges)
                else:
                    g = bu.update_pi_and_grads(phi, pr.nodes, d_edges, n_edges)
                torch.cuda.synchronize()
            finally:
                if nt is not None:
                    pr.ctx.lib.ammsb_debug_beta_pi_nt(-1)
            if form == "fused":
                check_names(pr.ctx, row, "fused")
            got_pi = pr.pi.host()[rows]
            assert np.array_equal(bits(got_pi), bits(pi_h[rows])), ("pi rows", form, nt, row)
            assert np.array_equal(bits(pr.phi_sum.cpu().numpy()[rows]), bits(phi_sum_h[rows])), ("phi_sum", form, nt, row)
            g = g.cpu().numpy().copy()
            err = np.abs(g.astype(np.float64) - exact).max() / np.abs(exact).max()
            assert err <= 1e-5, ("grads", form, nt, err, row)
            results.append(g)
            print("%s pi_nt=%s: %s, max rel err %.2e" % (form, nt, raw_names(pr.ctx), err), flush=True)
        for g in results[1:]:
            assert np.array_equal(bits(g), bits(results[0])), ("gradient differs between the forms", row)
        pr.ctx.close()

    # ---- perplexity: three calls, then two calculators on one context in turn (the folding form's ticket)
    def ppx(self, row):
        orc, hip = self.orc, self.hip
        N, K, _, cnt, wg = row.shape
        pr = self.problem(row, n_nodes=16)
        held, hset = None, None
        for c in range(cnt, cnt + 40):  # (the reference's cuckoo build can fail on small, structured key sets)
            try:
                held = pr.edges[:c]
                hset = orc.OracleSet(held)
                break
            except RuntimeError:
                continue
        assert hset is not None
        fake = orc.make_edge(pr.rng.integers(0, N, 600), pr.rng.integers(0, N, 600))
        he = np.concatenate([held, fake[~hset.has(fake)]]).astype(np.uint64)
        dh = hip.DeviceSet(pr.ctx, hset.slots, hset.num_bins, hset.prime_idx)
        calcs = [hip.PerplexityCalculator(pr.ctx, pr.beta, pr.pi, pr.ctx.from_numpy(he), dh, wg),
                 hip.PerplexityCalculator(pr.ctx, pr.beta, pr.pi, pr.ctx.from_numpy(he[: he.size * 2 // 3]), dh, wg)]
        edges = [he, he[: he.size * 2 // 3]]
        states = [np.zeros(e.size, dtype=np.float32) for e in edges]
        calls = [0, 0]
        for which in (0, 0, 0, 1, 0, 1, 1, 0):
            got = calcs[which]()
            pr.sync()
            calls[which] += 1
            check_names(pr.ctx, row, "ppx")
            sums, _ = orc.perplexity(pr.p_orc, pr.beta_h, pr.pi_h.reshape(-1), hset, edges[which], calls[which], wg, 1,
                                     states[which])
            assert np.array_equal(bits(calcs[which].ppx_per_edge.cpu().numpy()), bits(states[which])), ("state", which, row)
            l0, l1, c0, c1 = calcs[which].unpack(calcs[which].sums)
            assert (c0, c1) == (sums.link_cnt, sums.nonlink_cnt), ("counts", which, calls, row)
            assert abs(l0 - sums.link_ll) <= 1e-12 * abs(sums.link_ll), ("link ll", which, calls, row)
            assert abs(l1 - sums.nonlink_ll) <= 1e-12 * abs(sums.nonlink_ll), ("non-link ll", which, calls, row)
            want = -(sums.link_ll + sums.nonlink_ll) / (sums.link_cnt + sums.nonlink_cnt)
            assert abs(got - want) <= 1e-5 * abs(want), ("ppx", which, calls, row)
        pr.ctx.close()

    # ---- neighbour sampler: table, packed output and streams bit for bit, two calls
    def nbr(self, row):
        orc, hip, torch = self.orc, self.hip, self.torch
        N, _, n, nodes, wg = row.shape
        ctx = hip.Context(hip.make_params(N, 32, num_node_sample=n))
        nodes_h = np.random.default_rng(3).integers(0, N, size=nodes, dtype=np.uint32)
        smp = hip.NeighborSampler(ctx, nodes, (56, 57), wg)
        seeds = orc.rng_init(nodes * 2 * n, 56, 57)
        for _ in range(2):
            smp(nodes, ctx.from_numpy(nodes_h))
            torch.cuda.synchronize()
            check_names(ctx, row, "nbr")
            table, packed = orc.sample_neighbors(seeds, nodes_h, N, n, wg)
            assert np.array_equal(bits(smp.GetHash().cpu().numpy()), table), ("table", row)
            assert np.array_equal(bits(smp.GetData().cpu().numpy()), packed), ("packed", row)
            assert np.array_equal(smp.rand.host(), seeds), ("streams", row)
        ctx.close()

    # ---- the edges mode (division_edges.py): one update_phi (noise on) + update_pi per case, bit for bit
    def _edge_problem(self, row):
        N, K, n, nodes = edge_state_shape(row)
        pr = self.problem(row, n_nodes=nodes, deg=edge_deg(row))
        if N * K <= 1 << 20:  # the host tests build the same state without a device
            hs = de.host_state(self.orc, N, K, n, nodes, deg=edge_deg(row))
            for f in ("pi_h", "phi_sum_h", "beta_h", "nb_h", "nodes_h", "edges"):
                assert np.array_equal(getattr(hs, f), getattr(pr, f)), ("host_state differs from Problem", f)
        return pr

    def _upload(self, pr):
        pr.pi.load(pr.pi_h)
        pr.phi_sum.copy_(pr.ctx.from_numpy(pr.phi_sum_h))
        pr.beta.copy_(pr.ctx.from_numpy(pr.beta_h))
        pr.nb.copy_(pr.ctx.from_numpy(pr.nb_h))

    def phi_edges(self, row):
        orc, hip = self.orc, self.hip
        N, K, n, _, wg = row.shape
        nodes = edge_nodes(row)
        if any(k == "AMMSB_PHI_PERSIST" for k, _ in row.env):
            assert nodes > 32 * self.torch.cuda.get_device_properties(0).multi_processor_count, row
        pr = self._edge_problem(row)
        saved = de.Saved(pr)
        eps = pr.p_orc.epsilon
        upd = hip.PhiUpdater(pr.ctx, pr.beta, pr.pi, pr.phi_sum, pr.dset, nodes, (42, 43), wg,
                             streaming_only=row.flags == "streaming")
        seeds = orc.rng_init(nodes * wg, 42, 43)
        for case in de.CASES:
            saved.restore(pr)
            cls, tally = phi_case(pr, case, eps)
            flags = pr.oset.has(orc.make_edge(pr.nodes_h[:, None], pr.nb_h).reshape(-1)).reshape(pr.nb_h.shape)
            assert np.array_equal(flags, de.link_flags(pr)), ("link flags", case, row)
            self._upload(pr)
            upd.count_calls = 1
            upd.update_phi(pr.nodes, pr.nb, nodes)
            pr.sync()
            want = orc.update_phi(pr.p_orc, pr.beta_h, pr.pi_h.reshape(-1), pr.phi_sum_h, pr.oset, pr.nodes_h,
                                  pr.nb_h.reshape(-1), 1, seeds, wg, 1, True)
            got = upd.phi_vec.cpu().numpy()[:nodes]
            if not same_bits(got, want):
                bad = np.argwhere((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want)))
                raise AssertionError(("phi_vec", case, row, len(bad), bad[:5].tolist(),
                                      [(cls.fast[i].sum(), cls.slow[i].sum()) for i in np.unique(bad[:5, 0])]))
            assert np.array_equal(upd.rand.host(), seeds), ("streams", case, row)
            pi_h, phi_sum_h = pr.pi_h.copy(), pr.phi_sum_h.copy()
            orc.update_pi(pr.p_orc, pi_h.reshape(-1), phi_sum_h, want.reshape(-1), pr.nodes_h, wg, 1)
            upd.update_pi(pr.nodes, nodes)
            pr.sync()
            check_names(pr.ctx, row, case)
            finite = np.ones(N, dtype=bool)
            finite[pr.nodes_h[~np.isfinite(want).all(1)]] = False  # (where the oracle's phi_vec is finite)
            if N > 10000:
                keep = np.zeros(N, dtype=bool)
                keep[pr.nodes_h] = True
                finite &= keep
            rows = np.flatnonzero(finite)
            assert same_bits(pr.pi.host()[rows], pi_h[rows]), ("pi", case, row)
            assert same_bits(pr.phi_sum.cpu().numpy()[rows], phi_sum_h[rows]), ("phi_sum", case, row)
            print("  %s: fast %.3f slow %.3f undecided %.3f" % (case, tally["fast"], tally["slow"], tally["undecided"]), flush=True)
        pr.ctx.close()

    @contextlib.contextmanager
    def _slots(self):
        """AMMSB_BETA_SLOTS (read at every call) at the slot count the edge lists are laid out for"""
        old = os.environ.get("AMMSB_BETA_SLOTS")
        os.environ["AMMSB_BETA_SLOTS"] = str(de.BETA_SLOTS)
        try:
            yield
        finally:
            if old is None:
                del os.environ["AMMSB_BETA_SLOTS"]
            else:
                os.environ["AMMSB_BETA_SLOTS"] = old

    def grads_edges(self, row, refs, out=None):
        """gradient rows: trained / denormal / mixed pi, the node-strategy list, 64 slots; against summed_in_order bit for
        bit, and against the default form's gradient (refs) where the row keeps the slot count.  out: save, do not check."""
        orc, hip = self.orc, self.hip
        N, K, _, _, wg = row.shape
        pr = self._edge_problem(row)
        saved = de.Saved(pr)
        eps = pr.p_orc.epsilon
        for case in de.GRAD_CASES:
            saved.restore(pr)
            c = grad_case(orc, pr.p_orc, pr, case, eps, False, wg)
            mbe = c["edges"]
            assert np.array_equal(pr.oset.has(mbe), c["links"]), ("link flags", case, row)
            self._upload(pr)
            upd = hip.BetaUpdater(pr.ctx, pr.theta, pr.beta, pr.pi, pr.dset, (44, 45), wg)
            upd.count_calls += 1
            with self._slots():
                g = upd.calculate_grads(pr.ctx.from_numpy(mbe), mbe.size).cpu().numpy().copy()
            key = "%s_%s" % (ref_key(row), case)
            if out is not None:
                out[key] = g
                continue
            check_names(pr.ctx, row, case)
            want = self.summed_in_order(pr, mbe, wg, de.BETA_SLOTS)
            assert same_bits(g, want), ("grads: not the oracle's terms in the order of 64 slots", case, c["count"], row)
            if refs is not None and keeps_slots(row):
                assert same_bits(g, refs[key]), ("grads differ from the default form", case, row)
            print("  %s: %d edges %s" % (case, mbe.size, c["count"]), flush=True)
        pr.ctx.close()

    def fused_edges(self, row):
        orc, hip, torch = self.orc, self.hip, self.torch
        N, K, n, _, wg = row.shape
        pr = self._edge_problem(row)
        saved = de.Saved(pr)
        eps = pr.p_orc.epsilon
        phi = hip.PhiUpdater(pr.ctx, pr.beta, pr.pi, pr.phi_sum, pr.dset, de.MAX_EDGES + 1, (42, 43), wg, streaming_only=True)
        bu = hip.BetaUpdater(pr.ctx, pr.theta, pr.beta, pr.pi, pr.dset, (44, 45), wg)
        for case in de.GRAD_CASES:
            saved.restore(pr)
            c = grad_case(orc, pr.p_orc, pr, case, eps, True, wg)
            edges, nodes_h = c["edges"], c["nodes"]
            m = nodes_h.size
            assert np.array_equal(pr.oset.has(edges), c["links"]), ("link flags", case, row)
            d_edges, d_nodes = pr.ctx.from_numpy(edges), pr.ctx.from_numpy(nodes_h)
            phi.phi_vec[:m].copy_(pr.ctx.from_numpy(c["phi_vec"]))
            want = self.summed_in_order(pr, edges, wg, de.BETA_SLOTS, pi_h=c["pi"])
            rows = np.unique(nodes_h)
            for form in ("separate", "fused"):
                self._upload(pr)
                bu.count_calls = 1
                with self._slots():
                    if form == "separate":
                        phi.update_pi(d_nodes, m)
                        g = bu.calculate_grads(d_edges, edges.size)
                    else:
                        g = bu.update_pi_and_grads(phi, d_nodes, d_edges, edges.size)
                    torch.cuda.synchronize()
                if form == "fused":
                    check_names(pr.ctx, row, case)
                assert same_bits(pr.pi.host()[rows], c["pi"][rows]), ("pi rows", form, case, row)
                assert same_bits(pr.phi_sum.cpu().numpy()[rows], c["phi_sum"][rows]), ("phi_sum", form, case, row)
                assert same_bits(g.cpu().numpy(), want), ("grads", form, case, c["count"], row)
            print("  %s: %d edges %s" % (case, edges.size, c["count"]), flush=True)
        pr.ctx.close()

    def run_edges(self, row, refs):
        with self._phi_forms(row):
            if row.op == "phi":
                self.phi_edges(row)
            elif row.op == "grads":
                self.grads_edges(row, refs)
            elif row.op == "fused":
                self.fused_edges(row)

    @contextlib.contextmanager
    def _phi_forms(self, row):
        """the row's ammsb_debug_phi_forms switch, reset afterwards"""
        phi_forms = row.debug.get("phi_forms")
        lib = None
        if phi_forms is not None:
            from mcmc_ammsb_gpu_amd import _capi
            lib = _capi.load()
            lib.ammsb_debug_phi_forms(*phi_forms)
        try:
            yield
        finally:
            if lib is not None:
                lib.ammsb_debug_phi_forms(-1, -1, -1)

    def run(self, row, refs):
        with self._phi_forms(row):
            if row.op == "phi":
                self.phi(row)
            elif row.op == "grads":
                self.grads(row, refs.get(ref_key(row)) if refs is not None else None)
            elif row.op == "fused":
                self.fused(row)
            elif row.op == "ppx":
                self.ppx(row)
            elif row.op == "nbr":
                self.nbr(row)
            else:
                raise ValueError(row.op)


def main():
    index = int(sys.argv[1])
    env, rows = kf.groups()[index]
    for k, v in env:
        assert os.environ.get(k) == v, "the caller sets the group's environment: %s=%s" % (k, v)
    r = Runner()
    from mcmc_ammsb_gpu_amd import _capi
    lib = _capi.load()
    lib.ammsb_debug_phi_forms.argtypes = [C.c_int, C.c_int, C.c_int]
    lib.ammsb_debug_beta_pi_nt.argtypes = [C.c_int]
    if len(sys.argv) > 2 and sys.argv[2] == "edge-refs":
        assert env == ()
        out = {}
        for e, others in kf.groups()[1:]:
            for _, row in others:
                if row.op == "grads" and keeps_slots(row) and "%s_%s" % (ref_key(row), de.GRAD_CASES[0]) not in out:
                    r.grads_edges(row._replace(kernel={}), None, out)
        np.savez(sys.argv[3], **out)
        print("group ok", flush=True)
        return
    if len(sys.argv) > 2 and sys.argv[2] == "edges":
        first, last = (int(sys.argv[3]), int(sys.argv[4])) if len(sys.argv) > 4 else (0, len(kf.ROWS))
        refs = dict(np.load(sys.argv[5])) if len(sys.argv) > 5 else None
        for i, row in rows:
            if first <= i <= last and row.op in ("phi", "grads", "fused"):
                r.run_edges(row, refs)
                print("edge ok %d" % i, flush=True)
        print("group ok", flush=True)
        return
    refs = None
    if len(sys.argv) > 2 and sys.argv[2] != "-":
        refs = dict(np.load(sys.argv[2]))
    for i, row in rows:
        r.run(row, refs)
        print("row ok %d" % i, flush=True)
    if len(sys.argv) > 3:
        out = {}
        for e, others in kf.groups():
            if e == env:
                continue
            for _, row in others:
                if row.op == "grads" and keeps_slots(row) and ref_key(row) not in out:
                    out[ref_key(row)] = r.gradient(row)
        np.savez(sys.argv[3], **out)
    print("group ok", flush=True)


if __name__ == "__main__":
    main()
