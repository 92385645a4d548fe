#!/usr/bin/env python3
"""Same-process A/B of the pair pass of the overlapping NMI (include/ammsb_nmi.h) at K = 1024 and G in {5 000, 10^5}
on a synthetic overlap matrix with the sparsity of a SNAP cover against a fitted model: N = 10^6 nodes, community sizes
t_g drawn log-uniform from 3 to 10^4, each community's members spread over a few detected communities (about one
non-zero overlap per four members, at most K / 4), d_k around 2 N / K with a few communities above N / 2 (their
zero-overlap pairs cannot be skipped).  The contenders alternate in one process:
  ours      ammsb_nmi_begin + ammsb_nmi_accumulate over the whole matrix (nmi_fast), and over a copy whose base is 4
            bytes past a 16-byte boundary (nmi_generic);
  torch     the same statement in torch float64, in slabs of --torch-slab rows: the four cells, their h-terms, the
            qualifying mask, amin over both axes;
  update_pi ammsb_update_pi over 10^5 rows of a pi of K columns (8 K bytes a row): the project's own streaming ruler.
Each as ms (median and min of the rounds, device events) and, for ours, as 4 G K bytes / time against update_pi's rate
in the same run.  Untimed rounds run first until a second has passed and five consecutive rounds of the first case
agree within 3 % (at most --settle-s seconds).  Every GPU step runs under a time limit of its own (--step-limit-s): a
step that does not come back ends the process with status 124 and starts nothing more.
  python tools/nmi_ab.py [--cols K] [--rounds R] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--truths", type=int, nargs="+", default=[5_000, 100_000])
    ap.add_argument("--torch-slab", type=int, default=4096)
    ap.add_argument("--pi-rows", type=int, default=100_000)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--settle-s", type=float, default=8.0)
    ap.add_argument("--step-limit-s", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("nmi_ab.py needs a HIP device: a timing taken anywhere else says nothing")
    import ammsb_pkg
    ammsb_pkg.load()
    from mcmc_ammsb_gpu_amd import _nmi, ops
    N, K = args.nodes, args.cols
    ctx = ops.Context(ops.make_params(args.pi_rows, K, E=args.pi_rows))
    dev = ctx.device
    nm = ops.CoverNMI(ctx)
    lib = _nmi.load()
    rng = np.random.default_rng(2)
    d = np.maximum(1, rng.normal(2.0 * N / K, 0.3 * N / K, K)).astype(np.int64)
    d[rng.choice(K, 3, replace=False)] = rng.integers(N // 2 + 1, N, 3)
    d_dev = ctx.from_numpy(d)
    inf = float("inf")
    data, forms = {}, {}
    for G in args.truths:
        t = np.exp(rng.uniform(np.log(3.0), np.log(1e4), G)).round().astype(np.int64)
        ov = np.zeros((G, K), dtype=np.uint32)
        nnz = 0
        for g in range(G):
            n = int(min(K // 4, max(1, t[g] // 4)))
            cols = rng.choice(K, n, replace=False)
            ov[g, cols] = np.minimum(np.minimum(rng.integers(1, max(2, 2 * t[g] // n + 1), n), t[g]), d[cols])
            nnz += n
        flat = ctx.from_numpy(ov.reshape(-1))
        shifted = ctx.empty((G * K + 1,), torch.int32)
        shifted[1:].copy_(flat)
        data[G] = dict(t=ctx.from_numpy(t.astype(np.uint32)), t64=torch.from_numpy(t).to(dev), ov=flat.reshape(G, K),
                       shifted=shifted, density=nnz / float(G * K))
        del ov
    ptr = lambda x: C.c_void_p(x.data_ptr())   # noqa: E731

    def ours(G, misaligned):
        c = data[G]

        def f():
            st = nm.begin(N, c["t"], d_dev)
            if misaligned:   # (ops.CoverNMI takes tensors, whose storage is aligned: the raw call)
                _nmi.check(lib.ammsb_nmi_accumulate(C.c_void_p(c["shifted"].data_ptr() + 4), 0, G, N, ptr(c["t"]), G,
                                                    ptr(d_dev), K, ptr(st.H_truth), ptr(st.H_detected), ptr(st.c_truth),
                                                    ptr(st.c_detected), C.c_void_p(torch.cuda.current_stream().cuda_stream)))
            else:
                nm.accumulate(st, c["ov"], 0)
            forms[nm.kernel_name()] = True
        return f

    def h(x):
        p = x.clamp_min(1).to(torch.float64) / float(N)
        return torch.where(x > 0, -(p * torch.log2(p)), torch.zeros((), dtype=torch.float64, device=dev))

    def torch_way(G):
        c = data[G]
        dd = d_dev

        def f():
            HY = torch.where(dd >= N, 0.0, h(dd) + h((N - dd).clamp_min(0)))
            cy = torch.full((K,), inf, dtype=torch.float64, device=dev)
            for g0 in range(0, G, args.torch_slab):
                o = c["ov"][g0:g0 + args.torch_slab].to(torch.int64)
                t = c["t64"][g0:g0 + args.torch_slab]
                HX = torch.where(t >= N, 0.0, h(t) + h((N - t).clamp_min(0)))
                n10, n01 = t[:, None] - o, dd[None, :] - o
                n00 = N - t[:, None] - dd[None, :] + o
                lhs, rhs = h(o) + h(n00.clamp_min(0)), h(n01.clamp_min(0)) + h(n10.clamp_min(0))
                q = (n00 >= 0) & (n10 >= 0) & (n01 >= 0) & (lhs >= rhs)
                J = lhs + rhs
                torch.where(q, (J - HY[None, :]).clamp_min(0), inf).amin(1)
                cy = torch.minimum(cy, torch.where(q, (J - HX[:, None]).clamp_min(0), inf).amin(0))
        return f

    R = args.pi_rows
    pi2 = ops.RowPartitionedMatrix(ctx, R, K)
    phi_vec = torch.rand((R, K), device=dev, dtype=torch.float32)
    phi_sum = ctx.zeros((R,), torch.float32)
    nodes = torch.arange(R, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def update_pi():
        ctx.check(ctx.lib.ammsb_update_pi(ctx.handle, C.byref(pi2.desc), C.c_void_p(phi_sum.data_ptr()),
                                          C.c_void_p(phi_vec.data_ptr()), C.c_void_p(nodes.data_ptr()), R, 64, stream))
    cases = []
    for G in args.truths:
        cases += [("ours fast G=%d" % G, ours(G, False), 4.0 * G * K), ("ours generic G=%d" % G, ours(G, True), 4.0 * G * K),
                  ("torch G=%d" % G, torch_way(G), 4.0 * G * K)]
    cases += [("update_pi %d rows" % R, update_pi, 8.0 * R * K)]

    def timed(name, f):
        def late():
            sys.stderr.write("nmi_ab: %r did not come back within %g s\n" % (name, args.step_limit_s))
            sys.stderr.flush()
            os._exit(124)
        guard = threading.Timer(args.step_limit_s, late)
        guard.daemon = True
        guard.start()
        try:
            x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            x.record()
            f()
            y.record()
            y.synchronize()
            return x.elapsed_time(y)
        finally:
            guard.cancel()
    t0, recent, settle_rounds = time.perf_counter(), [], 0
    while True:
        for name, f, _ in cases:
            timed(name, f)
        recent = (recent + [timed(cases[0][0], cases[0][1])])[-5:]
        settle_rounds += 1
        el = time.perf_counter() - t0
        if (el >= 1.0 and len(recent) == 5 and max(recent) <= 1.03 * min(recent)) or el >= args.settle_s:
            break
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, f, _ in cases:
            times[name].append(timed(name, f))
    rec = {"tool": "nmi_ab", "device": torch.cuda.get_device_name(0), "nodes": N, "cols": K, "rounds": args.rounds,
           "torch_slab": args.torch_slab, "truths": {str(G): {"nonzero_share": round(data[G]["density"], 5)} for G in args.truths},
           "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)},
           "kernel_forms": sorted(forms), "cases": {}}
    for name, _, nbytes in cases:
        med = statistics.median(times[name])
        rec["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4),
                              "ms_max": round(max(times[name]), 4), "bytes": nbytes,
                              "TBps_median": round(nbytes / (med * 1e-3) / 1e12, 4)}
    c = rec["cases"]
    ruler = c["update_pi %d rows" % R]["TBps_median"]
    rec["torch_over_ours_fast"] = {str(G): round(c["torch G=%d" % G]["ms_median"] / c["ours fast G=%d" % G]["ms_median"], 2)
                                   for G in args.truths}
    rec["fast_rate_over_update_pi_rate"] = {str(G): round(c["ours fast G=%d" % G]["TBps_median"] / ruler, 4) for G in args.truths}
    rec["generic_over_fast"] = {str(G): round(c["ours generic G=%d" % G]["ms_median"] / c["ours fast G=%d" % G]["ms_median"], 2)
                                for G in args.truths}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
