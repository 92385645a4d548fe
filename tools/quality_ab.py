#!/usr/bin/env python3
"""Same-process A/B of the community-quality read-out at C3's shape (N = 10^6, K = 1024, one block; rows as fitted rows
look: gamma(1/K) draws, floored and normalised like update_pi leaves them; 4 M random training-like edges), at
thr in {0.05, 0.01}, the contenders alternating in one process:
  ours      ammsb_quality_mask (4 K + K / 8 bytes per row) and ammsb_quality_edges with counts (K / 4 + 8 bytes per
            edge), timed apart and together;
  torch     the statement a user had before: M = pi >= thr; (M[a] & M[b]).sum(0), (M[a] ^ M[b]).sum(0) and the uncovered
            count, in slabs of --torch-slab edges so that the n x K booleans fit;
  linkcomm  ammsb_linkcomm_edges, sizes only, over the same edges: the two-row gather over pi (8 K + 8 bytes per edge)
            that the membership bits exist to avoid, hence the floor of that way;
  update_pi ammsb_update_pi over all N rows of a pi of the same shape (8 N K bytes): the project's own streaming ruler
            for the mask pass.
Each as ms (median and min of the rounds, device events) and as bytes / time against 8 TB/s.  Untimed rounds run first
until a second has passed and five consecutive rounds of the first case agree within 3 % (at most --settle-s seconds).
  python tools/quality_ab.py [--rows N] [--cols K] [--edges E] [--rounds R] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES = 8e12
THRS = (0.05, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--edges", type=int, default=4_000_000)
    ap.add_argument("--torch-slab", type=int, default=262_144)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--settle-s", type=float, default=8.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("quality_ab.py needs a HIP device: a timing taken anywhere else says nothing")
    import ammsb_pkg
    ammsb_pkg.load()
    from mcmc_ammsb_gpu_amd import ops
    N, K = args.rows, args.cols
    eps = float(np.float32(1e-7))
    ctx = ops.Context(ops.make_params(N, K, E=N))
    dev = ctx.device
    pi = ops.RowPartitionedMatrix(ctx, N, K)
    blk = pi.blocks[0]
    torch.manual_seed(1)
    gam = torch.distributions.Gamma(torch.tensor(1.0 / K, device=dev), torch.tensor(1.0, device=dev))
    for lo in range(0, N, 65536):
        g = gam.sample((min(65536, N - lo), K)).clamp_min_(1e-24)
        blk[lo:lo + 65536].copy_(g / g.sum(1, keepdim=True))
    beta = torch.rand((2 * K,), device=dev)
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, N, args.edges).astype(np.uint64), rng.integers(0, N, args.edges).astype(np.uint64)
    keep = a != b
    a, b = a[keep], b[keep]
    keys = np.unique((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b))   # ascending, as TrainingLinks()
    E = int(keys.size)
    edges = ctx.from_numpy(keys)
    pu = torch.from_numpy((keys >> np.uint64(32)).astype(np.int64)).to(dev)
    pv = torch.from_numpy((keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).to(dev)
    cq, lc = ops.CommunityQuality(ctx), ops.LinkCommunities(ctx)
    sizes = ctx.zeros((K + 1,), torch.int64)
    pi2 = ops.RowPartitionedMatrix(ctx, N, K)
    phi_vec = blk.clone()
    phi_sum = ctx.zeros((N,), torch.float32)
    nodes = torch.arange(N, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    masks = {thr: cq.mask(pi, thr) for thr in THRS}
    forms = {"mask": cq.kernel_name()}
    memberships = {str(thr): round(float((blk[:65536] >= thr).sum().item()) / min(N, 65536), 2) for thr in THRS}   # per node, from a sample

    def ours_mask(thr):
        return lambda: cq.mask(pi, thr)

    def ours_edges(thr):
        def f():
            cq.edges(masks[thr], N, K, edges)
            forms["edges"] = cq.kernel_name()
        return f

    def ours_both(thr):
        return lambda: cq.edges(cq.mask(pi, thr), N, K, edges)

    def torch_way(thr):
        def f():
            internal = torch.zeros((K,), dtype=torch.int64, device=dev)
            boundary = torch.zeros((K,), dtype=torch.int64, device=dev)
            uncovered = torch.zeros((), dtype=torch.int64, device=dev)
            for lo in range(0, E, args.torch_slab):
                ma, mb = blk[pu[lo:lo + args.torch_slab]] >= thr, blk[pv[lo:lo + args.torch_slab]] >= thr
                both = ma & mb
                internal.add_(both.sum(0))
                boundary.add_((ma ^ mb).sum(0))
                uncovered.add_((~both.any(1)).sum())
        return f

    def linkcomm_sizes():
        sizes.zero_()
        lc.sizes(pi, beta, eps, edges, out=sizes)

    def update_pi():
        ctx.check(ctx.lib.ammsb_update_pi(ctx.handle, C.byref(pi2.desc), C.c_void_p(phi_sum.data_ptr()),
                                          C.c_void_p(phi_vec.data_ptr()), C.c_void_p(nodes.data_ptr()), N, 64, stream))
    W = (K + 63) // 64
    mask_bytes, edge_bytes, gather_bytes = N * (4.0 * K + 8 * W), E * (16.0 * W + 8), E * (8.0 * K + 8)
    cases = []
    for thr in THRS:
        cases += [("ours mask thr=%g" % thr, ours_mask(thr), mask_bytes), ("ours edges thr=%g" % thr, ours_edges(thr), edge_bytes),
                  ("ours mask+edges thr=%g" % thr, ours_both(thr), mask_bytes + edge_bytes),
                  ("torch thr=%g" % thr, torch_way(thr), gather_bytes)]
    cases += [("linkcomm sizes only", linkcomm_sizes, gather_bytes), ("update_pi all rows", update_pi, 8.0 * N * K)]

    def timed(f):
        x, y = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        x.record()
        f()
        y.record()
        y.synchronize()
        return x.elapsed_time(y)
    t0, recent, settle_rounds = time.perf_counter(), [], 0
    while True:
        for _, f, _ in cases:
            timed(f)
        recent = (recent + [timed(cases[0][1])])[-5:]
        settle_rounds += 1
        el = time.perf_counter() - t0
        if (el >= 1.0 and len(recent) == 5 and max(recent) <= 1.03 * min(recent)) or el >= args.settle_s:
            break
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, f, _ in cases:
            times[name].append(timed(f))
    rec = {"tool": "quality_ab", "device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "edges": E,
           "rounds": args.rounds, "torch_slab": args.torch_slab, "memberships_per_node": memberships,
           "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)},
           "kernel_forms": forms, "peak_bytes_per_s": PEAK_BYTES, "cases": {}}
    for name, _, nbytes in cases:
        med = statistics.median(times[name])
        rec["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4),
                              "ms_max": round(max(times[name]), 4), "bytes": nbytes,
                              "TBps_median": round(nbytes / (med * 1e-3) / 1e12, 3),
                              "share_of_8TBps": round(nbytes / (med * 1e-3) / PEAK_BYTES, 3)}
    c = rec["cases"]
    ms = lambda name: c[name]["ms_median"]   # noqa: E731
    rec["torch_over_ours"] = {str(t): round(ms("torch thr=%g" % t) / ms("ours mask+edges thr=%g" % t), 2) for t in THRS}
    rec["linkcomm_over_ours"] = {str(t): round(ms("linkcomm sizes only") / ms("ours mask+edges thr=%g" % t), 2) for t in THRS}
    rec["linkcomm_over_ours_edges_alone"] = {str(t): round(ms("linkcomm sizes only") / ms("ours edges thr=%g" % t), 2) for t in THRS}
    rec["mask_rate_over_update_pi_rate"] = {str(t): round(c["ours mask thr=%g" % t]["TBps_median"] /
                                                          c["update_pi all rows"]["TBps_median"], 3) for t in THRS}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
