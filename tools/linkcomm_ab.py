#!/usr/bin/env python3
"""Same-process A/B of the link-community read-out at C3's shape (N = 10^6, K = 1024, one block; rows as fitted rows
look: gamma(1/K) draws, floored and normalised like update_pi leaves them; 4 M random training-like edges), the
contenders alternating in one process:
  ours   ammsb_linkcomm_edges at T in {1, 4, 16} with sizes, and the sizes-only pass;
  torch  the statement a user had before: (pi[a] * pi[b] * beta).topk(T) plus the bincount of slot 0, in slabs of
         --torch-slab edges so that the n x K products fit;
  pairs  ammsb_linkpred_pairs over the same edges: the two-row gather alone, hence the floor for this kernel's traffic.
Each as ms (median and min of the rounds, device events) and as bytes / time against 8 TB/s, bytes = the two rows and
the key of every edge (8 K + 8) plus what the case writes.  Untimed rounds run first until a second has passed and five
consecutive rounds of the first case agree within 3 % (at most --settle-s seconds).
  python tools/linkcomm_ab.py [--rows N] [--cols K] [--edges E] [--rounds R] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_BYTES = 8e12
TOPS = (1, 4, 16)


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
        raise SystemExit("linkcomm_ab.py needs a HIP device: a timing taken anywhere else says nothing")
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
    b_odd = beta[1::2].contiguous()
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, N, args.edges).astype(np.uint64), rng.integers(0, N, args.edges).astype(np.uint64)
    keep = a != b
    a, b = a[keep], b[keep]
    keys = np.unique((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b))   # ascending, as TrainingLinks()
    E = int(keys.size)
    edges = ctx.from_numpy(keys)
    pu = torch.from_numpy((keys >> np.uint64(32)).astype(np.int64)).to(dev)
    pv = torch.from_numpy((keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).to(dev)
    lc, lp = ops.LinkCommunities(ctx), ops.LinkPredictor(ctx)
    sizes = ctx.zeros((K + 1,), torch.int64)
    forms = {}

    def ours(T):
        def f():
            sizes.zero_()
            lc.edges(pi, beta, eps, edges, T, sizes=sizes)
            forms["ours T=%d" % T] = lc.kernel_name()
        return f

    def ours_sizes():
        sizes.zero_()
        lc.sizes(pi, beta, eps, edges, out=sizes)

    def torch_top(T):
        def f():
            count = torch.zeros((K,), dtype=torch.int64, device=dev)
            for lo in range(0, E, args.torch_slab):
                t = blk[pu[lo:lo + args.torch_slab]] * blk[pv[lo:lo + args.torch_slab]] * b_odd
                _, ids = t.topk(T, dim=1)
                count += torch.bincount(ids[:, 0], minlength=K)
        return f

    def pairs():
        lp.pairs(pi, beta, eps, edges)
    cases = [("ours T=%d" % T, ours(T), 8 * T + 4) for T in TOPS] + [("ours sizes only", ours_sizes, 0)]
    cases += [("torch T=%d" % T, torch_top(T), 8 * T) for T in TOPS] + [("linkpred pairs", pairs, 4)]

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
    rec = {"tool": "linkcomm_ab", "device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "edges": E,
           "rounds": args.rounds, "torch_slab": args.torch_slab,
           "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)},
           "kernel_forms": forms, "peak_bytes_per_s": PEAK_BYTES, "cases": {}}
    for name, _, out_bytes in cases:
        med = statistics.median(times[name])
        nbytes = E * (8.0 * K + 8 + out_bytes)
        rec["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4),
                              "ms_max": round(max(times[name]), 4),
                              "TBps_median": round(nbytes / (med * 1e-3) / 1e12, 3),
                              "share_of_8TBps": round(nbytes / (med * 1e-3) / PEAK_BYTES, 3)}
    c = rec["cases"]
    rec["torch_over_ours"] = {str(T): round(c["torch T=%d" % T]["ms_median"] / c["ours T=%d" % T]["ms_median"], 2) for T in TOPS}
    rec["ours_over_pairs"] = {str(T): round(c["ours T=%d" % T]["ms_median"] / c["linkpred pairs"]["ms_median"], 2) for T in TOPS}
    rec["ours_T_over_T1"] = {str(T): round(c["ours T=%d" % T]["ms_median"] / c["ours T=1"]["ms_median"], 2) for T in TOPS}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
