#!/usr/bin/env python3
"""Same-process A/B of link prediction at C3's shape (N = 10^6, K = 1024, one block; rows as fitted rows look: gamma(1/K)
draws, floored and normalised like update_pi leaves them), the contenders alternating in one process:
  top    ammsb_linkpred_top at T = 10 for Q in {1, 32, 256, 1024}, without and with two exclusion sets, against the torch
         statement a user had before: scores = (pi[q] * w) @ pi.T + eps, the query masked, torch.topk(scores, 10).
  pairs  ammsb_linkpred_pairs over 163 148 pairs against (pi[u] * pi[v] * w).sum(1) + eps, and against the perplexity
         kernel over the same number of edges (the same 8K + 8 bytes per pair).
Each as ms (median and min of the rounds, device events).  For top: FLOP/s = 2 Q N K / time and its share of the f32
matrix-core rate at the shader clock held under load (64 FLOP / clk / SIMD x 1024 SIMDs x the clock ammsb_clock_probe
reads while `top` runs); for Q <= 32 also bytes of pi / time against 8 TB/s.  Untimed rounds run first until a second
has passed and five consecutive rounds of the first case agree within 3 % (at most --settle-s seconds).
  python tools/linkpred_ab.py [--rows N] [--cols K] [--rounds R] [--out FILE.json]
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
PAIRS = 163_148


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--settle-s", type=float, default=8.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("linkpred_ab.py needs a HIP device: a timing taken anywhere else says nothing")
    import ammsb_pkg
    ammsb_pkg.load()
    from mcmc_ammsb_gpu_amd import ops
    N, K, T = args.rows, args.cols, 10
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
    w = beta[1::2] - eps
    rng = np.random.default_rng(2)

    def keys(n):
        a, b = rng.integers(0, N, n).astype(np.uint64), rng.integers(0, N, n).astype(np.uint64)
        keep = a != b
        a, b = a[keep], b[keep]
        return np.unique((np.minimum(a, b) << np.uint64(32)) | np.maximum(a, b))
    training = ops.DeviceSet.build_on_device(ctx, keys(4_000_000))
    heldout = ops.DeviceSet.build_on_device(ctx, keys(PAIRS))
    lp = ops.LinkPredictor(ctx)
    lp.reserve(max(lp.workspace_bytes(q, T, N, K) for q in (1, 32, 256, 1024)))
    queries = {q: ctx.from_numpy(rng.integers(0, N, q).astype(np.uint32)) for q in (1, 32, 256, 1024)}
    qlong = {q: t.long() for q, t in queries.items()}
    rows = {q: torch.arange(q, device=dev) for q in queries}
    pair_keys = keys(PAIRS + 2000)[:PAIRS]
    edges = ctx.from_numpy(pair_keys)
    pu, pv = torch.from_numpy((pair_keys >> np.uint64(32)).astype(np.int64)).to(dev), \
        torch.from_numpy((pair_keys & np.uint64(0xFFFFFFFF)).astype(np.int64)).to(dev)
    ppx = ops.PerplexityCalculator(ctx, beta, pi, edges, heldout)
    forms = {}

    def ours(q, sets):
        def f():
            lp.top(pi, beta, eps, queries[q], T, exclude=sets)
            forms["top Q=%d" % q] = lp.kernel_name()
        return f

    def torch_top(q):
        def f():
            s = (blk[qlong[q]] * w) @ blk.T + eps
            s[rows[q], qlong[q]] = -1.0
            torch.topk(s, T, dim=1)
        return f

    def our_pairs():
        lp.pairs(pi, beta, eps, edges)
        forms["pairs"] = lp.kernel_name()

    def ppx_kernel():
        ppx.count_calls += 1   # 1-based, as Learner._perplexity counts
        ppx.partial()

    def torch_pairs():
        (blk[pu] * blk[pv] * w).sum(1) + eps
    cases = []
    for q in (1, 32, 256, 1024):
        cases += [("top Q=%d" % q, ours(q, ()), q), ("top Q=%d, two sets" % q, ours(q, (training, heldout)), q),
                  ("torch Q=%d" % q, torch_top(q), q)]
    cases += [("pairs", our_pairs, 0), ("torch pairs", torch_pairs, 0), ("perplexity kernel", ppx_kernel, 0)]

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
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
    # the shader clock while `top` at Q = 1024 runs
    probe = ops.ClockProbe(ctx)
    ours(1024, ())()
    probe.launch()
    ours(1024, ())()
    clock = probe.read()
    torch.cuda.synchronize()
    mhz = clock["mhz"] or 0.0
    peak_flops = 64.0 * 1024 * mhz * 1e6
    rec = {"tool": "linkpred_ab", "device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "T": T, "pairs": PAIRS,
           "rounds": args.rounds, "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)},
           "kernel_forms": forms, "clock_under_load": clock, "f32_mfma_peak_flops": peak_flops,
           "peak_bytes_per_s": PEAK_BYTES, "cases": {}}
    for name, _, q in cases:
        med = statistics.median(times[name])
        c = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4), "ms_max": round(max(times[name]), 4)}
        if q:
            c["TFLOPs_median"] = round(2.0 * q * N * K / (med * 1e-3) / 1e12, 2)
            if peak_flops:
                c["share_of_f32_mfma_rate"] = round(2.0 * q * N * K / (med * 1e-3) / peak_flops, 3)
            if q <= 32:
                c["TBps_median"] = round(4.0 * N * K / (med * 1e-3) / 1e12, 3)
        else:
            c["TBps_median"] = round(PAIRS * (8.0 * K + 8) / (med * 1e-3) / 1e12, 3)
        rec["cases"][name] = c
    c = rec["cases"]
    rec["torch_over_top"] = {str(q): round(c["torch Q=%d" % q]["ms_median"] / c["top Q=%d" % q]["ms_median"], 2)
                             for q in (1, 32, 256, 1024)}
    rec["exclusion_cost"] = {str(q): round(c["top Q=%d, two sets" % q]["ms_median"] / c["top Q=%d" % q]["ms_median"], 3)
                             for q in (1, 32, 256, 1024)}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
