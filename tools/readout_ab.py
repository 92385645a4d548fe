#!/usr/bin/env python3
"""Same-process A/B of the pi read-out at C3's shape (N = 10^6, K = 1024, one block; rows as fitted rows look: gamma(1/K)
draws, floored and normalised like update_pi leaves them), alternating in one process:
  (a) ammsb_readout_top with sizes: T = 4 thr = 0, T = 4 thr = 0.05, T = 16 thr = 0 (the worst case by construction)
  (b) what a user had before: torch.topk(pi, T) plus (pi >= thr).sum(0)
  (c) ammsb_update_pi over all N rows of a pi of the same shape: the project's own streaming yardstick
Each as ms (median and min of the rounds, device events) and as bytes-moved / time against 8 TB/s.  (a) reads pi once
(4 N K bytes), (b) reads it twice, (c) reads phi_vec and writes pi (8 N K bytes).  Untimed rounds run first until a
second has passed and five consecutive rounds of (a) agree within 3 % (at most --settle-s seconds).
  python tools/readout_ab.py [--rows N] [--cols K] [--rounds R] [--out FILE.json]
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
PEAK = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=30)
    ap.add_argument("--settle-s", type=float, default=8.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("readout_ab.py needs a HIP device: a timing taken anywhere else says nothing")
    import ammsb_pkg
    ammsb_pkg.load()
    from mcmc_ammsb_gpu_amd import ops
    N, K = args.rows, args.cols
    ctx = ops.Context(ops.make_params(N, K, E=N))
    dev = ctx.device
    pi = ops.RowPartitionedMatrix(ctx, N, K)
    blk = pi.blocks[0]
    torch.manual_seed(1)
    gam = torch.distributions.Gamma(torch.tensor(1.0 / K, device=dev), torch.tensor(1.0, device=dev))
    for lo in range(0, N, 65536):
        g = gam.sample((min(65536, N - lo), K)).clamp_min_(1e-24)
        blk[lo:lo + 65536].copy_(g / g.sum(1, keepdim=True))
    pi2 = ops.RowPartitionedMatrix(ctx, N, K)
    phi_vec = blk.clone()
    phi_sum = ctx.zeros((N,), torch.float32)
    nodes = torch.arange(N, dtype=torch.int32, device=dev)
    ro = ops.CommunityReadout(ctx)
    sizes = ctx.zeros((K,), torch.int64)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def readout(T, thr):
        def f():
            sizes.zero_()
            ro.top(pi, T, thr, sizes=sizes)
        return f

    def torch_way(T, thr):
        def f():
            torch.topk(blk, T, dim=1)
            (blk >= thr).sum(0)
        return f

    def update_pi():
        ctx.check(ctx.lib.ammsb_update_pi(ctx.handle, C.byref(pi2.desc), C.c_void_p(phi_sum.data_ptr()),
                                          C.c_void_p(phi_vec.data_ptr()), C.c_void_p(nodes.data_ptr()), N, 64, stream))
    row_bytes = 4.0 * N * K
    cases = [("readout T=4 thr=0", readout(4, 0.0), row_bytes), ("readout T=4 thr=0.05", readout(4, 0.05), row_bytes),
             ("readout T=16 thr=0", readout(16, 0.0), row_bytes), ("torch topk+sum T=4 thr=0", torch_way(4, 0.0), 2 * row_bytes),
             ("torch topk+sum T=4 thr=0.05", torch_way(4, 0.05), 2 * row_bytes),
             ("torch topk+sum T=16 thr=0", torch_way(16, 0.0), 2 * row_bytes), ("update_pi all rows", update_pi, 2 * row_bytes)]

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        f()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)
    # settle: untimed alternating rounds
    t0, recent, settle_rounds = time.perf_counter(), [], 0
    while True:
        for _, f, _ in cases:
            ms = timed(f)
        recent = (recent + [timed(cases[0][1])])[-5:]
        settle_rounds += 1
        el = time.perf_counter() - t0
        stable = len(recent) == 5 and max(recent) <= 1.03 * min(recent)
        if (el >= 1.0 and stable) or el >= args.settle_s:
            break
    kernel = ro.kernel_name()
    times = {name: [] for name, _, _ in cases}
    for _ in range(args.rounds):
        for name, f, _ in cases:
            times[name].append(timed(f))
    rec = {"tool": "readout_ab", "device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "rounds": args.rounds,
           "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)}, "readout_kernel": kernel,
           "peak_bytes_per_s": PEAK, "cases": {}}
    for name, _, nbytes in cases:
        med, best = statistics.median(times[name]), min(times[name])
        rec["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(best, 4), "ms_max": round(max(times[name]), 4),
                              "bytes": nbytes, "TBps_median": round(nbytes / (med * 1e-3) / 1e12, 3),
                              "share_of_8TBps": round(nbytes / (med * 1e-3) / PEAK, 3)}
    c = rec["cases"]
    rec["readout_T4_vs_torch"] = {thr: round(c["torch topk+sum T=4 thr=%s" % thr]["ms_median"] /
                                             c["readout T=4 thr=%s" % thr]["ms_median"], 2) for thr in ("0", "0.05")}
    rec["readout_T4_thr0_vs_update_pi_rate"] = round(c["readout T=4 thr=0"]["TBps_median"] /
                                                     c["update_pi all rows"]["TBps_median"], 3)
    line = json.dumps(rec)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
