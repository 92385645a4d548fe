#!/usr/bin/env python3
"""What the chain spread costs per iteration beside the chain average: bench.py's workload (default C3: N = 10^6, K = 1024,
mini-batch 65536) on the eager loop with device sampling, in ONE process and on ONE learner, in alternating windows with
the average off, the average on (the mean alone) and the spread on (mean and variance).  Every step is timed by itself (two
events around Run(1)); the figure is the median over the non-link steps (a mini-batch of the configured size) of each kind
of window, so the three are compared under the same clocks and the same placement of pi.  Also timed: one full flush of
mean and variance, one fill of a Bound view and one Unsettled.  Needs a GPU.  Writes profiles/spread_ab.json.

    python tools/spread_ab.py [--workload C3] [--windows 4] [--steps 40] [--out profiles/spread_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--workload", default="C3")
    ap.add_argument("--windows", type=int, default=4, help="windows of each kind")
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spread_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from bench import WORKLOADS, pick_wg
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd.learner import Config, Learner
    if not torch.cuda.is_available():
        raise SystemExit("spread_ab.py needs a HIP device")
    N, K, m, n, deg, k_true = WORKLOADS[args.workload]
    ds = hostlib.Dataset.robust(N, hostlib.generate_graph(N, k_true, deg, seed=20260101), heldout_ratio=0.01, rand_seed=1)
    wg = pick_wg(K, 0, 16)
    lrn = Learner(Config.from_cli_defaults(K=K, mini_batch_size=m, num_node_sample=n, strategy="Node", phi_wg_size=wg,
                                           beta_wg_size=wg, ppx_wg_size=wg, device_sampling=True, graph_launch=False), ds)
    lrn.step_log = []
    lrn.Run(args.steps)   # clocks, code objects, the first mini-batches
    lrn.drain()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def window():
        """-> ms of every non-link step of one window"""
        out = []
        for _ in range(args.steps):
            ev[0].record()
            lrn.Run(1)
            ev[1].record()
            ev[1].synchronize()
            if lrn.step_log[-1][0] == m:
                out.append(ev[0].elapsed_time(ev[1]))
        return out

    off, mean_on, spread_on = [], [], []
    for _ in range(args.windows):
        lrn.StopAverage()
        off += window()
        lrn.StartAverage()
        lrn.Run(2)        # the first averaged steps copy rows (no read of the mean): not what a long run pays
        mean_on += window()
        lrn.StartAverage(spread=True)
        lrn.Run(2)
        spread_on += window()
    lrn.drain()

    def timed(call):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = call()
        torch.cuda.synchronize()
        return r, 1e3 * (time.perf_counter() - t0)

    view, flush_ms = timed(lrn.Averaged)
    _, bound_ms = timed(lambda: view.Bound(-2))
    _, unsettled_ms = timed(lambda: view.Unsettled(10))
    med = lambda x: float(np.median(x)) if x else None   # noqa: E731
    over = lambda x: (med(x) / med(off) - 1.0) if off and x else None   # noqa: E731
    res = {"workload": args.workload, "N": N, "K": K, "mini_batch": m, "windows": args.windows, "steps_per_window": args.steps,
           "nonlink_steps": [len(off), len(mean_on), len(spread_on)], "nonlink_step_ms_off": med(off),
           "nonlink_step_ms_mean": med(mean_on), "nonlink_step_ms_spread": med(spread_on),
           "overhead_mean": over(mean_on), "overhead_spread": over(spread_on),
           "flushed_bytes_per_step_estimate": {"mean": 12 * K * (m + 1), "spread": 20 * K * (m + 1)},
           "full_flush_ms": flush_ms, "bound_view_ms": bound_ms, "unsettled_ms": unsettled_ms,
           "samples": view.samples, "device": torch.cuda.get_device_name(0),
           "how": "one process, one learner, eager loop with device sampling; alternating windows off / mean / spread, two "
                  "events around every Run(1)"}
    lrn.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
