#!/usr/bin/env python3
"""What the chain average costs per iteration: bench.py's workload (default C3: N = 10^6, K = 1024, mini-batch 65536) on the
eager loop, in ONE process and on ONE learner, in alternating windows with the average off and on.  Every step is timed by
itself (two events around Run(1)); the figure is the median over the non-link steps (a mini-batch of the configured size)
of each kind of window, so the two are compared under the same clocks and the same placement of pi.  Also timed: one full
flush (every row, what the first analysis after a run pays) and a flush when nothing ran since (nothing is launched).
Needs a GPU.  Writes profiles/average_ab.json.

    python tools/average_ab.py [--workload C3] [--windows 6] [--steps 40] [--out profiles/average_ab.json]
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
    ap.add_argument("--windows", type=int, default=6, help="windows of each kind")
    ap.add_argument("--steps", type=int, default=40, help="steps per window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "average_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from bench import WORKLOADS, pick_wg
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd.learner import Config, Learner
    if not torch.cuda.is_available():
        raise SystemExit("average_ab.py needs a HIP device")
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

    off, on = [], []
    for _ in range(args.windows):
        lrn.StopAverage()
        off += window()
        lrn.StartAverage()
        lrn.Run(2)        # the first averaged steps copy rows (no read of the mean): not what a long run pays
        on += window()
    lrn.drain()
    t0 = time.perf_counter()
    view = lrn.Averaged()
    torch.cuda.synchronize()
    flush_ms = 1e3 * (time.perf_counter() - t0)
    t0 = time.perf_counter()
    view.drain()
    noop_ms = 1e3 * (time.perf_counter() - t0)
    med = lambda x: float(np.median(x)) if x else None   # noqa: E731
    res = {"workload": args.workload, "N": N, "K": K, "mini_batch": m, "windows": args.windows, "steps_per_window": args.steps,
           "nonlink_steps_off": len(off), "nonlink_steps_on": len(on), "nonlink_step_ms_off": med(off), "nonlink_step_ms_on": med(on),
           "overhead": (med(on) / med(off) - 1.0) if off and on else None,
           "flushed_bytes_per_step_estimate": 12 * K * (m + 1), "full_flush_ms": flush_ms, "flush_when_clean_ms": noop_ms,
           "samples": view.samples, "device": torch.cuda.get_device_name(0),
           "how": "one process, one learner, eager loop with device sampling; alternating windows, two events around every Run(1)"}
    lrn.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
