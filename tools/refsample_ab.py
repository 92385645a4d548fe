"""Three sampling modes in ONE process, alternating (README: in-process comparisons only): the eager Python loop on a
bench.py workload (default C3) with (a) host sampling, (b) the own-stream device sampler, (c) the reference stream on
the device.  Prints edges/s per mode and round, and the wall time of one non-link mini-batch's sampler chain on an
otherwise idle device (enqueue to result available) for each mode.

    python tools/refsample_ab.py [--workload C3] [--steps 40] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = {"C1": (10_000, 32, 1024, 32, 32, 32), "C2": (100_000, 256, 8192, 32, 32, 64),
             "C3": (1_000_000, 1024, 65536, 32, 32, 64)}   # bench.py's


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="C3", choices=sorted(WORKLOADS))
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--chain-batches", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import __graft_entry__ as ge
    ge.build()
    import numpy as np
    import torch
    from mcmc_ammsb_gpu_amd import hostlib
    from mcmc_ammsb_gpu_amd.learner import Config, Learner
    N, K, m, n, deg, k_true = WORKLOADS[args.workload]
    wg = 64 if K >= 1024 else 32
    ds = hostlib.Dataset.robust(N, hostlib.generate_graph(N, k_true, deg, seed=20260101), heldout_ratio=0.01, rand_seed=1)
    modes = {"host": dict(device_sampling=False), "own": dict(device_sampling=True),
             "reference": dict(device_sampling=True, sampling_stream="reference")}
    learners = {}
    for name, kw in modes.items():
        cfg = Config.from_cli_defaults(K=K, mini_batch_size=m, num_node_sample=n, strategy="Node", phi_wg_size=wg,
                                       beta_wg_size=wg, ppx_wg_size=wg, graph_launch=False, pi_placement_candidates=0, **kw)
        learners[name] = Learner(cfg, ds)
        learners[name].Run(args.warmup)
        learners[name].drain()
    res = {"workload": args.workload, "steps": args.steps, "rounds": [], "epochs": learners["reference"].ref_sampler.num_epochs}
    for r in range(args.rounds):
        row = {}
        for name, lrn in learners.items():   # a, b, c, a, b, c, ...
            e0, t0 = lrn.edges_done, time.perf_counter()
            lrn.Run(args.steps)
            lrn.drain()
            dt = time.perf_counter() - t0
            row[name] = {"edges_per_s": (lrn.edges_done - e0) / dt, "ms_per_step": 1e3 * dt / args.steps}
        res["rounds"].append(row)
        print("round %d: %s" % (r, json.dumps(row)), flush=True)
    # one non-link mini-batch's sampler chain, device otherwise idle: enqueue -> mini-batch on the device
    chain = {}
    s = learners["host"].samples[0]
    seed, ts = 12345, []
    for _ in range(args.chain_batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e, v, w, seed = ds.sample(m, "NodeNonLink", seed)
        s.pin_edges[:e.size].copy_(torch.from_numpy(e.view(np.int64)))
        s.pin_nodes[:v.size].copy_(torch.from_numpy(v.view(np.int32)))
        s.dev_edges[:e.size].copy_(s.pin_edges[:e.size], non_blocking=True)
        s.dev_nodes[:v.size].copy_(s.pin_nodes[:v.size], non_blocking=True)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    chain["host"] = 1e3 * float(np.median(ts))
    lo, smp, ts = learners["own"], learners["own"].dev_sampler, []
    for _ in range(args.chain_batches):
        ch = smp.choose("NodeNonLink")
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        smp.enqueue(ch, lo.samples[0].dev_edges, lo.samples[0].dev_nodes)
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    chain["own"] = 1e3 * float(np.median(ts))
    lr, smp, ts, seed = learners["reference"], learners["reference"].ref_sampler, [], 12345
    for _ in range(args.chain_batches):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, _, _, seed = smp.enqueue("NodeNonLink", seed, lr.samples[0].dev_edges, lr.samples[0].dev_nodes)
        ts.append(time.perf_counter() - t0)
    chain["reference"] = 1e3 * float(np.median(ts))
    res["nonlink_chain_ms"] = chain
    res["edges_per_s_median"] = {k: float(np.median([row[k]["edges_per_s"] for row in res["rounds"]])) for k in modes}
    print(json.dumps(res), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    for lrn in learners.values():
        lrn.close()


if __name__ == "__main__":
    main()
