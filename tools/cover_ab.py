#!/usr/bin/env python3
"""Same-process A/B of the cover match at C3's shape (N = 10^6, K = 1024, one block; rows as fitted rows look: gamma(1/K)
draws, floored and normalised like update_pi leaves them), at thr in {0.05, 0.01}, against two ground-truth covers:
  planted   the cover the generator plants in C3's graph (hostlib.generate_cover(N, 64, seed 20260101): M ~ 2 N);
  snaplike  community sizes drawn log-uniform from 3 to 10^4 until M ~ 2 N, members uniform.
The contenders alternate in one process:
  ours      ammsb_cover_match, the whole call (memsets, the counting form, cover_finish, cover_unpack): cover_fast over
            the aligned block, and cover_generic over a copy of pi whose base is 4 bytes past a 16-byte boundary;
  torch     the statement a user had before, in slabs of at most --torch-slab members (whole communities): gather the
            rows, compare, index_add_ into a [slab's communities, K] matrix, argmax of o / (t + d) both ways;
  update_pi ammsb_update_pi over all N rows of a pi of the same shape (8 N K bytes, what M = 2 N rows of 4 K bytes are):
            the project's own streaming ruler.
Each as ms (median and min of the rounds, device events) and as bytes / time against 8 TB/s; ours moves 4 K bytes per
member.  Untimed rounds run first until a second has passed and five consecutive rounds of the first case agree within
3 % (at most --settle-s seconds).  Every GPU step runs under a time limit of its own (--step-limit-s): a step that does
not come back ends the process with status 124 and starts nothing more.
  python tools/cover_ab.py [--rows N] [--cols K] [--rounds R] [--out FILE.json]
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
PEAK_BYTES = 8e12
THRS = (0.05, 0.01)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--k-true", type=int, default=64)
    ap.add_argument("--torch-slab", type=int, default=131_072)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--settle-s", type=float, default=8.0)
    ap.add_argument("--step-limit-s", type=float, default=60.0)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("cover_ab.py needs a HIP device: a timing taken anywhere else says nothing")
    import ammsb_pkg
    ammsb_pkg.load()
    from mcmc_ammsb_gpu_amd import _cover, hostlib, ops
    from mcmc_ammsb_gpu_amd._capi import Rpm
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
    # the same values behind a base that no 16-byte load may use: the generic form
    shifted = ctx.empty((N * K + 1,), torch.float32)
    shifted[1:].copy_(blk.reshape(-1))
    desc = Rpm()
    desc.blocks[0] = shifted.data_ptr() + 4
    desc.rows_in_block, desc.num_rows, desc.num_cols, desc.num_blocks = N, N, K, 1

    class Shifted:
        cols = K
    Shifted.desc = desc

    rng = np.random.default_rng(2)
    covers = {"planted": hostlib.generate_cover(N, args.k_true, seed=20260101)}
    sizes = []
    while sum(sizes) < 2 * N:
        sizes.append(int(round(float(np.exp(rng.uniform(np.log(3.0), np.log(1e4)))))))
    sizes = [min(s, N) for s in sizes]
    off = np.zeros(len(sizes) + 1, dtype=np.uint64)
    off[1:] = np.cumsum(sizes)
    covers["snaplike"] = (off, np.concatenate([rng.choice(N, s, replace=False) for s in sizes]).astype(np.uint32))

    cm, ro = ops.CoverMatch(ctx), ops.CommunityReadout(ctx)
    dsize = {thr: ro.sizes(pi, thr).clone() for thr in THRS}
    on_dev = {}
    for name, (o, m) in covers.items():
        o, m = _cover.check_cover((o, m))
        t = np.diff(o.astype(np.int64))
        on_dev[name] = dict(offsets=ctx.from_numpy(o), members=ctx.from_numpy(m), G=int(o.size - 1), M=int(m.size),
                            idx=torch.from_numpy(m.astype(np.int64)).to(dev),
                            comm=torch.from_numpy(np.repeat(np.arange(t.size), t)).to(dev),
                            t=torch.from_numpy(t).to(dev), host_offsets=o.astype(np.int64))
        cm.reserve(cm.workspace_bytes(m.size, K))
    pi2 = ops.RowPartitionedMatrix(ctx, N, K)
    phi_vec = blk.clone()
    phi_sum = ctx.zeros((N,), torch.float32)
    nodes = torch.arange(N, dtype=torch.int32, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    forms = {}

    def ours(which, cover, thr):
        c = on_dev[cover]

        def f():
            cm.match(which, thr, c["offsets"], c["members"], dsize[thr])
            forms[cm.kernel_name()] = True
        return f

    def torch_way(cover, thr):
        c = on_dev[cover]
        ho, d = c["host_offsets"], dsize[thr].to(torch.float64)
        cuts, g = [0], 0          # whole communities, at most --torch-slab members each (a larger community alone)
        while g < c["G"]:
            h = g + 1
            while h < c["G"] and ho[h + 1] - ho[g] <= args.torch_slab:
                h += 1
            cuts.append(h)
            g = h

        def f():
            best_d = torch.full((K,), -1.0, dtype=torch.float64, device=dev)
            arg_d = torch.full((K,), -1, dtype=torch.int64, device=dev)
            for g0, g1 in zip(cuts[:-1], cuts[1:]):
                lo, hi = int(ho[g0]), int(ho[g1])
                ov = torch.zeros((g1 - g0, K), dtype=torch.int32, device=dev)
                for a in range(lo, hi, args.torch_slab):
                    b = min(hi, a + args.torch_slab)
                    ov.index_add_(0, c["comm"][a:b] - g0, (blk[c["idx"][a:b]] >= thr).to(torch.int32))
                ratio = torch.where(ov > 0, ov / (c["t"][g0:g1, None] + d[None, :]), -1.0)
                ratio.max(1)
                v, i = ratio.max(0)
                better = v > best_d
                best_d = torch.where(better, v, best_d)
                arg_d = torch.where(better, i + g0, arg_d)
        return f

    def update_pi():
        ctx.check(ctx.lib.ammsb_update_pi(ctx.handle, C.byref(pi2.desc), C.c_void_p(phi_sum.data_ptr()),
                                          C.c_void_p(phi_vec.data_ptr()), C.c_void_p(nodes.data_ptr()), N, 64, stream))
    cases = []
    for cover in covers:
        nbytes = 4.0 * K * on_dev[cover]["M"]
        for thr in THRS:
            cases += [("ours fast %s thr=%g" % (cover, thr), ours(pi, cover, thr), nbytes),
                      ("ours generic %s thr=%g" % (cover, thr), ours(Shifted, cover, thr), nbytes),
                      ("torch %s thr=%g" % (cover, thr), torch_way(cover, thr), nbytes)]
    cases += [("update_pi all rows", update_pi, 8.0 * N * K)]

    def timed(name, f):
        def late():
            sys.stderr.write("cover_ab: %r did not come back within %g s\n" % (name, args.step_limit_s))
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
    rec = {"tool": "cover_ab", "device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "unit": _cover.UNIT,
           "rounds": args.rounds, "torch_slab": args.torch_slab,
           "covers": {n: {"communities": c["G"], "members": c["M"]} for n, c in on_dev.items()},
           "settle": {"rounds": settle_rounds, "seconds": round(time.perf_counter() - t0, 2)},
           "kernel_forms": sorted(forms), "peak_bytes_per_s": PEAK_BYTES, "cases": {}}
    for name, _, nbytes in cases:
        med = statistics.median(times[name])
        rec["cases"][name] = {"ms_median": round(med, 4), "ms_min": round(min(times[name]), 4),
                              "ms_max": round(max(times[name]), 4), "bytes": nbytes,
                              "TBps_median": round(nbytes / (med * 1e-3) / 1e12, 3),
                              "share_of_8TBps": round(nbytes / (med * 1e-3) / PEAK_BYTES, 3)}
    c = rec["cases"]
    keys = ["%s thr=%g" % (cover, thr) for cover in covers for thr in THRS]
    rec["torch_over_ours_fast"] = {k: round(c["torch " + k]["ms_median"] / c["ours fast " + k]["ms_median"], 2) for k in keys}
    rec["generic_over_fast"] = {k: round(c["ours generic " + k]["ms_median"] / c["ours fast " + k]["ms_median"], 2) for k in keys}
    rec["fast_rate_over_update_pi_rate"] = {k: round(c["ours fast " + k]["TBps_median"] / c["update_pi all rows"]["TBps_median"], 3)
                                            for k in keys}
    print(json.dumps(rec))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(rec, indent=1) + "\n")


if __name__ == "__main__":
    main()
