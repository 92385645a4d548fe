#!/usr/bin/env python3
"""A/B of the Omega index's pair pass (libammsb_omega.so) against the torch statement in slabs
(M @ M.T per slab of rows + bincount), on synthetic bit-level covers:

    case a   n = 1e5, K = 1024, G = 5000
    case b   n = 1e6, K = G = 1024

Reports per case the pass's time, word-pairs per second (pairs x words of both row sets), that as a fraction of the
AND + population-count issue bound (256 CUs x 64 lanes x the shader clock held under load, which ammsb_clock_probe reads
beside a running pair launch, / 2 instructions per word),
the slowest single launch at the default launch_pairs, and the torch statement's time per pair measured on --torch-slabs
slabs (the whole statement at n = 1e6 would take hours).  Writes profiles/omega_ab.json.

    python tools/omega_ab.py [--cases a,b] [--torch-slabs 4] [--out profiles/omega_ab.json]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CASES = {"a": (100_000, 1024, 5000), "b": (1_000_000, 1024, 1024)}


def synthetic(rng, N, K, G):
    """pi with about K^-1/2 of the entries above 0.05; a ground truth in which every node is in 1 to 3 communities"""
    import torch
    pi = torch.rand((N, K), device="cuda") * 0.04
    pi[torch.rand((N, K), device="cuda") < K ** -0.5] = 0.5
    per = rng.integers(1, 4, N)
    nodes = np.repeat(np.arange(N, dtype=np.uint32), per)
    comm = rng.integers(0, G, nodes.size)
    keys = np.unique(comm.astype(np.int64) * N + nodes)     # sets: no node twice inside a community
    comm, nodes = keys // N, (keys % N).astype(np.uint32)
    offsets = np.zeros(G + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(comm, minlength=G))
    return pi, offsets, nodes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", default="a,b")
    ap.add_argument("--torch-slabs", type=int, default=4)
    ap.add_argument("--launch-pairs", type=int, default=1 << 31)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "omega_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _omega, ops
    result = {"device": torch.cuda.get_device_name(0), "launch_pairs": args.launch_pairs, "cases": {}}
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    om = ops.CoverOmega(ctx)
    for name in args.cases.split(","):
        N, K, G = CASES[name]
        rng = np.random.default_rng(1)
        pi_t, offsets, members = synthetic(rng, N, K, G)
        pi = ops.RowPartitionedMatrix(ctx, N, K, 0)
        pi.load(pi_t.cpu().numpy())
        position = ctx.from_numpy(np.arange(N, dtype=np.int32))
        dbits, dcount = om.detected_bits(pi, 0.05, n=N)
        tbits, tcount, tally = om.truth_bits(ctx.from_numpy(offsets), ctx.from_numpy(members), N, position, N)
        L = 1 + max(int(dcount.max().item()), int(tcount.max().item()))
        total = _omega.tiles(N)
        step = min(_omega.MAX_LAUNCH_TILES, max(1, args.launch_pairs // (_omega.TILE * _omega.TILE)))
        # not timed: the first launch loads the code and sets the kernel's LDS attribute; then the shader clock while a
        # launch of the timed size runs
        warm = ctx.zeros((3 * L + 1,), torch.int64)
        om.pairs(dbits, K, tbits, G, N, L, warm, 0, 1)
        probe = ops.ClockProbe(ctx)
        om.pairs(dbits, K, tbits, G, N, L, warm, 0, min(step, total))
        probe.launch()
        om.pairs(dbits, K, tbits, G, N, L, warm, 0, min(step, total))
        clock = probe.read()
        torch.cuda.synchronize()
        bound = 256 * 64 * (clock["mhz"] or 0.0) * 1e6 / 2
        hist = ctx.zeros((3 * L + 1,), torch.int64)
        launches = []
        for t0 in range(0, total, step):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            om.pairs(dbits, K, tbits, G, N, L, hist, t0, min(step, total - t0))
            b.record()
            b.synchronize()
            launches.append(a.elapsed_time(b) * 1e-3)
        P = N * (N - 1) // 2
        h = hist.cpu().numpy()
        assert int(h[L:2 * L].sum()) == P and int(h[3 * L]) == 0
        words = (K + 31) // 32 + (G + 31) // 32
        seconds = sum(launches)
        # the torch statement on a few slabs of rows against all columns
        MD, MT = (pi_t >= 0.05).to(torch.float16), torch.zeros((N, G), dtype=torch.float16, device="cuda")
        comm = np.repeat(np.arange(G), np.diff(offsets.astype(np.int64)))
        MT[torch.from_numpy(members.astype(np.int64)).cuda(), torch.from_numpy(comm).cuda()] = 1
        rows, spent, done = max(1, (256 << 20) // (4 * N)), 0.0, 0
        for sl in range(args.torch_slabs):
            lo = sl * rows
            if lo >= N:
                break
            hi = min(lo + rows, N)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            sd = (MD[lo:hi] @ MD.T).to(torch.int64).reshape(-1)
            st = (MT[lo:hi] @ MT.T).to(torch.int64).reshape(-1)
            torch.bincount(sd, minlength=L), torch.bincount(st, minlength=L), torch.bincount(sd[sd == st], minlength=L)
            b.record()
            b.synchronize()
            spent += a.elapsed_time(b) * 1e-3
            done += (hi - lo) * N
        result["cases"][name] = {
            "n": N, "K": K, "G": G, "L": L, "pairs": P, "words_per_pair": words, "launches": len(launches),
            "pair_pass_s": seconds, "slowest_launch_s": max(launches), "word_pairs_per_s": P * words / seconds,
            "clock_under_load": clock, "issue_bound_word_pairs_per_s": bound,
            "fraction_of_issue_bound": P * words / seconds / bound if bound else None,
            "torch_s_per_pair_square": spent / done, "torch_s_extrapolated": spent / done * N * N,
            "omega": _omega.scores(h[:L], h[L:2 * L], h[2 * L:3 * L], N)[0]}
        print(json.dumps({name: result["cases"][name]}), flush=True)
        del MD, MT, pi_t, dbits, tbits
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
