#!/usr/bin/env python3
"""What reducing the model costs: ammsb_reduce_rows over all of pi at C3's shape (N = 10^6, K = 1024) against the same
statement in torch -- index_add_ of the columns into their new communities over column slabs, then the division by the row
sum -- in ONE process, alternating, medians.  pi is one block here, and both sides include the host time of their loop
(row slabs on one side, column slabs on the other).  The torch statement adds in another order and sums in binary32, so the results
are compared within (n_j + 3) * 2^-22, not bit for bit.  The plan: a fifth of the columns merged in pairs, a tenth dropped.
The bytes alone are (K + K') * 4 * N; update_pi streams at about 0.8 of 8 TB/s.  No speed is a condition of anything.
Needs a GPU.  Writes profiles/reduce_ab.json.

    python tools/reduce_ab.py [--rows 1000000] [--cols 1024] [--rounds 7] [--out profiles/reduce_ab.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "reduce_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    from mcmc_ammsb_gpu_amd._reduce import Plan
    if not torch.cuda.is_available():
        raise SystemExit("reduce_ab.py needs a HIP device")
    N, K = args.rows, args.cols
    ctx = ops.Context(ops.make_params(N, K, E=16 * N))
    pi = ops.RowPartitionedMatrix(ctx, N, K)
    blk = pi.blocks[0]
    blk.copy_(torch.rand((N, K), device=blk.device).pow_(16).clamp_(min=1e-12))
    blk.div_(blk.sum(1, keepdim=True))
    phi = torch.rand((N,), device=blk.device) + 1
    theta = torch.rand((2 * K,), device=blk.device) + 0.5
    rng = np.random.default_rng(1)
    cols = rng.permutation(K)
    pairs = cols[:2 * (K // 10)].reshape(-1, 2)
    plan = Plan.identity(K).merge(pairs).drop(cols[-(K // 10):])
    red = ops.ModelReducer(ctx)
    out_pi = ops.RowPartitionedMatrix(ctx, N, plan.new_K)
    out_phi, out_theta = torch.empty_like(phi), ctx.empty((2 * plan.new_K,), torch.float32)
    index = torch.from_numpy(np.where(plan.map < 0, plan.new_K, plan.map).astype(np.int64)).to(blk.device)   # dropped -> a spare column
    acc = torch.empty((N, plan.new_K + 1), device=blk.device)
    ref = torch.empty((N, plan.new_K), device=blk.device)
    cslab = 64   # columns per index_add_

    def ours():
        red.run(pi, phi, theta, plan, out_pi=out_pi, out_phi=out_phi, out_theta=out_theta)

    def theirs():
        acc.zero_()
        for c0 in range(0, K, cslab):
            acc.index_add_(1, index[c0:c0 + cslab], blk[:, c0:c0 + cslab])
        kept = acc[:, :plan.new_K]
        torch.div(kept, kept.sum(1, keepdim=True), out=ref)

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(f):
        ev[0].record()
        f()
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    for f in (ours, theirs, ours, theirs):
        f()
    torch.cuda.synchronize()
    t_ours, t_theirs = [], []
    for _ in range(args.rounds):
        t_ours.append(timed(ours))
        t_theirs.append(timed(theirs))
    n_src = torch.from_numpy(np.diff(plan.csr()[0]).astype(np.float32)).to(blk.device)
    rel = ((out_pi.blocks[0] - ref).abs() / ref.clamp(min=1e-30) / (n_src + 3)).max().item()
    assert rel <= 2.0 ** -22, rel
    ms = float(np.median(t_ours))
    nbytes = (K + plan.new_K) * 4 * N
    res = {"N": N, "K": K, "new_K": plan.new_K, "dropped": int(plan.dropped.size), "last_kernel": red.kernel_name(),
           "reduce_ms": ms, "torch_ms": float(np.median(t_theirs)), "ratio": float(np.median(t_theirs)) / ms,
           "bytes": nbytes, "TB_per_s": nbytes / ms / 1e9, "update_pi_streams_at": "about 0.8 of 8 TB/s",
           "max_rel_difference_over_(n_j+3)": rel, "rounds": args.rounds, "device": torch.cuda.get_device_name(0),
           "how": "one process, alternating, medians; host time of the slab loop included on both sides"}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
