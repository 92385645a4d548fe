#!/usr/bin/env python3
"""A/B of the community relations (libammsb_relate.so) at C3's shape (N = 1e6, K = 1024), in one process,
alternating so that both sides of a pair see the same clocks and the same pi:

    bits     ammsb_relate_bits (community-major words) against ammsb_quality_mask on the same pi: the same bytes read,
             the same number of bits written, node-major there
    overlap  the bits + pair passes against the torch statement in node slabs: M = pi[lo:hi] >= thr, overlap +=
             M.T @ M in float32 (exact below 2^24 per slab) or float16 (slabs of at most 2048 rows, so that the float16
             result is exact)

Writes profiles/relate_ab.json: the medians, the ratio of the bits pass to the mask pass, the ratio of the torch statement
to bits + pairs, and whether the two overlaps are equal.

    python tools/relate_ab.py [--rows 1000000] [--cols 1024] [--reps 7] [--torch-dtype float|half] [--out FILE]"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e-3, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--cols", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--torch-dtype", default="float", choices=("half", "float"))
    ap.add_argument("--torch-slab", type=int, default=65536, help="rows per slab of the torch statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "relate_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    N, K, thr = args.rows, args.cols, args.threshold
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    cr, cq = ops.CommunityRelations(ctx), ops.CommunityQuality(ctx)
    pi = ops.RowPartitionedMatrix(ctx, N, K, 0)
    block = pi.blocks[0]
    block.uniform_(0.0, 0.8 * thr)
    block[torch.rand((N, K), device=block.device) < K ** -0.5] = 0.5   # about K^-1/2 of the entries are members
    dtype = torch.float16 if args.torch_dtype == "half" else torch.float32

    def ours():
        overlap = ctx.zeros((K, K), torch.int32)
        cr.pairs(cr.bits(pi, thr), K, N, overlap)
        return overlap

    # a float16 product comes back as float16, which holds a count exactly up to 2048: slabs of at most that many rows
    slab = min(args.torch_slab, 2048) if dtype == torch.float16 else args.torch_slab

    def statement():
        total = torch.zeros((K, K), dtype=torch.int64, device=block.device)
        for lo in range(0, N, slab):
            M = (block[lo:lo + slab] >= thr).to(dtype)
            total += (M.T @ M).to(torch.int64)
        return total

    bits = cr.bits(pi, thr)
    pairs_only = lambda: cr.pairs(bits, K, N, ctx.zeros((K, K), torch.int32))   # noqa: E731
    for fn in (lambda: cr.bits(pi, thr), lambda: cq.mask(pi, thr), pairs_only, ours, statement):   # not timed: code loading
        fn()
    torch.cuda.synchronize()
    t = {"relate_bits": [], "quality_mask": [], "relate_pairs": [], "bits_and_pairs": [], "torch_statement": []}
    equal = True
    for _ in range(args.reps):
        t["relate_bits"].append(timed(torch, lambda: cr.bits(pi, thr))[0])
        t["quality_mask"].append(timed(torch, lambda: cq.mask(pi, thr))[0])
        t["relate_pairs"].append(timed(torch, pairs_only)[0])
        s, a = timed(torch, ours)
        t["bits_and_pairs"].append(s)
        s, b = timed(torch, statement)
        t["torch_statement"].append(s)
        equal = equal and bool(torch.equal(a.to(torch.int64), b))
    med = {k: statistics.median(v) for k, v in t.items()}
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "threshold": thr, "reps": args.reps,
              "torch_dtype": args.torch_dtype, "torch_slab_rows": slab, "kernel_forms": [cr.kernel_name()],
              "median_s": med, "all_s": t, "pi_bytes": N * K * 4,
              "relate_bits_GBps": N * K * 4 / med["relate_bits"] / 1e9, "quality_mask_GBps": N * K * 4 / med["quality_mask"] / 1e9,
              "bits_over_mask": med["relate_bits"] / med["quality_mask"],
              "torch_over_bits_and_pairs": med["torch_statement"] / med["bits_and_pairs"], "overlaps_equal": equal}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
