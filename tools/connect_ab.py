#!/usr/bin/env python3
"""A/B of the community links (libammsb_connect.so) at C3's shape (N = 1e6, K = 1024, 16e6 links), in one
process, alternating so that both sides of a pair see the same clocks, the same pi and the same list:

    mask     ammsb_connect_mask (bits in community order) against ammsb_quality_mask on the same pi: the same bytes read,
             the same number of bits written
    edges    connect_edges_direct against connect_edges_runs (AMMSB_CONNECT_FORM) on the same sorted list, equal results
             asserted
    links    mask + edges + finish against the torch statement in edge slabs: directed += M[a].T @ M[b] in float32 (exact
             below 2^24 per slab), equal results asserted

The pi has a home community per node and a few more memberships; the list is assortative (most links stay inside the home
community), every link once as (min << 32) | max, ascending: what Learner.TrainingLinks() gives.

Writes profiles/connect_ab.json: the medians, the ratio of the mask pass to quality's, the ratio of the two edge forms
(the faster one on this list is to be the default for K <= 4096), the ratio of the torch statement to the whole call.

    python tools/connect_ab.py [--rows 1000000] [--cols 1024] [--links 16000000] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--links", type=int, default=16_000_000)
    ap.add_argument("--extra", type=int, default=2, help="memberships per node beside its home community")
    ap.add_argument("--inside", type=float, default=0.8, help="share of the links that stay inside the home community")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--torch-slab", type=int, default=1 << 18, help="edges per slab of the torch statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "connect_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    N, K, E, thr = args.rows, args.cols, args.links, args.threshold
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    cl, cq = ops.CommunityLinks(ctx), ops.CommunityQuality(ctx)
    pi = ops.RowPartitionedMatrix(ctx, N, K, 0)
    block = pi.blocks[0]
    dev = block.device
    g = torch.Generator(device=dev).manual_seed(1)
    block.uniform_(0.0, 0.8 * thr, generator=g)
    home = torch.arange(N, device=dev) * K // N          # consecutive nodes share a home community
    block[torch.arange(N, device=dev), home] = 0.5
    for _ in range(args.extra):
        block[torch.arange(N, device=dev), torch.randint(0, K, (N,), device=dev, generator=g)] = 0.2
    per = N // K
    a = torch.randint(0, N, (E,), device=dev, generator=g)
    inside = torch.rand((E,), device=dev, generator=g) < args.inside
    b = torch.where(inside, (a // per).clamp(max=K - 1) * per + torch.randint(0, per, (E,), device=dev, generator=g),
                    torch.randint(0, N, (E,), device=dev, generator=g)).clamp(max=N - 1)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    keys = torch.unique((lo << 32) | hi)[: E]            # sorted, every link once
    keys = keys[(keys >> 32) != (keys & 0xFFFFFFFF)].contiguous()
    n = int(keys.numel())

    def edges(form):
        os.environ["AMMSB_CONNECT_FORM"] = form
        try:
            return cl.edges(mask, N, K, keys)[0]
        finally:
            del os.environ["AMMSB_CONNECT_FORM"]

    def ours():
        return cl.finish(cl.edges(cl.mask(pi, thr), N, K, keys)[0])

    def statement():
        total = torch.zeros((K, K), dtype=torch.int64, device=dev)
        for s in range(0, n, args.torch_slab):
            k = keys[s:s + args.torch_slab]
            Ma, Mb = (block[k >> 32] >= thr).to(torch.float32), (block[k & 0xFFFFFFFF] >= thr).to(torch.float32)
            total += (Ma.T @ Mb).to(torch.int64)
        return total + total.T

    mask = cl.mask(pi, thr)
    for fn in (lambda: cl.mask(pi, thr), lambda: cq.mask(pi, thr), lambda: edges("d"), lambda: edges("r"), ours, statement):
        fn()   # not timed: code loading
    torch.cuda.synchronize()
    t = {"connect_mask": [], "quality_mask": [], "edges_direct": [], "edges_runs": [], "whole_call": [], "torch_statement": []}
    forms_equal = links_equal = True
    for _ in range(args.reps):
        t["connect_mask"].append(timed(torch, lambda: cl.mask(pi, thr))[0])
        t["quality_mask"].append(timed(torch, lambda: cq.mask(pi, thr))[0])
        s, d = timed(torch, lambda: edges("d"))
        t["edges_direct"].append(s)
        s, r = timed(torch, lambda: edges("r"))
        t["edges_runs"].append(s)
        forms_equal = forms_equal and bool(torch.equal(d, r))
        s, x = timed(torch, ours)
        t["whole_call"].append(s)
        s, y = timed(torch, statement)
        t["torch_statement"].append(s)
        links_equal = links_equal and bool(torch.equal(x, y))
    assert forms_equal and links_equal, (forms_equal, links_equal)
    med = {k: statistics.median(v) for k, v in t.items()}
    members = float((block >= thr).sum().item()) / N
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "links": n, "threshold": thr, "reps": args.reps,
              "memberships_per_node": members, "inside_share": args.inside, "torch_slab_edges": args.torch_slab,
              "median_s": med, "all_s": t, "pi_bytes": N * K * 4,
              "connect_mask_GBps": N * K * 4 / med["connect_mask"] / 1e9, "quality_mask_GBps": N * K * 4 / med["quality_mask"] / 1e9,
              "mask_over_quality_mask": med["connect_mask"] / med["quality_mask"],
              "direct_over_runs": med["edges_direct"] / med["edges_runs"],
              "faster_edge_form": "direct" if med["edges_direct"] <= med["edges_runs"] else "runs",
              "torch_over_whole_call": med["torch_statement"] / med["whole_call"],
              "forms_equal": forms_equal, "links_equal": links_equal}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
