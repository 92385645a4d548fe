#!/usr/bin/env python3
"""A/B of the overlapping modularity (libammsb_modularity.so) at C3's shape (N = 1e6, K = 1024, 16e6 links),
in one process, alternating so that both sides see the same clocks, the same pi and the same list:

    ours       mask (ops.CommunityLinks) + ammsb_modularity_edges + ammsb_modularity_nodes: 128-bit integer sums
    statement  the torch statement in edge slabs: O = M.sum(1); per slab w = 1 / (O[a] O[b]) in float64 and
               IN += ((M[a] & M[b]) * w[:, None]).sum(0); deg by bincount; SV = ((M * (deg / O)[:, None])).sum(0) in node
               slabs.  Float sums: q is compared to 1e-9, not bit for bit.

The pi has a home community per node and a few more memberships; the list is assortative (most links stay inside the home
community), every link once as (min << 32) | max, ascending: what Learner.TrainingLinks() gives.

Needs a GPU.  Writes profiles/modularity_ab.json: the medians, the ratio of the torch statement to the whole call, both q.

    python tools/modularity_ab.py [--rows 1000000] [--cols 1024] [--links 16000000] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--torch-slab", type=int, default=1 << 17, help="edges (and nodes) per slab of the torch statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "modularity_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import _modularity, ops
    N, K, E, thr = args.rows, args.cols, args.links, args.threshold
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    md = ops.Modularity(ctx)
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

    def ours():
        return md.run(pi, thr, keys)

    def q_of(out):
        internal, volume, counts, _ = out
        valid, skipped = (int(v) for v in counts.cpu().numpy())
        return _modularity.Modularity(thr, _modularity.wide(internal.cpu().numpy()), _modularity.wide(volume.cpu().numpy()),
                                      valid, skipped).q

    def statement():
        O = torch.zeros((N,), dtype=torch.float64, device=dev)
        for s in range(0, N, args.torch_slab):
            O[s:s + args.torch_slab] = (block[s:s + args.torch_slab] >= thr).sum(1)
        inv = torch.where(O > 0, 1.0 / O, torch.zeros_like(O))
        IN = torch.zeros((K,), dtype=torch.float64, device=dev)
        for s in range(0, n, args.torch_slab):
            k = keys[s:s + args.torch_slab]
            u, v = k >> 32, k & 0xFFFFFFFF
            both = (block[u] >= thr) & (block[v] >= thr)
            IN += (both * (inv[u] * inv[v])[:, None]).sum(0)
        deg = (torch.bincount(keys >> 32, minlength=N) + torch.bincount(keys & 0xFFFFFFFF, minlength=N)).to(torch.float64)
        SV = torch.zeros((K,), dtype=torch.float64, device=dev)
        for s in range(0, N, args.torch_slab):
            SV += ((block[s:s + args.torch_slab] >= thr) * (deg * inv)[s:s + args.torch_slab, None]).sum(0)
        two_m = 2.0 * n
        return float(((2.0 * IN - SV * SV / two_m) / two_m).sum().item())

    for fn in (ours, statement):
        fn()   # not timed: code loading
    torch.cuda.synchronize()
    t = {"whole_call": [], "torch_statement": []}
    q_ours = q_torch = None
    for _ in range(args.reps):
        s, out = timed(torch, ours)
        t["whole_call"].append(s)
        s, q_torch = timed(torch, statement)
        t["torch_statement"].append(s)
        again = q_of(out)
        assert q_ours is None or again == q_ours, "two runs of the library differ"
        q_ours = again
    assert abs(q_ours - q_torch) <= 1e-9, (q_ours, q_torch)
    med = {k: statistics.median(v) for k, v in t.items()}
    members = float((block >= thr).sum().item()) / N
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "links": n, "threshold": thr, "reps": args.reps,
              "memberships_per_node": members, "inside_share": args.inside, "torch_slab": args.torch_slab,
              "median_s": med, "all_s": t, "torch_over_whole_call": med["torch_statement"] / med["whole_call"],
              "q": q_ours, "q_torch": q_torch}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
