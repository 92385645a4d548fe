#!/usr/bin/env python3
"""A/B of the node roles (libammsb_roles.so) at C3's shape (N = 1e6, K = 1024, 16e6 links, three memberships
per node), in one process, alternating so that both sides see the same clocks, the same pi and the same adjacency:

    ours       mask (ops.CommunityLinks) + ammsb_roles_nodes over the symmetric CSR of the links
    statement  the torch statement in slabs of targets: gather the bool rows M[targets] of a slab, a segment sum per
               source node (index_add_ into an int32 [nodes of the slab, K] table), then degree, embedded, reached, votes,
               squares from the table and `topk` for the slots.  A slab ends on a row boundary.

The pi has a home community per node and a few more memberships; the list is assortative (most links stay inside the home
community), every link once, put into both ends' rows.

Needs a GPU.  Writes profiles/roles_ab.json: the medians, the ratio of the torch statement to the whole call, and whether
degree, embedded, reached, votes, squares and slot 0's count are equal (topk breaks ties its own way, so slot ids are not
compared).

    python tools/roles_ab.py [--rows 1000000] [--cols 1024] [--links 16000000] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--top", type=int, default=4)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--threshold", type=float, default=0.05)
    ap.add_argument("--torch-slab", type=int, default=1 << 14, help="source nodes per slab of the torch statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roles_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    N, K, E, thr, top = args.rows, args.cols, args.links, args.threshold, args.top
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    rl = ops.NodeRoles(ctx)
    pi = ops.RowPartitionedMatrix(ctx, N, K, 0)
    block = pi.blocks[0]
    dev = block.device
    g = torch.Generator(device=dev).manual_seed(1)
    block.uniform_(0.0, 0.8 * thr, generator=g)
    home = torch.arange(N, device=dev) * K // N          # consecutive nodes share a home community
    block[torch.arange(N, device=dev), home] = 0.5
    for _ in range(args.extra):
        block[torch.arange(N, device=dev), torch.randint(0, K, (N,), device=dev, generator=g)] = 0.2
    per = max(1, N // K)
    a = torch.randint(0, N, (E,), device=dev, generator=g)
    inside = torch.rand((E,), device=dev, generator=g) < args.inside
    b = torch.where(inside, (a // per).clamp(max=K - 1) * per + torch.randint(0, per, (E,), device=dev, generator=g),
                    torch.randint(0, N, (E,), device=dev, generator=g)).clamp(max=N - 1)
    lo, hi = torch.minimum(a, b), torch.maximum(a, b)
    keys = torch.unique((lo << 32) | hi)
    keys = keys[(keys >> 32) != (keys & 0xFFFFFFFF)]
    src, dst = torch.cat((keys >> 32, keys & 0xFFFFFFFF)), torch.cat((keys & 0xFFFFFFFF, keys >> 32))
    order = torch.sort(src, stable=True).indices
    rows = torch.bincount(src, minlength=N)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(rows, 0)
    src, targets64 = src[order], dst[order]
    targets = targets64.to(torch.int32).contiguous()
    bounds = offsets.cpu().tolist()

    def ours():
        return rl.run(pi, thr, offsets, targets, top=top)

    def statement():
        out = {n: torch.zeros(N, dtype=torch.int64, device=dev) for n in ("degree", "embedded", "reached", "votes", "squares", "c0")}
        for s in range(0, N, args.torch_slab):
            e = min(N, s + args.torch_slab)
            lo_t, hi_t = bounds[s], bounds[e]
            mine = block[s:e] >= thr
            table = torch.zeros((e - s, K), dtype=torch.int32, device=dev)
            if hi_t > lo_t:
                rows_b = block[targets64[lo_t:hi_t]] >= thr
                local = src[lo_t:hi_t] - s
                table.index_add_(0, local, rows_b.to(torch.int32))
                out["embedded"][s:e] = torch.zeros(e - s, dtype=torch.int64, device=dev).index_add_(
                    0, local, (rows_b & mine[local]).any(1).to(torch.int64))
            wide = table.to(torch.int64)
            out["degree"][s:e] = rows[s:e]
            out["reached"][s:e] = (table > 0).sum(1)
            out["votes"][s:e] = wide.sum(1)
            out["squares"][s:e] = (wide * wide).sum(1)
            out["c0"][s:e] = torch.topk(table, min(top, K), dim=1).values[:, 0]
        return out

    for fn in (ours, statement):
        fn()   # not timed: code loading
    torch.cuda.synchronize()
    t = {"whole_call": [], "torch_statement": []}
    equal = True
    for _ in range(args.reps):
        s, st = timed(torch, ours)
        t["whole_call"].append(s)
        s, ref = timed(torch, statement)
        t["torch_statement"].append(s)
        for n in ("degree", "embedded", "reached"):
            equal = equal and bool(torch.equal(st[n].to(torch.int64) & 0xFFFFFFFF, ref[n]))
        equal = equal and bool(torch.equal(st["votes"], ref["votes"])) and bool(torch.equal(st["squares"], ref["squares"]))
        equal = equal and bool(torch.equal(st["hcount"][:, 0].to(torch.int64) & 0xFFFFFFFF, ref["c0"]))
    assert equal, "the library and the torch statement differ"
    med = {k: statistics.median(v) for k, v in t.items()}
    members = float((block >= thr).sum().item()) / N
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "links": int(keys.numel()),
              "targets": int(targets.numel()), "threshold": thr, "top": top, "reps": args.reps, "memberships_per_node": members,
              "inside_share": args.inside, "torch_slab": args.torch_slab, "kernel": rl.kernel_name(), "median_s": med, "all_s": t,
              "torch_over_whole_call": med["torch_statement"] / med["whole_call"], "equal": equal}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
