#!/usr/bin/env python3
"""A/B of the triangles inside the detected communities (libammsb_triangles.so) at C3's shape (N = 1e6,
K = 1024, 16e6 links, three memberships per node), in one process, alternating so that both sides see the same clocks, the
same pi and the same simple adjacency:

    ours       mask (ops.CommunityLinks) + ammsb_triangles_nodes over the simple CSR of the links (the rows are verified
               on the device first, as in every call of ops.Triangles.nodes; that is part of the whole call)
    statement  the torch statement in slabs of directed links (a, b): every c > b of b's row (repeat_interleave over the
               row lengths above b) makes a wedge, and the wedge is a triangle iff the key (a << 32) | c is among the sorted
               keys of the adjacency (searchsorted); tri by index_add_, and for the triangles alone the bool rows of the
               three corners are gathered for tri_in and for the sum of ktri3.

The pi has a home community per node and a few more memberships; the list is assortative (most links stay inside the home
community, whose nodes are consecutive), every link once, put into both ends' rows.

Needs a GPU.  Writes profiles/triangles_ab.json: the medians, the ratio of the torch statement to the whole call, and
whether tri, tri_in and the sum of ktri3 are equal.

    python tools/triangles_ab.py [--rows 1000000] [--cols 1024] [--links 16000000] [--reps 5] [--out FILE]"""
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
    ap.add_argument("--torch-slab", type=int, default=1 << 20, help="directed links per slab of the torch statement")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "triangles_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    N, K, E, thr = args.rows, args.cols, args.links, args.threshold
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    tr = ops.Triangles(ctx)
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
    both = torch.unique(torch.cat(((a << 32) | b, (b << 32) | a)))   # the simple adjacency as sorted keys
    both = both[(both >> 32) != (both & 0xFFFFFFFF)]
    src, dst = both >> 32, both & 0xFFFFFFFF
    rows = torch.bincount(src, minlength=N)
    offsets = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    offsets[1:] = torch.cumsum(rows, 0)
    targets = dst.to(torch.int32).contiguous()
    # per node where its row's targets above the node begin
    above = offsets[:-1] + torch.zeros(N, dtype=torch.int64, device=dev).index_add_(0, src, (dst < src).to(torch.int64))
    M = both.numel()

    def ours():
        return tr.run(pi, thr, offsets, targets)

    def statement():
        tri = torch.zeros(N, dtype=torch.int64, device=dev)
        tri_in = torch.zeros(N, dtype=torch.int64, device=dev)
        ksum = 0
        for s in range(0, M, args.torch_slab):
            e = min(M, s + args.torch_slab)
            ea, eb = src[s:e], dst[s:e]
            n_c = offsets[eb + 1] - above[eb]          # the targets of b's row above b
            which = torch.repeat_interleave(torch.arange(e - s, device=dev), n_c)
            first = torch.cumsum(n_c, 0) - n_c
            c = dst[above[eb][which] + (torch.arange(which.numel(), device=dev) - first[which])]
            wa = ea[which]
            want = (wa << 32) | c
            at = torch.searchsorted(both, want).clamp(max=M - 1)
            hit = both[at] == want
            wa, wb, wc = wa[hit], eb[which][hit], c[hit]
            tri.index_add_(0, wa, torch.ones_like(wa))
            m = (block[wa] >= thr) & (block[wb] >= thr) & (block[wc] >= thr)
            tri_in.index_add_(0, wa, m.any(1).to(torch.int64))
            ksum += int(m.sum())
        return tri, tri_in, ksum

    for fn in (ours, statement):
        fn()   # not timed: code loading
    torch.cuda.synchronize()
    t = {"whole_call": [], "torch_statement": []}
    equal = True
    for _ in range(args.reps):
        s, st = timed(torch, ours)
        t["whole_call"].append(s)
        s, (tri, tri_in, ksum) = timed(torch, statement)
        t["torch_statement"].append(s)
        equal = equal and bool(torch.equal(st["tri"].to(torch.int64) & 0xFFFFFFFF, tri))
        equal = equal and bool(torch.equal(st["tri_in"].to(torch.int64) & 0xFFFFFFFF, tri_in))
        equal = equal and int(st["ktri3"].sum()) == ksum
    assert equal, "the library and the torch statement differ"
    med = {k: statistics.median(v) for k, v in t.items()}
    members = float((block >= thr).sum().item()) / N
    result = {"device": torch.cuda.get_device_name(0), "rows": N, "cols": K, "links": M // 2, "targets": M, "threshold": thr,
              "reps": args.reps, "memberships_per_node": members, "inside_share": args.inside, "torch_slab": args.torch_slab,
              "longest_row": int(rows.max()), "triangles": int(tri.sum()) // 3, "kernel": tr.kernel_name(), "median_s": med,
              "all_s": t, "torch_over_whole_call": med["torch_statement"] / med["whole_call"], "equal": equal}
    print(json.dumps(result), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
