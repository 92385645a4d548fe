#!/usr/bin/env python3
"""The community cores at C3's shape -- N = 10^6, K = 1024, three memberships per node, an assortative list of about 16
10^6 links -- alternating in one process: the device pass (mask, own, base, slots of libammsb_components.so, then degrees,
adjacency, the peel and finish of libammsb_cores.so) against the same statement in torch / numpy (the induced slot graph by
a sort of (directed link, shared community) pairs, then a round-synchronous peel: the slots of degree <= level leave, an
index_add_ lowers their neighbours), medians over the repeats, and equal integers asserted (core per slot, degeneracy and
nucleus per community).  Needs a GPU.  Writes profiles/cores_ab.json.

    python tools/cores_ab.py [--n 1000000] [--k 1024] [--links 16000000] [--repeats 3] [--out profiles/cores_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tools.components_ab import make_case  # noqa: E402


def torch_cores(torch, comm, offsets, targets, N, K):
    """-> (core per slot int64, the slot -> community map) by the statement, on the device in torch: the slots are (node, its
    sorted distinct communities); a directed link (a, b) and a community both hold give one entry of the slot graph"""
    dev = offsets.device
    comm = torch.sort(torch.as_tensor(comm, device=dev), 1).values
    fresh = torch.ones_like(comm, dtype=torch.bool)
    fresh[:, 1:] = comm[:, 1:] != comm[:, :-1]
    own = fresh.sum(1)
    base = torch.zeros(N + 1, dtype=torch.int64, device=dev)
    base[1:] = torch.cumsum(own, 0)
    rank = torch.cumsum(fresh, 1) - 1
    slot_of = base[:-1, None] + rank                       # [N, 3]: the slot of every listed membership
    slot_comm = torch.empty(int(base[-1]), dtype=torch.int64, device=dev)
    slot_comm[slot_of[fresh]] = comm[fresh]
    src = torch.repeat_interleave(torch.arange(N, device=dev), offsets[1:] - offsets[:-1])
    dst = targets.to(torch.int64) & 0xFFFFFFFF
    s_all, t_all = [], []
    for i in range(comm.shape[1]):
        for j in range(comm.shape[1]):
            hit = fresh[src, i] & fresh[dst, j] & (comm[src, i] == comm[dst, j])
            s_all.append(slot_of[src[hit], i])
            t_all.append(slot_of[dst[hit], j])
    s, t = torch.cat(s_all), torch.cat(t_all)
    M = int(base[-1])
    deg = torch.bincount(s, minlength=M)
    core = torch.zeros(M, dtype=torch.int64, device=dev)
    alive = torch.ones(M, dtype=torch.bool, device=dev)
    level = 0
    while bool(alive.any()):
        level = max(level, int(deg[alive].min()))
        while True:
            out = alive & (deg <= level)
            if not bool(out.any()):
                break
            core[out] = level
            alive &= ~out
            hit = out[s] & alive[t]
            deg.index_add_(0, t[hit], torch.full((int(hit.sum()),), -1, dtype=torch.int64, device=dev))
        level += 1
    return core, slot_comm


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--links", type=int, default=16_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cores_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("cores_ab.py needs a HIP device")
    N, K = args.n, args.k
    comm, keys = make_case(N, K, args.links, 7)
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    pi = ops.RowPartitionedMatrix(ctx, N, K)
    pi.blocks[0].zero_()
    pi.blocks[0][torch.arange(N, device="cuda")[:, None], ctx.from_numpy(comm)] = 0.3
    # the simple adjacency, once, as Learner._simple_csr builds it
    k = ctx.from_numpy(keys)
    a, b = (k >> 32) & 0xFFFFFFFF, k & 0xFFFFFFFF
    both = torch.unique(torch.cat(((a << 32) | b, (b << 32) | a)))
    both = both[(both >> 32) != (both & 0xFFFFFFFF)]
    offsets = torch.zeros(N + 1, dtype=torch.int64, device="cuda")
    offsets[1:] = torch.cumsum(torch.bincount(both >> 32, minlength=N), 0)
    targets = (both & 0xFFFFFFFF).to(torch.int32).contiguous()
    op = ops.CommunityCores(ctx)
    device_ms, torch_ms, out = [], [], None
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = op.run(pi, 0.05, offsets, targets)
        torch.cuda.synchronize()
        device_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        want, slot_comm = torch_cores(torch, comm, offsets, targets, N, K)
        torch.cuda.synchronize()
        torch_ms.append(1e3 * (time.perf_counter() - t0))
    st, _, M, dev_comm, indeg = out[:5]
    assert torch.equal(st["deg"].to(torch.int64) & 0xFFFFFFFF, want), "the device pass differs from the statement"
    assert torch.equal(dev_comm.to(torch.int64) & 0xFFFF, slot_comm)
    top = torch.zeros(K, dtype=torch.int64, device="cuda").scatter_reduce_(0, slot_comm, want, "amax")
    assert torch.equal(st["degeneracy"].to(torch.int64), top)
    assert torch.equal(st["nucleus"], torch.bincount(slot_comm[want == top[slot_comm]], minlength=K))
    counts = st["counts"].cpu().numpy().tolist()
    res = {"N": N, "K": K, "links": int(keys.size), "slots": int(M), "entries": counts[1], "scans": counts[2], "rounds": counts[3],
           "degeneracy_max": int(top.max()), "repeats": args.repeats, "device_ms_median": float(np.median(device_ms)),
           "torch_ms_median": float(np.median(torch_ms)), "ratio": float(np.median(torch_ms) / np.median(device_ms)),
           "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
