#!/usr/bin/env python3
"""The community components at C3's shape -- N = 10^6, K = 1024, three memberships per node, an assortative list of about
16 10^6 links -- alternating in one process: the device pass (mask, own, base, slots, edges, finish of
libammsb_components.so) against the statement per community on the host (scipy.sparse.csgraph.connected_components on the
induced subgraph where scipy is importable, else a numpy label propagation by minimum), medians over the repeats, and
equal integers asserted (components, largest, singletons per community).  Needs a GPU.  Writes profiles/components_ab.json.

    python tools/components_ab.py [--n 1000000] [--k 1024] [--links 16000000] [--repeats 5] [--out profiles/components_ab.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_case(N, K, links, seed):
    """three memberships per node, the first by blocks of consecutive nodes; links mostly inside a block of 64 nodes"""
    rng = np.random.default_rng(seed)
    comm = np.stack((np.arange(N) * K // N, rng.integers(0, K, N), rng.integers(0, K, N)), 1)
    a = rng.integers(0, N, links)
    near = rng.random(links) < 0.9
    b = np.where(near, np.minimum(a + rng.integers(1, 64, links), N - 1), rng.integers(0, N, links))
    return comm, (a.astype(np.uint64) << np.uint64(32)) | b.astype(np.uint64)


def host_components(comm, keys, N, K):
    """-> (components, largest, singletons) [K] by the statement, community by community"""
    try:
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        coo_matrix = connected_components = None
    M = np.zeros((N, K), bool)
    M[np.arange(N)[:, None], comm] = True
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    out = np.zeros((3, K), np.int64)
    for k in range(K):
        ids = np.flatnonzero(M[:, k])
        if not ids.size:
            continue
        new = np.full(N, -1, np.int64)
        new[ids] = np.arange(ids.size)
        keep = M[a, k] & M[b, k]
        u, v = new[a[keep]], new[b[keep]]
        if connected_components is not None:
            _, label = connected_components(coo_matrix((np.ones(u.size, bool), (u, v)), shape=(ids.size, ids.size)), directed=False)
        else:
            label = np.arange(ids.size)
            while True:
                low = np.minimum(label[u], label[v])
                nxt = label.copy()
                np.minimum.at(nxt, u, low)
                np.minimum.at(nxt, v, low)
                nxt = nxt[nxt]
                if np.array_equal(nxt, label):
                    break
                label = nxt
        sizes = np.bincount(np.unique(label, return_inverse=True)[1])
        out[:, k] = sizes.size, sizes.max(), int((sizes == 1).sum())
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--k", type=int, default=1024)
    ap.add_argument("--links", type=int, default=16_000_000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "components_ab.json"))
    args = ap.parse_args()
    import torch
    import __graft_entry__ as ge
    ge.build()
    from mcmc_ammsb_gpu_amd import ops
    if not torch.cuda.is_available():
        raise SystemExit("components_ab.py needs a HIP device")
    N, K = args.n, args.k
    comm, keys = make_case(N, K, args.links, 7)
    ctx = ops.Context(ops.make_params(1024, 32, E=1024))
    pi = ops.RowPartitionedMatrix(ctx, N, K)
    pi.blocks[0].zero_()
    pi.blocks[0][torch.arange(N, device="cuda")[:, None], ctx.from_numpy(comm)] = 0.3
    op = ops.CommunityComponents(ctx)
    d_keys = ctx.from_numpy(keys)
    device_ms, host_ms, st = [], [], None
    for _ in range(args.repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        st, _, M = op.run(pi, 0.05, d_keys)
        torch.cuda.synchronize()
        device_ms.append(1e3 * (time.perf_counter() - t0))
        t0 = time.perf_counter()
        want = host_components(comm, keys, N, K)
        host_ms.append(1e3 * (time.perf_counter() - t0))
    got = np.stack([st[n].cpu().numpy().astype(np.int64) for n in ("components", "largest", "singletons")])
    assert np.array_equal(got, want), "the device pass differs from the statement"
    assert st["counts"].cpu().numpy().tolist()[3] == 0
    res = {"N": N, "K": K, "links": int(keys.size), "slots": int(M), "repeats": args.repeats,
           "device_ms_median": float(np.median(device_ms)), "host_ms_median": float(np.median(host_ms)),
           "ratio": float(np.median(host_ms) / np.median(device_ms)), "device": torch.cuda.get_device_name(0)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
