"""The definitions of include/ammsb_components.h once, in numpy and plain Python: the memberships numbered node by node
("slots"), a sequential union-find over (key, shared community) in the order of the list, roots as minimum node ids, and
the integers per slot, per community and per node that follow.  test_components_host.py checks it against reachability by
boolean powers of the dense induced adjacency; the device tests assert every integer equal to it."""
import numpy as np

PER_COMMUNITY = ("members", "components", "largest", "largest_root", "singletons")
PER_SLOT = ("community", "root", "size")
COUNTS = ("links", "skipped", "shared")


def members(pi, thr):
    """-> [N, K] bool: pi[a, k] >= thr as a binary32 compare (a NaN is never a member)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(pi, dtype=np.float32) >= np.float32(thr)


def statement(M, keys):
    """M: [N, K] bool memberships; keys: (a << 32) | b -> name -> value: offsets [N + 1] uint64; community uint16, root,
    size uint32 [slots]; members, components, singletons uint64, largest uint32, largest_root int32 [K]; stray [N] uint32;
    links, skipped, shared ints"""
    M = np.asarray(M, dtype=bool)
    N, K = M.shape
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N)
    a, b = a[ok], b[ok]
    offsets = np.zeros(N + 1, np.int64)
    offsets[1:] = np.cumsum(M.sum(axis=1, dtype=np.int64))
    slots = int(offsets[-1])
    slot_node, slot_comm = np.nonzero(M)            # (row-major: node by node, the communities of a node ascending)
    rank = np.cumsum(M, axis=1, dtype=np.int32) - 1   # rank[a, k]: the place of k in S_a where k is in it
    parent = list(range(slots))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    shared = 0
    for lo in range(0, a.size, 4096):               # (key, shared community) in the order of the list
        both = M[a[lo:lo + 4096]] & M[b[lo:lo + 4096]]
        at, k = np.nonzero(both)
        shared += at.size
        sa = (offsets[a[lo + at]] + rank[a[lo + at], k]).tolist()
        sb = (offsets[b[lo + at]] + rank[b[lo + at], k]).tolist()
        for x, y in zip(sa, sb):
            x, y = find(x), find(y)
            if x != y:
                parent[max(x, y)] = min(x, y)
    root_slot = np.array([find(s) for s in range(slots)], dtype=np.int64)
    root = slot_node[root_slot].astype(np.int64) if slots else np.zeros(0, np.int64)
    per_root = np.bincount(root_slot, minlength=slots)
    size = per_root[root_slot] if slots else np.zeros(0, np.int64)
    # (slots ascend with the nodes, so the smallest slot of a component is that of its smallest node)
    heads = np.flatnonzero(per_root > 0)
    hk, hsize, hroot = slot_comm[heads], per_root[heads], slot_node[heads]
    out = {"offsets": offsets.astype(np.uint64), "community": slot_comm.astype(np.uint16), "root": root.astype(np.uint32),
           "size": size.astype(np.uint32)}
    out["members"] = M.sum(axis=0, dtype=np.uint64)
    out["components"] = np.bincount(hk, minlength=K).astype(np.uint64)
    out["singletons"] = np.bincount(hk[hsize == 1], minlength=K).astype(np.uint64)
    largest, largest_root = np.zeros(K, np.uint32), np.full(K, -1, np.int32)
    for i in np.lexsort((-hroot, hsize, hk)):       # per community size ascending, equal sizes by root descending: the last wins
        largest[hk[i]], largest_root[hk[i]] = hsize[i], hroot[i]
    out["largest"], out["largest_root"] = largest, largest_root
    out["stray"] = np.bincount(slot_node[root != largest_root[slot_comm]], minlength=N).astype(np.uint32)
    out["links"], out["skipped"], out["shared"] = int(a.size), int(keys.size - a.size), int(shared)
    return out


def result_of(cc, thr, base):
    """the statement's integers as a _components.Components"""
    return cc.Components(thr, base["members"], base["components"], base["largest"], base["largest_root"], base["singletons"],
                         base["offsets"], base["community"], base["root"], base["size"], base["stray"], base["links"],
                         base["skipped"], base["shared"])


def reachability(M, keys):
    """the same components another way, for small shapes: per community the dense adjacency induced on its members, with
    loops, squared as a boolean matrix until it no longer grows -> per community {member: (root, size)}"""
    M = np.asarray(M, dtype=bool)
    N, K = M.shape
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N)
    A = np.zeros((N, N), bool)
    A[a[ok], b[ok]] = A[b[ok], a[ok]] = True
    out = []
    for k in range(K):
        ids = np.flatnonzero(M[:, k])
        R = A[np.ix_(ids, ids)] | np.eye(ids.size, dtype=bool)
        while True:
            R2 = (R.astype(np.int32) @ R.astype(np.int32)) > 0
            if np.array_equal(R2, R):
                break
            R = R2
        out.append({int(ids[i]): (int(ids[np.flatnonzero(R[i])[0]]), int(R[i].sum())) for i in range(ids.size)})
    return out
