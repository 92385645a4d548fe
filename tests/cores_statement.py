"""The definitions of include/ammsb_cores.h once, in numpy and plain Python: the simple symmetric adjacency of a key list, the
memberships numbered node by node ("slots"), the induced slot graph (indeg, nbr_off, nbr), the core numbers by the bucket
peeling of Batagelj and Zaversnik over that graph, and the integers per community and per node that follow.
test_cores_host.py checks it against the definition itself (definitional(): for each c, delete the vertices of degree < c of
the dense induced adjacency until nothing changes); the device tests assert every integer equal to it."""
import numpy as np

PER_COMMUNITY = ("members", "inlinks2", "degeneracy", "nucleus", "isolated")
PER_SLOT = ("community", "indeg", "core")
PER_NODE = ("best_core", "best_comm", "in_nucleus")


def members(pi, thr):
    """-> [N, K] bool: pi[a, k] >= thr as a binary32 compare (a NaN is never a member)"""
    with np.errstate(invalid="ignore"):
        return np.asarray(pi, dtype=np.float32) >= np.float32(thr)


def simple_csr(keys, N):
    """keys (a << 32) | b -> (offsets [N + 1] uint64, targets uint32, skipped, dropped): both directions of every key with
    both ends < N, rows strictly ascending, no loops, no repeats; skipped counts the keys with an end >= N, dropped the
    repeats (in either order) and the loops"""
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N)
    a, b = a[ok], b[ok]
    both = np.unique(np.concatenate(((a << 32) | b, (b << 32) | a)))
    both = both[(both >> 32) != (both & 0xFFFFFFFF)]
    offsets = np.zeros(N + 1, np.uint64)
    offsets[1:] = np.cumsum(np.bincount(both >> 32, minlength=N))
    return offsets, (both & 0xFFFFFFFF).astype(np.uint32), int(keys.size - a.size), int(a.size - both.size // 2)


def slot_graph(M, offsets, targets):
    """-> (base [N + 1] int64, slot_node, slot_comm, indeg [slots] int64, nbr_off [slots + 1] int64, nbr int64): the slot of
    (a, k) is base[a] + the rank of k in S_a; row s = (a, k) of nbr lists the slots of (b, k) for the b of a's row in k, in
    the order of that row"""
    M = np.asarray(M, dtype=bool)
    N = M.shape[0]
    base = np.zeros(N + 1, np.int64)
    base[1:] = np.cumsum(M.sum(axis=1, dtype=np.int64))
    slot_node, slot_comm = np.nonzero(M)            # (row-major: node by node, the communities of a node ascending)
    rank = np.cumsum(M, axis=1, dtype=np.int64) - 1
    off = np.asarray(offsets).astype(np.int64)
    src = np.repeat(np.arange(N), np.diff(off))
    dst = np.asarray(targets).astype(np.int64)
    s_rows, t_rows = [], []
    for lo in range(0, src.size, 1 << 14):          # (directed link, shared community), link by link, communities ascending
        u, v = src[lo:lo + (1 << 14)], dst[lo:lo + (1 << 14)]
        at, k = np.nonzero(M[u] & M[v])
        s_rows.append(base[u[at]] + rank[u[at], k])
        t_rows.append(base[v[at]] + rank[v[at], k])
    s = np.concatenate(s_rows) if s_rows else np.zeros(0, np.int64)
    t = np.concatenate(t_rows) if t_rows else np.zeros(0, np.int64)
    order = np.argsort(s, kind="stable")            # (stable: a row keeps the order of the node's row of targets)
    slots = int(base[-1])
    indeg = np.bincount(s, minlength=slots).astype(np.int64)
    nbr_off = np.zeros(slots + 1, np.int64)
    nbr_off[1:] = np.cumsum(indeg)
    return base, slot_node, slot_comm, indeg, nbr_off, t[order]


def peel(indeg, nbr_off, nbr):
    """core numbers by bucket peeling (Batagelj and Zaversnik, 2003): the vertices in bins by degree, the one of the smallest
    degree leaves and every neighbour of a larger degree moves one bin down.  A row is (nbr_off[s], indeg[s])"""
    n = len(indeg)
    deg = [int(d) for d in indeg]
    if not n:
        return np.zeros(0, np.int64)
    off, nb = [int(x) for x in nbr_off], [int(x) for x in nbr]
    md = max(deg)
    start = [0] * (md + 2)
    for d in deg:
        start[d + 1] += 1
    for d in range(1, md + 2):
        start[d] += start[d - 1]
    place, pos, vert = start[:md + 1], [0] * n, [0] * n
    for v in range(n):
        pos[v] = place[deg[v]]
        vert[pos[v]] = v
        place[deg[v]] += 1
    rows = [int(d) for d in indeg]
    for i in range(n):
        v = vert[i]
        for u in nb[off[v]:off[v] + rows[v]]:
            if deg[u] > deg[v]:
                du, pu = deg[u], pos[u]
                pw = start[du]
                w = vert[pw]
                if u != w:
                    pos[u], pos[w], vert[pu], vert[pw] = pw, pu, w, u
                start[du] += 1
                deg[u] -= 1
    return np.asarray(deg, dtype=np.int64)


def summarise(N, K, base, slot_comm, indeg, core):
    """the K- and N-sized integers of the header from the slots"""
    slot_comm, indeg, core = (np.asarray(x).astype(np.int64) for x in (slot_comm, indeg, core))
    out = {"members": np.bincount(slot_comm, minlength=K).astype(np.uint64)}
    inl = np.zeros(K, np.uint64)
    np.add.at(inl, slot_comm, indeg.astype(np.uint64))
    out["inlinks2"] = inl
    top = np.zeros(K, np.int64)
    np.maximum.at(top, slot_comm, core)
    out["degeneracy"] = top.astype(np.uint32)
    out["nucleus"] = np.bincount(slot_comm[core == top[slot_comm]], minlength=K).astype(np.uint64)
    out["isolated"] = np.bincount(slot_comm[core == 0], minlength=K).astype(np.uint64)
    best_core, best_comm, inner = np.zeros(N, np.uint32), np.full(N, -1, np.int32), np.zeros(N, np.uint32)
    for a in range(N):
        lo, hi = int(base[a]), int(base[a + 1])
        if hi > lo:
            c = core[lo:hi]
            j = int(np.argmax(c))                   # (the first of the largest: the lowest community)
            best_core[a], best_comm[a] = c[j], slot_comm[lo + j]
            t = top[slot_comm[lo:hi]]
            inner[a] = int(((t > 0) & (c == t)).sum())
    out["best_core"], out["best_comm"], out["in_nucleus"] = best_core, best_comm, inner
    return out


def statement(M, keys):
    """M: [N, K] bool memberships; keys: (a << 32) | b -> name -> value: offsets [N + 1] uint64; community uint16, indeg, core
    uint32 [slots]; nbr_off [slots + 1] uint64, nbr uint32 [L]; members, inlinks2, nucleus, isolated uint64, degeneracy uint32
    [K]; best_core, in_nucleus uint32, best_comm int32 [N]; M, L, skipped, dropped ints; csr = (offsets, targets) of the
    simple adjacency"""
    M = np.asarray(M, dtype=bool)
    N, K = M.shape
    offsets, targets, skipped, dropped = simple_csr(keys, N)
    base, slot_node, slot_comm, indeg, nbr_off, nbr = slot_graph(M, offsets, targets)
    core = peel(indeg, nbr_off, nbr)
    out = summarise(N, K, base, slot_comm, indeg, core)
    out.update({"offsets": base.astype(np.uint64), "community": slot_comm.astype(np.uint16), "indeg": indeg.astype(np.uint32),
                "core": core.astype(np.uint32), "nbr_off": nbr_off.astype(np.uint64), "nbr": nbr.astype(np.uint32),
                "M": int(base[-1]), "L": int(nbr_off[-1]), "skipped": skipped, "dropped": dropped, "csr": (offsets, targets)})
    return out


def result_of(co, thr, base):
    """the statement's integers as a _cores.Cores"""
    return co.Cores(thr, base["members"], base["inlinks2"], base["degeneracy"], base["nucleus"], base["isolated"], base["offsets"],
                    base["community"], base["indeg"], base["core"], base["best_core"], base["best_comm"], base["in_nucleus"],
                    base["skipped"], base["dropped"])


def definitional(M, keys):
    """the core numbers from the definition, for small shapes: per community the dense adjacency induced on its members; for
    c = 1, 2, ... delete the vertices of degree < c until nothing changes, and whoever is left has core >= c
    -> per community {member: core}"""
    M = np.asarray(M, dtype=bool)
    N, K = M.shape
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1)
    a, b = (keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (a < N) & (b < N) & (a != b)
    A = np.zeros((N, N), bool)
    A[a[ok], b[ok]] = A[b[ok], a[ok]] = True
    out = []
    for k in range(K):
        ids = np.flatnonzero(M[:, k])
        sub = A[np.ix_(ids, ids)]
        core = np.zeros(ids.size, np.int64)
        alive = np.ones(ids.size, bool)
        c = 1
        while alive.any():
            while True:
                d = (sub & alive[None, :]).sum(axis=1)
                weak = alive & (d < c)
                if not weak.any():
                    break
                alive &= ~weak
            core[alive] = c
            c += 1
        out.append({int(ids[i]): int(core[i]) for i in range(ids.size)})
    return out
