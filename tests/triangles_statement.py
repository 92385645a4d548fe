"""The integer statement of include/ammsb_triangles.h, written once, in numpy: what test_triangles_host.py checks on the CPU
against powers of the dense adjacency and what triangles_child.py asserts the device equal to.  A plain module: numpy and
nothing of the package.

    M = pi >= np.float32(thr)
    for each a, for each b in row a:  C = (row a after b) & (row b)     (both ascending: the c > b that close a triangle)
        tri[a] += |C|;  m = M[a] & M[b] & M[C];  tri_in[a] += m.any(1).sum();  tk[a] += m.sum(0)
    tri_comms[a] = (tk[a] > 0).sum();  ktri3 += tk[a];  kpart += tk[a] > 0
    degree = the row's length; kmembers = M.sum(0); wedges[k] = the sum over the members a of k of C(c[a, k], 2) with
    c[a, k] = M[row a, k].sum()
"""
import numpy as np

NODE = ("tri", "tri_in", "tri_comms")
SUMS = ("ktri3", "kpart")


def members(pi, thr):
    return pi >= np.float32(thr)


def common(x, y):
    """two ascending arrays without repeats -> their common values, ascending"""
    if x.size > y.size:
        x, y = y, x
    if not x.size:
        return x
    at = np.minimum(np.searchsorted(y, x), y.size - 1)
    return x[y[at] == x]


def statement(M, off, tgt, first=0, count=None):
    """M [N, K] bool, a simple CSR -> name -> array: tri, tri_in, tri_comms, degree [count] uint32 of the nodes first ..
    first + count - 1; ktri3, kpart, kmembers, wedges over them as lists of Python ints; counts = [sum of tri, 0]"""
    N, K = M.shape
    count = N - first if count is None else count
    out = {n: np.zeros(count, np.uint32) for n in NODE + ("degree",)}
    ktri3, kpart = np.zeros(K, np.int64), np.zeros(K, np.int64)
    kmembers, wedges = np.zeros(K, np.int64), np.zeros(K, np.int64)
    rows = [tgt[int(off[a]):int(off[a + 1])].astype(np.int64) for a in range(N)]
    for i in range(count):
        a = first + i
        R = rows[a]
        tk = np.zeros(K, np.int64)
        tri = tri_in = 0
        for j, b in enumerate(R.tolist()):
            C = common(R[j + 1:], rows[b])
            if not C.size:
                continue
            tri += C.size
            ab = M[a] & M[b]
            if ab.any():
                m = M[C] & ab
                tri_in += int(m.any(1).sum())
                tk += m.sum(0)
        out["tri"][i], out["tri_in"][i], out["tri_comms"][i], out["degree"][i] = tri, tri_in, (tk > 0).sum(), R.size
        ktri3 += tk
        kpart += tk > 0
        c = M[R].sum(0).astype(np.int64)
        kmembers += M[a]
        wedges += np.where(M[a], c * (c - 1) // 2, 0)
    out.update(ktri3=ktri3.tolist(), kpart=kpart.tolist(), kmembers=kmembers.tolist(), wedges=wedges.tolist(),
               counts=[int(out["tri"].astype(np.int64).sum()), 0])
    return out


def csr_of_pairs(pairs, N, lead=0):
    """unordered pairs of distinct nodes -> the simple CSR (offsets uint64 with offsets[0] = lead, targets uint32 with
    `lead` unused targets in front)"""
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    src, dst = np.concatenate((pairs[:, 0], pairs[:, 1])), np.concatenate((pairs[:, 1], pairs[:, 0]))
    keys = np.unique(src * N + dst)
    keys = keys[keys // N != keys % N]
    off = np.zeros(N + 1, np.uint64)
    off[0] = lead
    off[1:] = lead + np.cumsum(np.bincount(keys // N, minlength=N))
    return off, np.concatenate((np.full(lead, 0xFFFFFFFF, np.int64), keys % N)).astype(np.uint32)


def dense(off, tgt, N):
    A = np.zeros((N, N), np.int64)
    for a in range(N):
        A[a, tgt[int(off[a]):int(off[a + 1])].astype(np.int64)] = 1
    return A
