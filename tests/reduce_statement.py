"""The numpy statement of include/ammsb_reduce.h, stated once: test_reduce_host.py checks it against the dense float64
definition, reduce_child.py asserts the device's results equal to it bit for bit.  Plans come in as the map[K] of the header
(-1: dropped); every function builds the inverse CSR itself, so nothing here depends on the package."""
import numpy as np

F32, F64 = np.float32, np.float64
ULP24 = 2.0 ** -24


def csr(map_):
    """-> (src_off [K' + 1], src): the sources of each new community, ascending"""
    m = np.asarray(map_, dtype=np.int64)
    kept = np.flatnonzero(m >= 0)
    new_K = int(m.max()) + 1
    order = kept[np.argsort(m[kept], kind="stable")]
    off = np.zeros(new_K + 1, np.int64)
    off[1:] = np.cumsum(np.bincount(m[kept], minlength=new_K))
    assert (np.diff(off) >= 1).all(), "a new community without a source"
    return off, order


def merged(x, map_):
    """x [n, K] float32 -> t [n, K'] float32: per new community the left-to-right binary32 sum of its sources' columns,
    ascending; one source is a copy of its bits"""
    off, src = csr(map_)
    x = np.ascontiguousarray(x, dtype=F32)
    n_src = np.diff(off)
    t = x[:, src[off[:-1]]].copy()
    with np.errstate(all="ignore"):
        for i in range(1, int(n_src.max())):
            cols = np.flatnonzero(n_src > i)
            t[:, cols] = t[:, cols] + x[:, src[off[cols] + i]]      # float32 + float32, rounded once
    return t


def lane_sum(t):
    """t [n, K'] float32 -> s [n] float64: virtual lane v adds the columns v, v + 64, ... ascending into a binary64 0,
    then six halving adds x[v] = x[v] + x[v + d], d = 32 .. 1"""
    n, K2 = t.shape
    rows = -(-K2 // 64)
    pad = np.zeros((n, rows * 64), F64)
    pad[:, :K2] = t
    with np.errstate(all="ignore"):
        x = np.zeros((n, 64), F64)
        for r in range(rows):                          # row by row: lane v meets its columns in ascending order
            x = x + pad[:, 64 * r:64 * r + 64]
        for d in (32, 16, 8, 4, 2, 1):
            x = x[:, :d] + x[:, d:2 * d]
    return x[:, 0]


def rows(pi, phi_sum, map_):
    """-> (pi' [n, K'] float32, phi_sum' [n] float32, emptied rows as a bool vector)"""
    m = np.asarray(map_, dtype=np.int64)
    t = merged(pi, m)
    phi_sum = np.ascontiguousarray(phi_sum, dtype=F32)
    if not (m < 0).any():
        return t, phi_sum.copy(), np.zeros(t.shape[0], bool)
    with np.errstate(all="ignore"):
        sf = lane_sum(t).astype(F32)
        emptied = ~(sf > 0)
        out = t / sf[:, None]
        out[emptied] = F32(1.0) / F32(t.shape[1])
        phi = phi_sum * sf
        phi[emptied] = phi_sum[emptied]
    return out.astype(F32), phi.astype(F32), emptied


def theta(th, map_):
    """th [K, 2] float32 -> [K', 2]"""
    return np.ascontiguousarray(merged(np.ascontiguousarray(th, dtype=F32).reshape(-1, 2).T, map_).T)


def dense(pi, map_):
    """the float64 definition: P = pi64 @ A, rows divided by their sum when the plan drops -> (P, n_j)"""
    m = np.asarray(map_, dtype=np.int64)
    K, new_K = m.size, int(m.max()) + 1
    A = np.zeros((K, new_K))
    A[np.flatnonzero(m >= 0), m[m >= 0]] = 1.0
    P = np.asarray(pi, dtype=F64) @ A
    if (m < 0).any():
        P = P / P.sum(1, keepdims=True)
    return P, A.sum(0)
