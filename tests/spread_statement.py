"""The numpy statement of include/ammsb_spread.h: the four entry points in the binary32 / binary64 operations the header
names, one numpy operation each, so that the device's results can be asserted bit for bit.  And the dense variance the lazy
one stands for, in float64, with the bound the header derives between the two.  test_spread_host.py checks the statement
against the definition on the CPU; spread_child.py asserts the device's results equal to it."""
import numpy as np

from average_statement import claimed

F32, F64 = np.float32, np.float64


def bound_var(F):
    """|var - exact variance of the samples| after F data-writing flushes of a row (n <= 2^24): the header's
    13 F 2^-24 + F^2 2^-43"""
    F = np.asarray(F, dtype=F64)
    return 13.0 * F * 2.0 ** -24 + F * F * 2.0 ** -43


def rows(pi, mean, var, last, n, nodes=None, first=0, count=None):
    """ammsb_spread_rows, in place on mean, var [N, K] float32 and last [N] uint32 -> the rows whose data was written"""
    N = pi.shape[0]
    assert pi.dtype == F32 and mean.dtype == F32 and var.dtype == F32 and last.dtype == np.uint32
    assert mean.shape == pi.shape == var.shape
    if nodes is None:
        count = N - first if count is None else count
        assert first + count <= N
        ids = np.arange(first, first + count, dtype=np.int64)
        if n == 0:
            return ids[:0]
    else:
        assert n >= 1 and first == 0
        ids = claimed(nodes if count is None else np.asarray(nodes)[:count], N)
    old = last[ids]
    last[ids] = n
    w = np.uint32(n) - old                      # (n >= old is the caller's side of the contract)
    copy, fold = ids[(w != 0) & (old == 0)], ids[(w != 0) & (old != 0)]
    mean[copy] = pi[copy]                       # neither mean nor var is read: they may hold anything
    var[copy] = F32(0)
    if fold.size:
        with np.errstate(all="ignore"):
            r = (w[(w != 0) & (old != 0)].astype(F32) / F32(n))[:, None]                # r = float(w) / float(n)
            d = pi[fold] - mean[fold]                                                   # d = pi - mean
            mean[fold] = mean[fold] + r * d                                             # mean' = mean + r * d
            s = F32(1) - r                                                              # s = 1 - r
            e = d * d                                                                   # e = d * d
            e = e * s                                                                   # e = e * s
            e = e - var[fold]                                                           # e = e - var
            e = r * e                                                                   # e = r * e
            var[fold] = var[fold] + e                                                   # var' = var + e
        assert r.dtype == F32 and e.dtype == F32
    return np.concatenate([copy, fold])


def vector(x, mean64, m2, n):
    """ammsb_spread_vector, in place on mean64 and m2 [len] float64"""
    assert x.dtype == F32 and mean64.dtype == F64 and m2.dtype == F64 and n >= 1
    v = x.astype(F64)
    if n == 1:
        mean64[:] = v
        m2[:] = 0.0
    else:
        delta = v - mean64
        mean64[:] = mean64 + delta / F64(n)
        m2[:] = m2 + delta * (v - mean64)


def bound(mean, var, z):
    """ammsb_spread_bound -> out float32: min(1, max(0, mean + z sqrt(var))), a NaN -> 0"""
    assert mean.dtype == F32 and var.dtype == F32 and np.isfinite(z)
    with np.errstate(all="ignore"):
        t = mean + F32(z) * np.sqrt(var)          # numpy's float32 sqrt is the correctly rounded one
        out = np.where(t > 0, np.minimum(t, F32(1)), F32(0)).astype(F32)
    assert t.dtype == F32
    return out


def rowsum(var):
    """ammsb_spread_rowsum: var [n, K] float32 -> [n] float64: virtual lane v adds the columns v, v + 64, ... ascending
    into a binary64 0, then six halving adds x[v] = x[v] + x[v + d], d = 32 .. 1 (reduce_statement.lane_sum's order)"""
    n, K = var.shape
    trips = -(-K // 64)
    pad = np.zeros((n, trips * 64), F64)
    pad[:, :K] = var
    with np.errstate(all="ignore"):
        x = np.zeros((n, 64), F64)
        for t in range(trips):
            x = x + pad[:, 64 * t:64 * t + 64]
        for d in (32, 16, 8, 4, 2, 1):
            x = x[:, :d] + x[:, d:2 * d]
    return x[:, 0]


class Lazy:
    """the state a caller keeps, and the calls a loop makes around an iteration"""

    def __init__(self, N, K, B):
        self.mean, self.var = np.full((N, K), np.nan, F32), np.full((N, K), np.nan, F32)
        self.last = np.zeros(N, np.uint32)
        self.beta64, self.m2 = np.full(B, np.nan, F64), np.full(B, np.nan, F64)
        self.n = 0
        self.flushes = np.zeros(N, np.int64)     # data-writing flushes per row: the F of the bound

    def before(self, pi, nodes):
        """the iteration is about to overwrite the rows `nodes`"""
        if self.n:
            self.flushes[rows(pi, self.mean, self.var, self.last, self.n, nodes=nodes)] += 1

    def after(self, beta):
        """the iteration is over: (pi, beta) are sample n + 1"""
        self.n += 1
        vector(beta, self.beta64, self.m2, self.n)

    def read(self, pi, slabs=1):
        """-> (mean, var) with every row flushed"""
        N = pi.shape[0]
        cuts = np.linspace(0, N, slabs + 1).astype(np.int64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            self.flushes[rows(pi, self.mean, self.var, self.last, self.n, first=int(lo), count=int(hi - lo))] += 1
        return self.mean, self.var


class Dense:
    """every sample kept, in float64"""

    def __init__(self):
        self.pi, self.beta = [], []

    def after(self, pi, beta):
        self.pi.append(pi.astype(F64))
        self.beta.append(beta.astype(F64))

    def read(self):
        """-> (mean pi, var pi, mean beta, var beta): population variances"""
        p, b = np.stack(self.pi), np.stack(self.beta)
        return p.mean(0), p.var(0), b.mean(0), b.var(0)
