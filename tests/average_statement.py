"""The numpy statement of include/ammsb_average.h: the three entry points in the binary32 / binary64 operations the header
names, one numpy operation each, so that the device's results can be asserted bit for bit.  And the dense mean the lazy one
stands for, in float64, with the bound between the two."""
import numpy as np

ULP22 = 2.0 ** -22   # one flush moves a stored mean of values in [0, 1] by at most 4 * 2^-24 beside the exact recurrence


def claimed(nodes, N):
    """the rows a node list flushes: every id < N once (the first claimant flushes, the others see w == 0)"""
    nodes = np.asarray(nodes, dtype=np.uint32).astype(np.int64)
    return np.unique(nodes[nodes < N])


def rows(pi, mean, last, n, nodes=None, first=0, count=None):
    """ammsb_average_rows, in place on mean [N, K] float32 and last [N] uint32 -> the rows whose data was written"""
    N = pi.shape[0]
    assert pi.dtype == np.float32 and mean.dtype == np.float32 and last.dtype == np.uint32 and mean.shape == pi.shape
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
    mean[copy] = pi[copy]                       # mean is not read: it may hold anything
    if fold.size:
        r = w[(w != 0) & (old != 0)].astype(np.float32) / np.float32(n)                 # one divide
        d = pi[fold] - mean[fold]                                                       # one subtract
        mean[fold] = mean[fold] + r[:, None] * d                                        # one multiply, one add
    return np.concatenate([copy, fold])


def vector(x, mean64, n):
    """ammsb_average_vector, in place on mean64 [len] float64"""
    assert x.dtype == np.float32 and mean64.dtype == np.float64 and n >= 1
    if n == 1:
        mean64[:] = x.astype(np.float64)
    else:
        mean64[:] = mean64 + (x.astype(np.float64) - mean64) / np.float64(n)


def rounded(mean64):
    """ammsb_average_round"""
    return mean64.astype(np.float32)


class Lazy:
    """the state a caller keeps, and the calls a loop makes around an iteration"""

    def __init__(self, N, K, B, garbage=True):
        self.mean = np.full((N, K), np.nan, np.float32) if garbage else np.zeros((N, K), np.float32)
        self.last = np.zeros(N, np.uint32)
        self.beta64 = np.full(B, np.nan, np.float64)
        self.n = 0
        self.flushes = np.zeros(N, np.int64)     # data-writing flushes per row: the F of the bound

    def before(self, pi, nodes):
        """the iteration is about to overwrite the rows `nodes`"""
        if self.n:
            self.flushes[rows(pi, self.mean, self.last, self.n, nodes=nodes)] += 1

    def after(self, beta):
        """the iteration is over: (pi, beta) are sample n + 1"""
        self.n += 1
        vector(beta, self.beta64, self.n)

    def read(self, pi, slabs=1):
        """-> (mean, beta32) with every row flushed"""
        N = pi.shape[0]
        cuts = np.linspace(0, N, slabs + 1).astype(np.int64)
        for lo, hi in zip(cuts[:-1], cuts[1:]):
            self.flushes[rows(pi, self.mean, self.last, self.n, first=int(lo), count=int(hi - lo))] += 1
        return self.mean, rounded(self.beta64)


class Dense:
    """the mean of every sample, in float64"""

    def __init__(self, N, K, B):
        self.pi, self.beta, self.n = np.zeros((N, K), np.float64), np.zeros(B, np.float64), 0

    def after(self, pi, beta):
        self.pi += pi
        self.beta += beta
        self.n += 1

    def read(self):
        return self.pi / self.n, self.beta / self.n
