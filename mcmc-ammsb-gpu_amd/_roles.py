"""ctypes view of libammsb_roles.so (include/ammsb_roles.h): how a single node sits in the detected cover -- per node of an
adjacency how many of its neighbours are in each community, reduced on the device to integers -- and the host-side helpers
that need no device: the derived measures (embeddedness, participation coefficient, within-community z-score), the node
roles read off them, and the roles text file.  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and
nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, _g9

MAX_COLS = 8192          # AMMSB_ROLES_MAX_COLS
W1_MAX_COLS = 4096       # AMMSB_ROLES_W1_MAX_COLS
MAX_TOP = 16             # AMMSB_ROLES_MAX_TOP
MAX_ROW = 2 ** 25        # AMMSB_ROLES_MAX_ROW
ALL, OWN = 0, 1          # AMMSB_ROLES_ALL, AMMSB_ROLES_OWN
AMONG = {"all": ALL, "own": OWN}

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_roles_nodes": (C.c_int, [_vp, _u64, _u32, _vp, _vp, _u64, _u64, _u32, _u32, _u32] + [_vp] * 14),
    "ammsb_roles_last_kernel_name": (C.c_char_p, []),
    "ammsb_roles_last_error": (C.c_char_p, []),
}

# every kernel the dispatcher of csrc/ammsb_roles.hip can launch
KERNEL_FORMS = ("roles_nodes_w1", "roles_nodes_w2")

_LIBRARY = PostfitLibrary("roles", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "node roles")


def check_top(top):
    """-> top, the slots kept per node: 1..16"""
    if isinstance(top, bool) or top != int(top) or not 1 <= int(top) <= MAX_TOP:
        raise AmmsbError("node roles: top must be in 1..%d, not %r" % (MAX_TOP, top))
    return int(top)


def check_among(among):
    """'all' or 'own' -> AMMSB_ROLES_ALL or AMMSB_ROLES_OWN"""
    if among not in AMONG:
        raise AmmsbError("node roles: among must be 'all' or 'own', not %r" % (among,))
    return AMONG[among]


def check_min_count(min_count):
    """-> min_count, a uint32"""
    if isinstance(min_count, bool) or min_count != int(min_count) or not 0 <= int(min_count) < 2 ** 32:
        raise AmmsbError("node roles: min_count must be in 0..2^32 - 1, not %r" % (min_count,))
    return int(min_count)


def check_nodes(nodes, N):
    """None or (first, count) -> (first, count) inside 0..N"""
    if nodes is None:
        return 0, int(N)
    try:
        first, count = (int(v) for v in nodes)
    except (TypeError, ValueError):
        raise AmmsbError("node roles: nodes must be (first, count), not %r" % (nodes,))
    if first < 0 or count < 0 or first + count > int(N):
        raise AmmsbError("node roles: the nodes %d .. %d are not inside 0 .. %d" % (first, first + count, int(N)))
    return first, count


def check_rows(longest):
    """-> the longest row of an adjacency, which must not be longer than 2^25 (squares is exact up to there)"""
    longest = int(longest)
    if longest > MAX_ROW:
        raise AmmsbError("node roles: a row of %d targets; the library takes rows of at most 2^25" % longest)
    return longest


def derive(degree, embedded, votes, squares, home, hcount, ksum, ksq, kmembers):
    """-> (embeddedness [n], participation [n], z [n, top]) in float64 from the integers, as the header states them: each
    integer converted once, then embedded / degree; 1 - squares / (votes votes); and per filled slot with k = home,
    n_k = kmembers[k] >= 2: mean = ksum[k] / n_k, var = ksq[k] / n_k - mean mean, z = (hcount - mean) / sqrt(var) where
    var > 0.  -1, -1 and 0 where they are not defined."""
    d, e = degree.astype(np.float64), embedded.astype(np.float64)
    v, s = votes.astype(np.float64), squares.astype(np.float64)
    emb, part = np.full(d.shape, -1.0), np.full(d.shape, -1.0)
    np.divide(e, d, out=emb, where=degree > 0)
    vv = v * v
    ratio = np.zeros(d.shape)
    np.divide(s, vv, out=ratio, where=votes > 0)
    part[votes > 0] = (1.0 - ratio)[votes > 0]
    z = np.zeros(home.shape, dtype=np.float64)
    if home.size:
        n = kmembers.astype(np.float64)
        mean, var = np.zeros(n.shape), np.zeros(n.shape)
        some = kmembers >= 2
        np.divide(ksum.astype(np.float64), n, out=mean, where=some)
        np.divide(ksq.astype(np.float64), n, out=var, where=some)
        var = var - mean * mean
        good = some & (var > 0)
        sigma = np.ones(n.shape)
        np.sqrt(var, out=sigma, where=good)
        k = np.where(home >= 0, home, 0)
        use = (home >= 0) & good[k]
        z[use] = ((hcount.astype(np.float64) - mean[k]) / sigma[k])[use]
    return emb, part, z


class Roles:
    """What Learner.NodeRoles returns, for the nodes first .. first + n - 1.  Integers, exact (include/ammsb_roles.h):
    degree, own, embedded, reached [n] uint32; votes, squares [n] uint64; home [n, top] int32, hcount [n, top] uint32,
    hflags [n] uint32; ksum, ksq, kmembers [K] uint64 (over these nodes); valid and skipped targets.  In float64 on the
    host: embeddedness, participation [n] and z [n, top]."""

    def __init__(self, threshold, among, top, min_count, degree, own, embedded, reached, votes, squares, home, hcount, hflags,
                 ksum, ksq, kmembers, valid, skipped, N=0, first=0):
        self.threshold, self.among, self.N, self.first = float(threshold), among, int(N), int(first)
        check_among(among)
        self.top, self.min_count = int(top), check_min_count(min_count)
        if not 0 <= self.top <= MAX_TOP:
            raise AmmsbError("node roles: top outside 0..16")
        self.valid, self.skipped = int(valid), int(skipped)
        u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)   # noqa: E731
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)   # noqa: E731
        try:
            self.degree, self.own, self.embedded, self.reached = u32(degree), u32(own), u32(embedded), u32(reached)
            self.votes, self.squares = u64(votes), u64(squares)
            self.ksum, self.ksq, self.kmembers = u64(ksum), u64(ksq), u64(kmembers)
            n = self.degree.size
            self.home = np.ascontiguousarray(home, dtype=np.int32).reshape(n, self.top)
            self.hcount = np.ascontiguousarray(hcount, dtype=np.uint32).reshape(n, self.top)
            self.hflags = u32(hflags) if self.top else np.zeros(n, dtype=np.uint32)
        except (OverflowError, ValueError, TypeError):
            raise AmmsbError("node roles: an array does not fit its type or the others' shape")
        K = self.ksum.size
        if any(x.size != n for x in (self.own, self.embedded, self.reached, self.votes, self.squares, self.hflags)) or \
                self.ksq.size != K or self.kmembers.size != K or min(self.valid, self.skipped, self.first) < 0:
            raise AmmsbError("node roles: the arrays do not fit each other, or a count is negative")
        if self.home.size and (self.home.min() < -1 or self.home.max() >= K):
            raise AmmsbError("node roles: a slot names no community")
        self.embeddedness, self.participation, self.z = derive(self.degree, self.embedded, self.votes, self.squares, self.home,
                                                               self.hcount, self.ksum, self.ksq, self.kmembers)

    def _ids(self, which):
        return (np.flatnonzero(which) + self.first).astype(np.int64)

    def hubs(self, z=2.5):
        """-> the nodes, ascending, with a filled slot whose community they belong to and a z-score >= z there"""
        mine = ((self.hflags[:, None] >> np.arange(self.top, dtype=np.uint32)[None, :]) & 1).astype(bool)
        return self._ids((mine & (self.home >= 0) & (self.z >= z)).any(axis=1))

    def connectors(self, p=0.62):
        """-> the nodes, ascending, whose participation coefficient is >= p"""
        return self._ids((self.votes > 0) & (self.participation >= p))

    def misplaced(self):
        """-> the nodes, ascending, with a neighbour, whose neighbourhood votes first for a community they are not in: slot
        0 filled and bit 0 of hflags clear"""
        if not self.top:
            return self._ids(np.zeros(self.degree.size, dtype=bool))
        return self._ids((self.degree > 0) & (self.home[:, 0] >= 0) & ((self.hflags & 1) == 0))

    def __repr__(self):
        return "Roles(n=%d, K=%d, threshold=%s, among=%s, top=%d)" % (self.degree.size, self.ksum.size,
                                                                       _g9(np.float32(self.threshold)), self.among, self.top)


# ---------------------------------------------------------------------------------------------- the text file
def write_roles(path, N, r):
    """A Roles as a text file, byte for byte what mcmc::Learner::WriteNodeRoles writes: `# N K M threshold among top min_count
    skipped` (M targets in the rows, `skipped` of them >= N), per community `c k members ksum ksq`, per node `n a degree own
    embedded reached votes squares nslots k0 c0 f0 ...` with the filled slots only.  Integers throughout."""
    with open(path, "w") as f:
        f.write("# %d %d %d %s %s %d %d %d\n" % (N, r.ksum.size, r.valid + r.skipped, _g9(np.float32(r.threshold)), r.among,
                                                 r.top, r.min_count, r.skipped))
        for k in range(r.ksum.size):
            f.write("c %d %d %d %d\n" % (k, r.kmembers[k], r.ksum[k], r.ksq[k]))
        home, hcount, hflags = r.home.tolist(), r.hcount.tolist(), r.hflags.tolist()
        for i in range(r.degree.size):
            slots = [(k, c, (hflags[i] >> j) & 1) for j, (k, c) in enumerate(zip(home[i], hcount[i])) if k >= 0]
            f.write("n %d %d %d %d %d %d %d %d%s\n" % (r.first + i, r.degree[i], r.own[i], r.embedded[i], r.reached[i], r.votes[i],
                                                      r.squares[i], len(slots), "".join(" %d %d %d" % s for s in slots)))


def read_roles(path):
    """-> (N, Roles)"""
    bad = AmmsbError("%s: not a node-roles file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 9 or head[0] != "#" or head[5] not in AMONG:
            raise bad
        try:
            N, K, M, top, min_count, skipped = (int(head[i]) for i in (1, 2, 3, 6, 7, 8))
            thr = float(np.float32(float(head[4])))
        except ValueError:
            raise bad
        if min(N, K, M, top, min_count, skipped) < 0 or skipped > M or top > MAX_TOP or not thr >= 0:
            raise bad
        per_k, per_n, home, hcount, hflags = [], [], [], [], []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                v = [int(x) for x in w[1:]]
                if min(v) < 0:
                    raise ValueError
                if w[0] == "c":
                    if len(v) != 4 or v[0] != len(per_k) or len(per_k) >= K or per_n or max(v) >= 2 ** 64:
                        raise ValueError
                    per_k.append(v[1:])
                elif w[0] == "n":
                    if len(v) < 8 or len(v) != 8 + 3 * v[7] or v[7] > top or len(per_k) != K or \
                            (per_n and v[0] != per_n[-1][0] + 1) or v[0] >= N or max(v[1:5]) >= 2 ** 32 or \
                            max(v[5:7]) >= 2 ** 64:
                        raise ValueError
                    slots = [v[8 + 3 * j:11 + 3 * j] for j in range(v[7])]
                    if any(k >= K or c >= 2 ** 32 or flag > 1 for k, c, flag in slots):
                        raise ValueError
                    per_n.append(v[:7])
                    home.append([s[0] for s in slots] + [-1] * (top - len(slots)))
                    hcount.append([s[1] for s in slots] + [0] * (top - len(slots)))
                    hflags.append(sum(s[2] << j for j, s in enumerate(slots)))
                else:
                    raise ValueError
            except (ValueError, OverflowError):
                raise AmmsbError("%s: malformed line %d" % (path, no))
    if len(per_k) != K:
        raise AmmsbError("%s: %d community lines, the header says %d" % (path, len(per_k), K))
    col = lambda rows, i: [r[i] for r in rows]   # noqa: E731
    r = Roles(thr, head[5], top, min_count, col(per_n, 1), col(per_n, 2), col(per_n, 3), col(per_n, 4), col(per_n, 5),
              col(per_n, 6), np.array(home, dtype=np.int32).reshape(len(per_n), top),
              np.array(hcount, dtype=np.uint64).reshape(len(per_n), top), hflags, col(per_k, 1), col(per_k, 2), col(per_k, 0),
              M - skipped, skipped, N=N, first=per_n[0][0] if per_n else 0)
    if int(r.degree.astype(np.uint64).sum()) > r.valid:
        raise AmmsbError("%s: the degrees sum to more than the valid targets" % path)
    return N, r
