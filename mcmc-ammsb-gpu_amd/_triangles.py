"""ctypes view of libammsb_triangles.so (include/ammsb_triangles.h): the triangles of a simple adjacency that lie inside the
detected communities -- per node and per community, reduced on the device to integers -- and the host-side helpers that
need no device: the simplification of an adjacency as numpy states it, the derived measures (triangle participation
ratio, clustering of a community, local clustering, the share of a node's triangles inside a shared community), and the
triangles text file.  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, _g9

MAX_COLS = 8192          # AMMSB_TRIANGLES_MAX_COLS
W1_MAX_COLS = 4096       # AMMSB_TRIANGLES_W1_MAX_COLS
MAX_ROW = 65535          # AMMSB_TRIANGLES_MAX_ROW
ROW_LDS = 1024           # AMMSB_TRIANGLES_ROW_LDS

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_triangles_nodes": (C.c_int, [_vp, _u64, _u32, _vp, _vp, _u64, _u64] + [_vp] * 7),
    "ammsb_triangles_last_kernel_name": (C.c_char_p, []),
    "ammsb_triangles_last_error": (C.c_char_p, []),
}

# every kernel the dispatcher of csrc/ammsb_triangles.hip can launch
KERNEL_FORMS = ("triangles_nodes_w1", "triangles_nodes_w2")

_LIBRARY = PostfitLibrary("triangles", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "triangles")


def check_nodes(nodes, N):
    """None or (first, count) -> (first, count) inside 0..N"""
    if nodes is None:
        return 0, int(N)
    try:
        first, count = (int(v) for v in nodes)
    except (TypeError, ValueError):
        raise AmmsbError("triangles: nodes must be (first, count), not %r" % (nodes,))
    if first < 0 or count < 0 or first + count > int(N):
        raise AmmsbError("triangles: the nodes %d .. %d are not inside 0 .. %d" % (first, first + count, int(N)))
    return first, count


def check_rows(longest):
    """-> the longest row of an adjacency, which must not be longer than 65535 (no uint32 counter wraps up to there)"""
    longest = int(longest)
    if longest > MAX_ROW:
        raise AmmsbError("triangles: a row of %d targets; the library takes rows of at most %d" % (longest, MAX_ROW))
    return longest


def _simplify(a, b, N):
    """directed entries (a, b) as int64 arrays -> (offsets [N + 1] uint64, targets uint32, skipped, dropped): both
    directions of every entry with both ends < N as 64-bit keys, sorted, made unique, loops removed.  skipped: entries with
    an end >= N; dropped: the valid entries that did not become a link of their own (repeats in either order, loops)."""
    N = int(N)
    ok = (a < N) & (b < N)
    a, b = a[ok].astype(np.uint64), b[ok].astype(np.uint64)
    keys = np.unique(np.concatenate(((a << np.uint64(32)) | b, (b << np.uint64(32)) | a)))
    src, dst = keys >> np.uint64(32), keys & np.uint64(0xFFFFFFFF)
    keep = src != dst
    src, dst = src[keep].astype(np.int64), dst[keep]
    off = np.zeros(N + 1, np.uint64)
    off[1:] = np.cumsum(np.bincount(src, minlength=N))
    return off, dst.astype(np.uint32), int((~ok).sum()), int(a.size - dst.size // 2)


def simple_csr_host(offsets, targets, N):
    """the numpy statement of the simplification, for a CSR over N rows (row a is targets[offsets[a] .. offsets[a + 1])):
    every target b of row a is the entry (a, b) -> (offsets, targets, skipped, dropped) of _simplify.  A symmetric CSR
    lists every link twice, so half of its valid entries count as dropped."""
    offsets = np.asarray(offsets).astype(np.int64)
    lengths = np.diff(offsets)
    src = np.repeat(np.arange(int(N), dtype=np.int64), lengths)
    dst = np.asarray(targets)[int(offsets[0]):int(offsets[-1])].astype(np.int64)
    return _simplify(src, dst, N)


def simple_csr_of_keys(keys, N):
    """the same for a list of keys (a << 32) | b, the ends in either order"""
    keys = np.ascontiguousarray(keys, dtype=np.uint64).reshape(-1)
    return _simplify((keys >> np.uint64(32)).astype(np.int64), (keys & np.uint64(0xFFFFFFFF)).astype(np.int64), N)


def derive(degree, tri, tri_in, ktri3, kpart, kmembers, wedges, whole=True):
    """-> (tpr [K], triangles [K] uint64, clustering [K], local_clustering [n], inside [n], total, transitivity,
    avg_clustering) from the integers, as the header states them: each integer converted once, a value -1 where its
    denominator is 0.  whole: the arrays cover every node, so every triangle was met at its three corners and 3 divides
    ktri3 and the sum of tri (asserted); over a range of nodes triangles and total are the quotients rounded down."""
    degree, tri, tri_in = (np.asarray(x, dtype=np.uint32) for x in (degree, tri, tri_in))
    ktri3, kpart, kmembers, wedges = (np.asarray(x, dtype=np.uint64) for x in (ktri3, kpart, kmembers, wedges))
    sum_tri = int(tri.astype(np.uint64).sum())
    if whole and ((ktri3 % np.uint64(3)).any() or sum_tri % 3):
        raise AmmsbError("triangles: a count over all nodes is not a multiple of 3: the adjacency is not symmetric")
    f = lambda x: x.astype(np.float64)   # noqa: E731
    tpr, clustering = np.full(ktri3.shape, -1.0), np.full(ktri3.shape, -1.0)
    np.divide(f(kpart), f(kmembers), out=tpr, where=kmembers > 0)
    np.divide(f(ktri3), f(wedges), out=clustering, where=wedges > 0)
    d = f(degree)
    pairs = d * (d - 1.0) / 2.0
    local, inside = np.full(d.shape, -1.0), np.full(d.shape, -1.0)
    np.divide(f(tri), pairs, out=local, where=degree >= 2)
    np.divide(f(tri_in), f(tri), out=inside, where=tri > 0)
    deg = degree.astype(np.uint64)
    all_pairs = int((deg * (deg - np.uint64(1)) // np.uint64(2))[degree >= 2].sum())
    transitivity = float(sum_tri) / float(all_pairs) if all_pairs else -1.0
    some = local[degree >= 2]
    avg = float(np.cumsum(some)[-1]) / float(some.size) if some.size else -1.0   # (cumsum adds in node order)
    return tpr, ktri3 // np.uint64(3), clustering, local, inside, sum_tri // 3, transitivity, avg


class Triangles:
    """What Learner.Triangles returns, for the nodes first .. first + n - 1.  Integers, exact (include/ammsb_triangles.h):
    degree, tri, tri_in, tri_comms [n] uint32; ktri3, kpart, kmembers, wedges [K] uint64 (over these nodes); M, the targets
    of the simple adjacency (twice its links); skipped, the keys with an end >= N, and dropped, the repeats and loops.  In
    float64 on the host: tpr, clustering [K], local_clustering, inside [n], transitivity, avg_clustering; triangles [K]
    uint64 and total are integers."""

    def __init__(self, threshold, degree, tri, tri_in, tri_comms, ktri3, kpart, kmembers, wedges, M, skipped, dropped, N=0,
                 first=0):
        self.threshold, self.N, self.first = float(threshold), int(N), int(first)
        self.M, self.skipped, self.dropped = int(M), int(skipped), int(dropped)
        u32 = lambda x: np.ascontiguousarray(x, dtype=np.uint32).reshape(-1)   # noqa: E731
        u64 = lambda x: np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)   # noqa: E731
        try:
            self.degree, self.tri, self.tri_in, self.tri_comms = u32(degree), u32(tri), u32(tri_in), u32(tri_comms)
            self.ktri3, self.kpart, self.kmembers, self.wedges = u64(ktri3), u64(kpart), u64(kmembers), u64(wedges)
        except (OverflowError, ValueError, TypeError):
            raise AmmsbError("triangles: an array does not fit its type")
        n, K = self.degree.size, self.ktri3.size
        if any(x.size != n for x in (self.tri, self.tri_in, self.tri_comms)) or \
                any(x.size != K for x in (self.kpart, self.kmembers, self.wedges)) or \
                min(self.M, self.skipped, self.dropped, self.first) < 0:
            raise AmmsbError("triangles: the arrays do not fit each other, or a count is negative")
        if (self.tri_in > self.tri).any() or (self.kpart > self.kmembers).any():
            raise AmmsbError("triangles: tri_in above tri, or more members in a triangle than members")
        self.whole = self.first == 0 and n == self.N
        (self.tpr, self.triangles, self.clustering, self.local_clustering, self.inside, self.total, self.transitivity,
         self.avg_clustering) = derive(self.degree, self.tri, self.tri_in, self.ktri3, self.kpart, self.kmembers, self.wedges,
                                       self.whole)

    def without_triangles(self, min_size=3):
        """-> the communities, ascending, with at least min_size members none of which is a corner of a triangle inside:
        stars, chains and pairs that a first-order score lets through"""
        return np.flatnonzero((self.kmembers >= np.uint64(max(0, int(min_size)))) & (self.kpart == 0)).astype(np.int64)

    def __repr__(self):
        return "Triangles(n=%d, K=%d, threshold=%s, total=%d)" % (self.degree.size, self.ktri3.size,
                                                                  _g9(np.float32(self.threshold)), self.total)


# ---------------------------------------------------------------------------------------------- the text file
def write_triangles(path, N, r):
    """A Triangles as a text file, byte for byte what mcmc::Learner::WriteTriangles writes: `# N K M threshold skipped dropped
    total`, per community `c k members part tri3 wedges`, per node `n a degree tri tri_in tri_comms`.  Integers
    throughout."""
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d %d %d\n" % (N, r.ktri3.size, r.M, _g9(np.float32(r.threshold)), r.skipped, r.dropped, r.total))
        for k in range(r.ktri3.size):
            f.write("c %d %d %d %d %d\n" % (k, r.kmembers[k], r.kpart[k], r.ktri3[k], r.wedges[k]))
        for i in range(r.degree.size):
            f.write("n %d %d %d %d %d\n" % (r.first + i, r.degree[i], r.tri[i], r.tri_in[i], r.tri_comms[i]))


def read_triangles(path):
    """-> (N, Triangles)"""
    bad = AmmsbError("%s: not a triangles file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 8 or head[0] != "#":
            raise bad
        try:
            N, K, M, skipped, dropped, total = (int(head[i]) for i in (1, 2, 3, 5, 6, 7))
            thr = float(np.float32(float(head[4])))
        except ValueError:
            raise bad
        if min(N, K, M, skipped, dropped, total) < 0 or not thr >= 0:
            raise bad
        per_k, per_n = [], []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                v = [int(x) for x in w[1:]]
                if min(v) < 0:
                    raise ValueError
                if w[0] == "c":
                    if len(v) != 5 or v[0] != len(per_k) or len(per_k) >= K or per_n or max(v) >= 2 ** 64:
                        raise ValueError
                    per_k.append(v[1:])
                elif w[0] == "n":
                    if len(v) != 5 or len(per_k) != K or (per_n and v[0] != per_n[-1][0] + 1) or v[0] >= N or \
                            max(v[1:]) >= 2 ** 32:
                        raise ValueError
                    per_n.append(v)
                else:
                    raise ValueError
            except (ValueError, OverflowError):
                raise AmmsbError("%s: malformed line %d" % (path, no))
    if len(per_k) != K:
        raise AmmsbError("%s: %d community lines, the header says %d" % (path, len(per_k), K))
    col = lambda rows, i: [r[i] for r in rows]   # noqa: E731
    r = Triangles(thr, col(per_n, 1), col(per_n, 2), col(per_n, 3), col(per_n, 4), col(per_k, 2), col(per_k, 1), col(per_k, 0),
                  col(per_k, 3), M, skipped, dropped, N=N, first=per_n[0][0] if per_n else 0)
    if r.total != total:
        raise AmmsbError("%s: the header's total is not a third of the nodes' triangles" % path)
    return N, r
