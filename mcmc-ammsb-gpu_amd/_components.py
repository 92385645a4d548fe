"""ctypes view of libammsb_components.so (include/ammsb_components.h): the connected components of every detected community
inside the graph of an edge list -- a lock-free union-find on the device over the memberships -- and the host-side helpers
that need no device: the slot numbering, the derived measures (the share of the largest component, fragmentation, the share
of connected communities), the refined and the trimmed cover, and the components text file.  A signature table of its own:
_capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, _g9

MAX_COLS = 8192          # AMMSB_COMPONENTS_MAX_COLS
W1_MAX_COLS = 4096       # AMMSB_COMPONENTS_W1_MAX_COLS
MAX_EDGES = 1 << 31      # AMMSB_COMPONENTS_MAX_EDGES
MAX_SLOTS = 1 << 32      # AMMSB_COMPONENTS_MAX_SLOTS
MAX_STEPS = 1 << 20      # AMMSB_COMPONENTS_MAX_STEPS

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_components_own": (C.c_int, [_vp, _u64, _u32, _vp, _vp]),
    "ammsb_components_slots": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _u64, _u64, _vp, _vp, _vp, _vp]),
    "ammsb_components_edges": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _u64, _vp, _vp, _vp]),
    "ammsb_components_finish": (C.c_int, [_u64, _u32, _vp, _u64] + [_vp] * 14),
    "ammsb_components_last_kernel_name": (C.c_char_p, []),
    "ammsb_components_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_components.hip can launch
KERNEL_FORMS = ("components_own_w1", "components_own_w2", "components_slots_w1", "components_slots_w2", "components_edges_w1",
                "components_edges_w2", "components_finish_roots", "components_finish_sizes", "components_finish_slots",
                "components_finish_best", "components_finish_stray")

_LIBRARY = PostfitLibrary("components", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "components")


def check_keys(n):
    """-> the number of keys of one call, which must be below 2^31"""
    n = int(n)
    if n >= MAX_EDGES:
        raise AmmsbError("components: an edge list of %d keys; the library takes fewer than 2^31" % n)
    return n


def check_slots(M, threshold=None):
    """-> M, the memberships of the cover, which must be below 2^32: a slot is a uint32"""
    M = int(M)
    if M >= MAX_SLOTS:
        at = "" if threshold is None else " at the threshold %s" % _g9(np.float32(threshold))
        raise AmmsbError("components: the cover has %d memberships%s; the library takes fewer than 2^32 "
                         "(raise the threshold)" % (M, at))
    return M


def check_giveups(n):
    """counts[3] of the library: unions that hit the fuse of 2^20 steps were left undone, so the result is no result"""
    if int(n):
        raise AmmsbError("components: %d finds or hooks took more than %d steps and were given up" % (int(n), MAX_STEPS))


def slot_base(own, threshold=None):
    """own [N] -> (base [N + 1] uint64, the exclusive prefix sum, M = base[N]); refuses M >= 2^32"""
    own = np.ascontiguousarray(own, dtype=np.uint32).reshape(-1)
    base = np.zeros(own.size + 1, np.uint64)
    np.cumsum(own, dtype=np.uint64, out=base[1:])
    return base, check_slots(base[-1], threshold)


def derive(members, components, largest):
    """-> (giant [K], fragmentation [K], connected) in float64 as the header states them: each integer converted once, -1
    where members is 0, connected -1 where every community is empty"""
    members, components = (np.asarray(x, dtype=np.uint64) for x in (members, components))
    largest = np.asarray(largest, dtype=np.uint32)
    some = members > 0
    giant = np.full(members.shape, -1.0)
    np.divide(largest.astype(np.float64), members.astype(np.float64), out=giant, where=some)
    fragmentation = np.where(some, 1.0 - giant, -1.0)
    n = int(some.sum())
    connected = float(int((components == 1).sum())) / float(n) if n else -1.0
    return giant, fragmentation, connected


class Components:
    """What Learner.CommunityComponents returns.  Integers, exact (include/ammsb_components.h): members, components,
    singletons [K] uint64, largest [K] uint32, largest_root [K] int32; the memberships as a CSR over the nodes: offsets
    [N + 1] uint64 and per slot community (uint16), root, size (uint32) [M]; stray [N] uint32; links, skipped, shared, M.  In
    float64 on the host: giant, fragmentation [K] and connected."""

    def __init__(self, threshold, members, components, largest, largest_root, singletons, offsets, community, root, size, stray,
                 links, skipped, shared):
        self.threshold = float(threshold)
        self.links, self.skipped, self.shared = int(links), int(skipped), int(shared)
        flat = lambda x, dt: np.ascontiguousarray(x, dtype=dt).reshape(-1)   # noqa: E731
        try:
            self.members, self.components, self.singletons = (flat(x, np.uint64) for x in (members, components, singletons))
            self.largest, self.largest_root = flat(largest, np.uint32), flat(largest_root, np.int32)
            self.offsets, self.community = flat(offsets, np.uint64), flat(community, np.uint16)
            self.root, self.size, self.stray = flat(root, np.uint32), flat(size, np.uint32), flat(stray, np.uint32)
        except (OverflowError, ValueError, TypeError):
            raise AmmsbError("components: an array does not fit its type")
        K = self.members.size
        self.N, self.M = self.offsets.size - 1, self.root.size
        if self.N < 0 or any(x.size != K for x in (self.components, self.singletons, self.largest, self.largest_root)) or \
                any(x.size != self.M for x in (self.community, self.size)) or self.stray.size != self.N or \
                int(self.offsets[0]) != 0 or int(self.offsets[-1]) != self.M or (np.diff(self.offsets.astype(np.int64)) < 0).any() or \
                min(self.links, self.skipped, self.shared) < 0:
            raise AmmsbError("components: the arrays do not fit each other, or a count is negative")
        if (self.M and int(self.community.max()) >= K) or (self.largest > self.members).any() or \
                (self.components > self.members).any() or (self.singletons > self.components).any():
            raise AmmsbError("components: a community id >= K, or counts that contradict each other")
        self.giant, self.fragmentation, self.connected = derive(self.members, self.components, self.largest)

    def node(self):
        """-> [M] uint32: the node of every slot"""
        return np.repeat(np.arange(self.N, dtype=np.uint32), np.diff(self.offsets.astype(np.int64)))

    def disconnected(self, min_size=2):
        """-> the communities, ascending, with more than one component of at least min_size members"""
        heads = (self.root == self.node()) & (self.size >= max(0, int(min_size)))
        return np.flatnonzero(np.bincount(self.community[heads], minlength=self.members.size) > 1).astype(np.int64)

    def _csr(self, keep):
        """-> (node, community, root) of the slots `keep`, sorted by (community, root, node)"""
        node, k = self.node()[keep], self.community[keep].astype(np.int64)
        root = self.root[keep].astype(np.int64)
        order = np.lexsort((node, root, k))
        return node[order], k[order], root[order]

    def cover(self, min_size=3):
        """-> (offsets uint64, members uint32): the refined cover as a host CSR -- every component of at least min_size
        members a community of its own, ordered by (community, root), its members ascending"""
        node, k, root = self._csr(self.size >= max(0, int(min_size)))
        new = np.ones(node.size, bool)
        new[1:] = (k[1:] != k[:-1]) | (root[1:] != root[:-1])
        return np.append(np.flatnonzero(new), node.size).astype(np.uint64), node

    def trimmed(self):
        """-> (offsets [K + 1] uint64, members uint32): per community only its largest component, members ascending"""
        node, k, _ = self._csr(self.root.astype(np.int64) == self.largest_root[self.community.astype(np.int64)])
        offsets = np.zeros(self.members.size + 1, np.uint64)
        np.cumsum(np.bincount(k, minlength=self.members.size), out=offsets[1:])
        return offsets, node

    def __repr__(self):
        return "Components(N=%d, K=%d, M=%d, threshold=%s, connected=%s)" % (
            self.N, self.members.size, self.M, _g9(np.float32(self.threshold)), _g9(self.connected))


def stray_of(offsets, community, root, largest_root):
    """-> stray [N] uint32: per node its slots whose root is not the root of its community's largest component"""
    lengths = np.diff(np.asarray(offsets).astype(np.int64))
    node = np.repeat(np.arange(lengths.size), lengths)
    out = np.asarray(root).astype(np.int64) != np.asarray(largest_root).astype(np.int64)[np.asarray(community).astype(np.int64)]
    return np.bincount(node[out], minlength=lengths.size).astype(np.uint32)


# ---------------------------------------------------------------------------------------------- the text file
def write_components(path, r):
    """A Components as a text file, byte for byte what mcmc::Learner::WriteCommunityComponents writes: `# N K E M threshold
    skipped shared` (E: all keys), per community `c k members components largest largest_root singletons`, per node `n a
    nslots k0 root0 size0 ...`.  Integers throughout."""
    with open(path, "w") as f:
        f.write("# %d %d %d %d %s %d %d\n" % (r.N, r.members.size, r.links + r.skipped, r.M, _g9(np.float32(r.threshold)),
                                              r.skipped, r.shared))
        for k in range(r.members.size):
            f.write("c %d %d %d %d %d %d\n" % (k, r.members[k], r.components[k], r.largest[k], r.largest_root[k], r.singletons[k]))
        off = r.offsets.astype(np.int64)
        trip = np.stack((r.community.astype(np.int64), r.root.astype(np.int64), r.size.astype(np.int64)), 1).reshape(-1).tolist()
        for a in range(r.N):
            lo, hi = int(off[a]), int(off[a + 1])
            f.write(" ".join(["n", str(a), str(hi - lo)] + [str(v) for v in trip[3 * lo:3 * hi]]) + "\n")


def read_components(path):
    """-> Components (stray is recomputed from the slots)"""
    bad = AmmsbError("%s: not a components file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 8 or head[0] != "#":
            raise bad
        try:
            N, K, E, M, skipped, shared = (int(head[i]) for i in (1, 2, 3, 4, 6, 7))
            thr = float(np.float32(float(head[5])))
        except ValueError:
            raise bad
        if min(N, K, E, M, skipped, shared) < 0 or skipped > E or not thr >= 0:
            raise bad
        per_k, counts, slots = [], [], []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                v = [int(x) for x in w[1:]]
                if w[0] == "c":
                    if len(v) != 6 or v[0] != len(per_k) or len(per_k) >= K or counts or min(v[:4] + v[5:]) < 0 or v[4] < -1:
                        raise ValueError
                    per_k.append(v[1:])
                elif w[0] == "n":
                    if len(per_k) != K or len(v) < 2 or v[0] != len(counts) or v[0] >= N or v[1] < 0 or \
                            len(v) != 2 + 3 * v[1] or (v[1] and min(v[2:]) < 0):
                        raise ValueError
                    counts.append(v[1])
                    slots += v[2:]
                else:
                    raise ValueError
            except (ValueError, OverflowError):
                raise AmmsbError("%s: malformed line %d" % (path, no))
    if len(per_k) != K or len(counts) != N or len(slots) != 3 * M:
        raise AmmsbError("%s: %d community lines, %d node lines and %d slots; the header says %d, %d and %d"
                         % (path, len(per_k), len(counts), len(slots) // 3, K, N, M))
    col = lambda i: [r[i] for r in per_k]   # noqa: E731
    offsets = np.zeros(N + 1, np.uint64)
    np.cumsum(np.asarray(counts, dtype=np.uint64), out=offsets[1:])
    trip = np.asarray(slots, dtype=np.int64).reshape(-1, 3)
    if trip.size and int(trip[:, 0].max()) >= K:
        raise AmmsbError("%s: a slot of a community >= K" % path)
    stray = stray_of(offsets, trip[:, 0], trip[:, 1], col(3))
    return Components(thr, col(0), col(1), col(2), col(3), col(4), offsets, trip[:, 0], trip[:, 1], trip[:, 2], stray,
                      E - skipped, skipped, shared)
