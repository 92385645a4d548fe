"""ctypes view of libammsb_cores.so (include/ammsb_cores.h): the k-core decomposition of the subgraph every detected
community induces in a simple adjacency -- two build passes and a level-synchronous peel on the device over the slot
numbering of the components library -- and the host-side helpers that need no device: the checks, the derived measures
(coreness, the nucleus' share, the mean core number), the shells, the c-cores and nuclei as covers, the fringe, and the
cores text file.  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, _g9

MAX_COLS = 8192          # AMMSB_CORES_MAX_COLS
W1_MAX_COLS = 4096       # AMMSB_CORES_W1_MAX_COLS
MAX_SLOTS = 1 << 32      # AMMSB_CORES_MAX_SLOTS
MAX_NBR = 1 << 32        # AMMSB_CORES_MAX_NBR
PEEL_LANES = 16          # AMMSB_CORES_PEEL_LANES
MAX_BYTES = 4 << 30      # the hosts' default budget for nbr

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_cores_degrees": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp, _vp]),
    "ammsb_cores_adjacency": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _u64, _u64, _vp, _vp, _u64, _vp, _vp]),
    "ammsb_cores_scan": (C.c_int, [_u64, _u32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_cores_peel": (C.c_int, [_u64, _u32, _u64, _u64, _vp, _vp, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_cores_finish": (C.c_int, [_u64, _u32, _vp, _u64] + [_vp] * 12),
    "ammsb_cores_last_kernel_name": (C.c_char_p, []),
    "ammsb_cores_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_cores.hip can launch
KERNEL_FORMS = ("cores_degrees_w1", "cores_degrees_w2", "cores_adjacency_w1", "cores_adjacency_w2", "cores_scan", "cores_peel",
                "cores_finish_communities", "cores_finish_nodes")

_LIBRARY = PostfitLibrary("cores", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "cores")


def check_slots(M, threshold=None):
    """-> M, the memberships of the cover, which must be below 2^32: a slot is a uint32"""
    M = int(M)
    if M >= MAX_SLOTS:
        at = "" if threshold is None else " at the threshold %s" % _g9(np.float32(threshold))
        raise AmmsbError("cores: the cover has %d memberships%s; the library takes fewer than 2^32 "
                         "(raise the threshold)" % (M, at))
    return M


def check_links(L, max_bytes=MAX_BYTES, threshold=None):
    """-> L, the entries of nbr (the sum of the inner degrees), which must be below 2^32 and fit max_bytes at 4 bytes each"""
    L, max_bytes = int(L), int(max_bytes)
    if L >= MAX_NBR or 4 * L > max_bytes:
        at = "" if threshold is None else " at the threshold %s" % _g9(np.float32(threshold))
        raise AmmsbError("cores: the induced subgraphs hold %d neighbour entries%s, %d bytes; the library takes fewer than "
                         "2^32 entries and max_bytes is %d (raise the threshold)" % (L, at, 4 * L, max_bytes))
    return L


def check_nodes(N):
    """-> N, which the Python host takes below 2^31 (the simplification sorts signed 64-bit keys)"""
    N = int(N)
    if N < 0 or N >= 2 ** 31:
        raise AmmsbError("cores: N = %d; the simplification sorts signed 64-bit keys and takes N < 2^31" % N)
    return N


def derive(community, core, members, degeneracy, nucleus):
    """-> (coreness [M], nucleus_share [K], mean_core [K]) in float64 as the header states them: each integer converted
    once; -1 where the degeneracy (coreness) or members (the other two) is 0; the sum of the core numbers in integers"""
    community = np.asarray(community).astype(np.int64)
    core, degeneracy = np.asarray(core, dtype=np.uint32), np.asarray(degeneracy, dtype=np.uint32)
    members, nucleus = np.asarray(members, dtype=np.uint64), np.asarray(nucleus, dtype=np.uint64)
    top = degeneracy[community] if community.size else np.zeros(0, np.uint32)
    coreness = np.full(core.shape, -1.0)
    np.divide(core.astype(np.float64), top.astype(np.float64), out=coreness, where=top > 0)
    some = members > 0
    share, mean = np.full(members.shape, -1.0), np.full(members.shape, -1.0)
    np.divide(nucleus.astype(np.float64), members.astype(np.float64), out=share, where=some)
    total = np.zeros(members.size, np.uint64)
    np.add.at(total, community, core.astype(np.uint64))
    np.divide(total.astype(np.float64), members.astype(np.float64), out=mean, where=some)
    return coreness, share, mean


def per_node_of(offsets, community, core, degeneracy):
    """-> (best_core uint32, best_comm int32, in_nucleus uint32) [N] as the header states them, from the slots"""
    off = np.asarray(offsets).astype(np.int64)
    N, lengths = off.size - 1, np.diff(off)
    community, core = np.asarray(community).astype(np.int64), np.asarray(core).astype(np.int64)
    node = np.repeat(np.arange(N), lengths)
    best_core, best_comm = np.zeros(N, np.int64), np.full(N, -1, np.int64)
    if core.size:
        np.maximum.at(best_core, node, core)
        first = np.full(N, np.iinfo(np.int64).max)
        hit = core == best_core[node]
        np.minimum.at(first, node[hit], community[hit])
        best_comm = np.where(lengths > 0, first, -1)
    top = np.asarray(degeneracy).astype(np.int64)[community] if core.size else np.zeros(0, np.int64)
    inner = np.bincount(node[(top > 0) & (core == top)], minlength=N) if core.size else np.zeros(N, np.int64)
    return best_core.astype(np.uint32), best_comm.astype(np.int32), inner.astype(np.uint32)


class Cores:
    """What Learner.CommunityCores returns.  Integers, exact (include/ammsb_cores.h): members, inlinks2, nucleus, isolated
    [K] uint64, degeneracy [K] uint32; the memberships as a CSR over the nodes: offsets [N + 1] uint64 and per slot community
    (uint16), indeg, core (uint32) [M]; best_core, in_nucleus (uint32), best_comm (int32) [N]; M, L, skipped, dropped, and
    the launch counts scans and rounds (diagnostic).  In float64 on the host: coreness [M], nucleus_share, mean_core [K]."""

    def __init__(self, threshold, members, inlinks2, degeneracy, nucleus, isolated, offsets, community, indeg, core, best_core,
                 best_comm, in_nucleus, skipped=0, dropped=0, scans=0, rounds=0):
        self.threshold = float(threshold)
        self.skipped, self.dropped, self.scans, self.rounds = int(skipped), int(dropped), int(scans), int(rounds)
        flat = lambda x, dt: np.ascontiguousarray(x, dtype=dt).reshape(-1)   # noqa: E731
        try:
            self.members, self.inlinks2, self.nucleus, self.isolated = (flat(x, np.uint64) for x in (members, inlinks2, nucleus, isolated))
            self.degeneracy = flat(degeneracy, np.uint32)
            self.offsets, self.community = flat(offsets, np.uint64), flat(community, np.uint16)
            self.indeg, self.core = flat(indeg, np.uint32), flat(core, np.uint32)
            self.best_core, self.in_nucleus = flat(best_core, np.uint32), flat(in_nucleus, np.uint32)
            self.best_comm = flat(best_comm, np.int32)
        except (OverflowError, ValueError, TypeError):
            raise AmmsbError("cores: an array does not fit its type")
        K = self.members.size
        self.N, self.M = self.offsets.size - 1, self.core.size
        if self.N < 0 or any(x.size != K for x in (self.inlinks2, self.nucleus, self.isolated, self.degeneracy)) or \
                any(x.size != self.M for x in (self.community, self.indeg)) or \
                any(x.size != self.N for x in (self.best_core, self.best_comm, self.in_nucleus)) or \
                int(self.offsets[0]) != 0 or int(self.offsets[-1]) != self.M or (np.diff(self.offsets.astype(np.int64)) < 0).any() or \
                min(self.skipped, self.dropped, self.scans, self.rounds) < 0:
            raise AmmsbError("cores: the arrays do not fit each other, or a count is negative")
        if (self.M and int(self.community.max()) >= K) or (self.core > self.indeg).any() or \
                ((self.core == 0) != (self.indeg == 0)).any() or (self.nucleus > self.members).any() or \
                (self.isolated > self.members).any() or int(self.members.sum()) != self.M:
            raise AmmsbError("cores: a community id >= K, or counts that contradict each other")
        self.L = int(self.indeg.sum(dtype=np.uint64))
        self.coreness, self.nucleus_share, self.mean_core = derive(self.community, self.core, self.members, self.degeneracy,
                                                                   self.nucleus)

    def node(self):
        """-> [M] uint32: the node of every slot"""
        return np.repeat(np.arange(self.N, dtype=np.uint32), np.diff(self.offsets.astype(np.int64)))

    def shells(self, k):
        """-> the histogram of the core numbers of community k: [degeneracy[k] + 1] int64 ([0] for an empty community)"""
        k = int(k)
        if not 0 <= k < self.members.size:
            raise AmmsbError("cores: no community %d" % k)
        return np.bincount(self.core[self.community == k].astype(np.int64), minlength=int(self.degeneracy[k]) + 1).astype(np.int64)

    def _csr(self, keep, empty):
        """the slots `keep` as a host CSR ordered by community (members ascending); empty: keep the empty ones
        -> (offsets uint64, members uint32, the communities of the rows)"""
        node, k = self.node()[keep], self.community[keep].astype(np.int64)
        order = np.lexsort((node, k))
        per = np.bincount(k, minlength=self.members.size)
        rows = np.arange(self.members.size) if empty else np.flatnonzero(per)
        offsets = np.zeros(rows.size + 1, np.uint64)
        np.cumsum(per[rows], out=offsets[1:])
        return offsets, node[order], rows.astype(np.int64)

    def cover(self, c):
        """-> (offsets uint64, members uint32, community int64): the c-cores of all communities as a host CSR ordered by
        k, the empty ones left out"""
        return self._csr(self.core >= max(0, int(c)), False)

    def nuclei(self):
        """-> (offsets, members, community): per community of degeneracy >= 1 its innermost core"""
        top = self.degeneracy[self.community.astype(np.int64)] if self.M else np.zeros(0, np.uint32)
        return self._csr((top >= 1) & (self.core == top), False)

    def fringe(self, c=1):
        """-> the slots, ascending, with core <= c"""
        return np.flatnonzero(self.core <= max(0, int(c))).astype(np.int64)

    def __repr__(self):
        return "Cores(N=%d, K=%d, M=%d, L=%d, threshold=%s, degeneracy<=%d)" % (
            self.N, self.members.size, self.M, self.L, _g9(np.float32(self.threshold)),
            int(self.degeneracy.max()) if self.degeneracy.size else 0)


# ---------------------------------------------------------------------------------------------- the text file
def write_cores(path, r):
    """A Cores as a text file, byte for byte what mcmc::Learner::WriteCommunityCores writes: `# N K M L threshold skipped
    dropped`, per community `c k members inlinks2 degeneracy nucleus isolated`, per node `n a nslots k0 indeg0 core0 ...`.
    Integers throughout."""
    with open(path, "w") as f:
        f.write("# %d %d %d %d %s %d %d\n" % (r.N, r.members.size, r.M, r.L, _g9(np.float32(r.threshold)), r.skipped, r.dropped))
        for k in range(r.members.size):
            f.write("c %d %d %d %d %d %d\n" % (k, r.members[k], r.inlinks2[k], r.degeneracy[k], r.nucleus[k], r.isolated[k]))
        off = r.offsets.astype(np.int64)
        trip = np.stack((r.community.astype(np.int64), r.indeg.astype(np.int64), r.core.astype(np.int64)), 1).reshape(-1).tolist()
        for a in range(r.N):
            lo, hi = int(off[a]), int(off[a + 1])
            f.write(" ".join(["n", str(a), str(hi - lo)] + [str(v) for v in trip[3 * lo:3 * hi]]) + "\n")


def read_cores(path):
    """-> Cores (the per-node arrays are recomputed from the slots; scans and rounds are not in the file)"""
    bad = AmmsbError("%s: not a cores file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 8 or head[0] != "#":
            raise bad
        try:
            N, K, M, L, skipped, dropped = (int(head[i]) for i in (1, 2, 3, 4, 6, 7))
            thr = float(np.float32(float(head[5])))
        except ValueError:
            raise bad
        if min(N, K, M, L, skipped, dropped) < 0 or not thr >= 0:
            raise bad
        per_k, counts, slots = [], [], []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                v = [int(x) for x in w[1:]]
                if w[0] == "c":
                    if len(v) != 6 or v[0] != len(per_k) or len(per_k) >= K or counts or min(v) < 0:
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
    if int(trip[:, 1].sum()) != L:
        raise AmmsbError("%s: the inner degrees add up to %d; the header says %d" % (path, int(trip[:, 1].sum()), L))
    best_core, best_comm, inner = per_node_of(offsets, trip[:, 0], trip[:, 2], col(2))
    return Cores(thr, col(0), col(1), col(2), col(3), col(4), offsets, trip[:, 0], trip[:, 1], trip[:, 2], best_core, best_comm,
                 inner, skipped, dropped)
