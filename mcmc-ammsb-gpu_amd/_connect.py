"""ctypes view of libammsb_connect.so (include/ammsb_connect.h): how the detected communities are linked to each other --
the K x K matrix of the links of an edge list between every two of them and per community the partners it is linked to
most -- and the host-side helpers that need no device: the derived densities, the bridged pairs, and the
linked-communities text file.  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, Rpm, _g9

MAX_COLS = 8192        # AMMSB_CONNECT_MAX_COLS
MAX_TOP = 64           # AMMSB_CONNECT_MAX_TOP
RUNS_MAX_COLS = 4096   # AMMSB_CONNECT_RUNS_MAX_COLS
LINKS, DENSITY = 0, 1  # AMMSB_CONNECT_LINKS, _DENSITY
MEASURES = {"links": LINKS, "density": DENSITY}

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_connect_mask_bytes": (_u64, [_u64, _u32]),
    "ammsb_connect_mask": (C.c_int, [C.POINTER(Rpm), _f32, _vp, _vp]),
    "ammsb_connect_edges": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _vp]),
    "ammsb_connect_finish": (C.c_int, [_vp, _u32, _vp, _vp]),
    "ammsb_connect_top": (C.c_int, [_vp, _vp, _u32, _u32, _u32, _u64, _vp, _vp, _vp, _vp]),
    "ammsb_connect_last_kernel_name": (C.c_char_p, []),
    "ammsb_connect_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_connect.hip can launch
KERNEL_FORMS = ("connect_mask_fast", "connect_mask_generic", "connect_edges_direct", "connect_edges_runs", "connect_finish",
                "connect_top")

_LIBRARY = PostfitLibrary("connect", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "community links")


def check_args(by, top, min_links):
    """-> (measure code, top, min_links) as the library takes them"""
    if by not in MEASURES:
        raise AmmsbError("community links: by must be one of %s, not %r" % (", ".join(sorted(MEASURES)), by))
    top, min_links = int(top), int(min_links)
    if not 1 <= top <= MAX_TOP:
        raise AmmsbError("community links: top must be in 1..%d, not %d" % (MAX_TOP, top))
    if not 0 <= min_links < 2 ** 64:
        raise AmmsbError("community links: min_links must be in 0..2^64 - 1, not %d" % min_links)
    return MEASURES[by], top, min_links


def _ratio(num, den):
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den > 0)
    return out


class Linked:
    """What Learner.LinkedCommunities returns.  Integers, exact: size [K] int64 (CommunitySizes(threshold)), internal [K]
    int64 (the links inside k: half the diagonal of the link matrix), partner [K, top] int32 (-1 in an empty slot), links
    [K, top] uint64 (the links between k and that partner) and shared [K, top] uint32 (the nodes they share), ranked by
    `by`; valid and skipped, the keys of the edge list that were counted and those with an end >= N; matrix [K, K] uint64
    with dense=True, else None.  In float64 on the host: density [K, top] = links / (d_k d_l - shared), 0 in empty slots
    (and where there is no pair of distinct nodes), and within [K] = 2 internal / (d_k (d_k - 1)), -1 where d_k < 2."""

    def __init__(self, threshold, by, min_links, size, internal, partner, links, shared, valid, skipped, matrix=None, N=0):
        if by not in MEASURES:
            raise AmmsbError("community links: by must be one of %s, not %r" % (", ".join(sorted(MEASURES)), by))
        self.threshold, self.by, self.min_links, self.N = float(threshold), by, int(min_links), int(N)
        self.valid, self.skipped = int(valid), int(skipped)
        self.size = np.ascontiguousarray(size, dtype=np.int64)
        self.internal = np.ascontiguousarray(internal, dtype=np.int64)
        self.partner = np.ascontiguousarray(partner, dtype=np.int32)
        self.links = np.ascontiguousarray(links, dtype=np.uint64)
        self.shared = np.ascontiguousarray(shared, dtype=np.uint32)
        K = self.size.size
        if self.size.ndim != 1 or self.internal.shape != self.size.shape or self.partner.ndim != 2 or \
                self.partner.shape != self.links.shape or self.partner.shape != self.shared.shape or \
                self.partner.shape[0] != K:
            raise AmmsbError("community links: size [K], internal [K], partner, links and shared [K, top] do not fit")
        self.top = int(self.partner.shape[1])
        self.matrix = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.uint64)
        filled = self.partner >= 0
        d = self.size.astype(np.uint64)
        d_k = np.broadcast_to(d[:, None], self.partner.shape)
        d_l = d[np.where(filled, self.partner, 0)]
        pairs = np.where(filled, d_k * d_l - self.shared.astype(np.uint64), np.uint64(0))
        self.density = _ratio(np.where(filled, self.links, np.uint64(0)), pairs)
        self.within = np.full(K, -1.0, dtype=np.float64)
        big = self.size >= 2
        np.divide(2.0 * self.internal.astype(np.float64), (d * (d - np.uint64(1))).astype(np.float64), out=self.within, where=big)

    def bridged(self, min_ratio=1.0):
        """-> the pairs (k, l), k < l, where one lists the other and the density between them is at least min_ratio times
        the smaller of the two densities within, both of which are > 0; ascending.  Two such columns are linked to each
        other as densely as one of them is inside: one community split in two."""
        out = set()
        for k, t in zip(*np.nonzero(self.partner >= 0)):
            l = int(self.partner[k, t])
            wk, wl = self.within[k], self.within[l]
            if wk > 0 and wl > 0 and self.density[k, t] >= float(min_ratio) * min(wk, wl):
                out.add((min(int(k), l), max(int(k), l)))
        return sorted(out)

    def __repr__(self):
        return "Linked(K=%d, top=%d, by=%s, threshold=%s, partners=%d, links=%d)" % (
            self.size.size, self.top, self.by, _g9(np.float32(self.threshold)), int((self.partner >= 0).sum()), self.valid)


# ---------------------------------------------------------------------------------------------- the text file
def write_linked(path, N, r):
    """A Linked as a text file, byte for byte what mcmc::Learner::WriteLinkedCommunities writes: `# N K E threshold by top
    min_links skipped` (E keys in the edge list, `skipped` of them with an end >= N), then per community `k size internal n
    l0 w0 o0 l1 w1 o1 ...` with its n partners, the links to each and the nodes shared with each.  Integers only below the
    header."""
    with open(path, "w") as f:
        f.write("# %d %d %d %s %s %d %d %d\n" % (N, r.size.size, r.valid + r.skipped, _g9(np.float32(r.threshold)), r.by, r.top,
                                                r.min_links, r.skipped))
        for k in range(r.size.size):
            n = int((r.partner[k] >= 0).sum())
            f.write("%d %d %d %d" % (k, r.size[k], r.internal[k], n))
            for t in range(n):
                f.write(" %d %d %d" % (r.partner[k, t], r.links[k, t], r.shared[k, t]))
            f.write("\n")


def read_linked(path):
    """-> (N, Linked)"""
    bad = AmmsbError("%s: not a linked-communities file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 9 or head[0] != "#" or head[5] not in MEASURES:
            raise bad
        try:
            N, K, E, top, min_links, skipped = (int(head[i]) for i in (1, 2, 3, 6, 7, 8))
            thr = float(np.float32(float(head[4])))
        except ValueError:
            raise bad
        if min(N, K, E, min_links, skipped) < 0 or skipped > E or not 1 <= top <= MAX_TOP:
            raise bad
        size, internal = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        partner = np.full((K, top), -1, dtype=np.int32)
        links = np.zeros((K, top), dtype=np.uint64)
        shared = np.zeros((K, top), dtype=np.uint32)
        k = 0
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                ints = [int(v) for v in w]
            except ValueError:
                ints = []
            if len(ints) < 4 or k >= K or ints[0] != k or min(ints) < 0 or not 0 <= ints[3] <= top or \
                    len(ints) != 4 + 3 * ints[3] or any(l >= K for l in ints[4::3]):
                raise AmmsbError("%s: malformed line %d" % (path, no))
            size[k], internal[k] = ints[1], ints[2]
            partner[k, :ints[3]] = ints[4::3]
            links[k, :ints[3]] = ints[5::3]
            shared[k, :ints[3]] = ints[6::3]
            k += 1
    if k != K:
        raise AmmsbError("%s: %d community lines, the header says %d" % (path, k, K))
    return N, Linked(thr, head[5], min_links, size, internal, partner, links, shared, E - skipped, skipped, N=N)
