"""ctypes view of libammsb_relate.so (include/ammsb_relate.h): how the detected communities relate to each other -- the
K x K matrix of the nodes every two of them share and per community the partners it overlaps most -- and the host-side
helpers that need no device: the derived shares (Jaccard, inside, contained), the duplicate and nested pairs, and the
related-communities text file.  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, Rpm, _g9

MAX_COLS = 8192    # AMMSB_RELATE_MAX_COLS
MAX_TOP = 64       # AMMSB_RELATE_MAX_TOP
TILE = 128         # AMMSB_RELATE_TILE
OVERLAP, JACCARD, CONTAINED = 0, 1, 2    # AMMSB_RELATE_OVERLAP, _JACCARD, _CONTAINED
MEASURES = {"overlap": OVERLAP, "jaccard": JACCARD, "contained": CONTAINED}

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_relate_bits_bytes": (_u64, [_u64, _u32]),
    "ammsb_relate_bits": (C.c_int, [C.POINTER(Rpm), _f32, _u64, _u64, _vp, _vp]),
    "ammsb_relate_pairs": (C.c_int, [_vp, _u32, _u64, _vp, _vp]),
    "ammsb_relate_top": (C.c_int, [_vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp]),
    "ammsb_relate_last_kernel_name": (C.c_char_p, []),
    "ammsb_relate_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_relate.hip can launch
KERNEL_FORMS = ("relate_bits_fast", "relate_bits_generic", "relate_pairs", "relate_top")

_LIBRARY = PostfitLibrary("relate", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "community relations")


def check_args(by, top, min_overlap):
    """-> (measure code, top, min_overlap) as the library takes them"""
    if by not in MEASURES:
        raise AmmsbError("community relations: by must be one of %s, not %r" % (", ".join(sorted(MEASURES)), by))
    top, min_overlap = int(top), int(min_overlap)
    if not 1 <= top <= MAX_TOP:
        raise AmmsbError("community relations: top must be in 1..%d, not %d" % (MAX_TOP, top))
    if not 0 <= min_overlap < 2 ** 32:
        raise AmmsbError("community relations: min_overlap must be in 0..2^32 - 1, not %d" % min_overlap)
    return MEASURES[by], top, min_overlap


def slab_rows(K, max_bytes):
    """rows of pi whose bits fit max_bytes: a multiple of 64 with K rows / 8 <= max_bytes, at least 64"""
    return max(64, int(max_bytes) * 8 // int(K) // 64 * 64)


def _share(num, den):
    out = np.zeros(num.shape, dtype=np.float64)
    np.divide(num.astype(np.float64), den.astype(np.float64), out=out, where=den > 0)
    return out


class Related:
    """What Learner.RelatedCommunities returns.  Integers, exact: size [K] int64 (CommunitySizes(threshold)), partner
    [K, top] int32 (-1 in an empty slot) and overlap [K, top] uint32 (the nodes k shares with that partner), ranked by
    `by`; matrix [K, K] uint32 with dense=True, else None.  In float64 on the host, 0 in empty slots: jaccard = o /
    (d_k + d_l - o), inside = o / d_k (how much of k lies in the partner) and contained = o / d_l (how much of the
    partner lies in k)."""

    def __init__(self, threshold, by, min_overlap, size, partner, overlap, matrix=None, N=0):
        if by not in MEASURES:
            raise AmmsbError("community relations: by must be one of %s, not %r" % (", ".join(sorted(MEASURES)), by))
        self.threshold, self.by, self.min_overlap, self.N = float(threshold), by, int(min_overlap), int(N)
        self.size = np.ascontiguousarray(size, dtype=np.int64)
        self.partner = np.ascontiguousarray(partner, dtype=np.int32)
        self.overlap = np.ascontiguousarray(overlap, dtype=np.uint32)
        K = self.size.size
        if self.size.ndim != 1 or self.partner.ndim != 2 or self.partner.shape != self.overlap.shape or \
                self.partner.shape[0] != K:
            raise AmmsbError("community relations: size [K], partner [K, top] and overlap [K, top] do not fit")
        self.top = int(self.partner.shape[1])
        self.matrix = None if matrix is None else np.ascontiguousarray(matrix, dtype=np.uint32)
        filled = self.partner >= 0
        o = np.where(filled, self.overlap, 0).astype(np.int64)
        d_k = np.broadcast_to(self.size[:, None], o.shape)
        d_l = np.where(filled, self.size[np.where(filled, self.partner, 0)], 0)
        self.jaccard = _share(o, np.where(filled, d_k + d_l - o, 0))
        self.inside = _share(o, np.where(filled, d_k, 0))
        self.contained = _share(o, d_l)

    def _pairs(self, keep):
        k, t = np.nonzero(keep & (self.partner >= 0))
        return sorted(set(zip(k.tolist(), self.partner[k, t].tolist())))

    def duplicates(self, min_jaccard=1.0):
        """-> the pairs (k, l), k < l, where one lists the other with jaccard >= min_jaccard, ascending"""
        return sorted({(min(k, l), max(k, l)) for k, l in self._pairs(self.jaccard >= float(min_jaccard))})

    def nested(self, min_share=1.0):
        """-> the pairs (k, l) where k lists l and at least min_share of l lies inside k (contained >= min_share),
        ascending; two identical communities are nested both ways"""
        return self._pairs(self.contained >= float(min_share))

    def __repr__(self):
        return "Related(K=%d, top=%d, by=%s, threshold=%s, partners=%d)" % (
            self.size.size, self.top, self.by, _g9(np.float32(self.threshold)), int((self.partner >= 0).sum()))


# ---------------------------------------------------------------------------------------------- the text file
def write_related(path, N, r):
    """A Related as a text file, byte for byte what mcmc::Learner::WriteRelatedCommunities writes: `# N K threshold by top
    min_overlap`, then per community `k size n l0 o0 l1 o1 ...` with its n partners.  Integers only below the header."""
    with open(path, "w") as f:
        f.write("# %d %d %s %s %d %d\n" % (N, r.size.size, _g9(np.float32(r.threshold)), r.by, r.top, r.min_overlap))
        for k in range(r.size.size):
            n = int((r.partner[k] >= 0).sum())
            f.write("%d %d %d" % (k, r.size[k], n))
            for t in range(n):
                f.write(" %d %d" % (r.partner[k, t], r.overlap[k, t]))
            f.write("\n")


def read_related(path):
    """-> (N, Related)"""
    bad = AmmsbError("%s: not a related-communities file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 7 or head[0] != "#" or head[4] not in MEASURES:
            raise bad
        try:
            N, K, top, min_overlap = int(head[1]), int(head[2]), int(head[5]), int(head[6])
            thr = float(np.float32(float(head[3])))
        except ValueError:
            raise bad
        if min(N, K, min_overlap) < 0 or not 1 <= top <= MAX_TOP:
            raise bad
        size = np.zeros(K, dtype=np.int64)
        partner = np.full((K, top), -1, dtype=np.int32)
        overlap = np.zeros((K, top), dtype=np.uint32)
        k = 0
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                ints = [int(v) for v in w]
            except ValueError:
                ints = []
            if len(ints) < 3 or k >= K or ints[0] != k or min(ints) < 0 or not 0 <= ints[2] <= top or \
                    len(ints) != 3 + 2 * ints[2] or any(l >= K for l in ints[3::2]):
                raise AmmsbError("%s: malformed line %d" % (path, no))
            size[k] = ints[1]
            partner[k, :ints[2]] = ints[3::2]
            overlap[k, :ints[2]] = ints[4::2]
            k += 1
    if k != K:
        raise AmmsbError("%s: %d community lines, the header says %d" % (path, k, K))
    return N, Related(thr, head[4], min_overlap, size, partner, overlap, N=N)
