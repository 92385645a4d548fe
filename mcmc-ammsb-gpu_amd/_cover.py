"""ctypes view of libammsb_cover.so (include/ammsb_cover.h): the best match of every ground-truth community among the
detected ones and back -- and the host-side helpers that need no device: the derived measures (F1, Jaccard and their
means), the SNAP `cmty` reader and writer, and the cover-match text file.  A signature table of its own:
_capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, Rpm, _g9

MAX_COLS = 8192    # AMMSB_COVER_MAX_COLS
UNIT = 128         # AMMSB_COVER_UNIT

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_cover_workspace_bytes": (_u64, [_u64, _u32]),
    "ammsb_cover_match": (C.c_int, [_P(Rpm), _f32, _vp, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp,
                                    _u64, _vp]),
    "ammsb_cover_last_kernel_name": (C.c_char_p, []),
    "ammsb_cover_last_error": (C.c_char_p, []),
}

# every kernel the dispatcher of csrc/ammsb_cover.hip can launch: the two counting forms and the two finishing passes
KERNEL_FORMS = ("cover_fast", "cover_generic", "cover_finish", "cover_unpack")

_LIBRARY = PostfitLibrary("cover", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "cover match")


def check_cover(truth):
    """truth: (offsets, members) host arrays, or a list of id lists (kept as written: no sorting, no de-duplication).
    -> (offsets [G + 1] uint64, members [M] uint32), contiguous"""
    if isinstance(truth, tuple) and len(truth) == 2 and not isinstance(truth[0], (list, tuple)):
        offsets, members = np.asarray(truth[0]), np.asarray(truth[1])
        if offsets.ndim != 1 or members.ndim != 1 or offsets.size < 1 or offsets.dtype.kind not in "iu" or \
                (members.size and members.dtype.kind not in "iu"):
            raise AmmsbError("cover match: offsets [G + 1] and members [M] must be 1-d integer arrays")
        if members.size and (int(members.min()) < 0 or int(members.max()) > 0xFFFFFFFF):
            raise AmmsbError("cover match: a member id outside 0..2^32 - 1")
        if int(offsets.min()) < 0:
            raise AmmsbError("cover match: a negative offset")
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        members = np.ascontiguousarray(members, dtype=np.uint32)
    else:
        lists = [np.asarray(c, dtype=np.int64).reshape(-1) for c in truth]
        sizes = np.array([c.size for c in lists], dtype=np.uint64)
        offsets = np.zeros(len(lists) + 1, dtype=np.uint64)
        np.cumsum(sizes, out=offsets[1:])
        flat = np.concatenate(lists) if lists else np.zeros(0, np.int64)
        if flat.size and (int(flat.min()) < 0 or int(flat.max()) > 0xFFFFFFFF):
            raise AmmsbError("cover match: a member id outside 0..2^32 - 1")
        members = np.ascontiguousarray(flat, dtype=np.uint32)
    if int(offsets[0]) != 0 or int(offsets[-1]) != members.size or (np.diff(offsets.astype(np.int64)) < 0).any():
        raise AmmsbError("cover match: offsets must ascend from 0 to the number of members")
    if offsets.size - 1 >= 1 << 31 or members.size >= 1 << 32:
        raise AmmsbError("cover match: 2^31 communities or 2^32 members, or more")
    return offsets, members


def check_sets(offsets, members, what, why):
    """ValueError if a community of the cover (offsets [G + 1], members [M], as check_cover returns them) lists a node
    twice: `what` opens the message, `why` is the measure that is defined on sets"""
    offsets, members = np.asarray(offsets).astype(np.int64), np.asarray(members).astype(np.int64)
    if members.size < 2:
        return
    # sort by (community, member): a duplicate is two equal neighbours of one community
    comm = np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))
    order = np.lexsort((members, comm))
    c, m = comm[order], members[order]
    twice = np.flatnonzero((c[1:] == c[:-1]) & (m[1:] == m[:-1]))
    if twice.size:
        raise ValueError("%s: ground-truth community %d lists node %d twice (%s is defined on sets)"
                         % (what, int(c[twice[0]]), int(m[twice[0]]), why))


# ---------------------------------------------------------------------------------------------- derived measures
def f1(overlap, size_a, size_b):
    """-> float64: 2 o / (a + b), 0 where o == 0"""
    o, s = np.asarray(overlap, dtype=np.float64), np.asarray(size_a, np.float64) + np.asarray(size_b, np.float64)
    out = np.zeros(o.shape)
    np.divide(2.0 * o, s, out=out, where=(o > 0) & (s > 0))
    return out


def jaccard(overlap, size_a, size_b):
    """-> float64: o / (a + b - o), 0 where o == 0"""
    o = np.asarray(overlap, dtype=np.float64)
    s = np.asarray(size_a, np.float64) + np.asarray(size_b, np.float64) - o
    out = np.zeros(o.shape)
    np.divide(o, s, out=out, where=(o > 0) & (s > 0))
    return out


def _other(best, sizes):
    """the size of each best match (0 for -1)"""
    best = np.asarray(best, dtype=np.int64)
    sizes = np.asarray(sizes, dtype=np.int64)
    out = np.zeros(best.shape, dtype=np.int64)
    ok = best >= 0
    out[ok] = sizes[best[ok]]
    return out


def _mean_over(values, present):
    """added in index order, as mcmc::Learner::CoverMatch::Derive adds them (numpy's sum adds pairwise): the two writers
    print the same bytes"""
    if not present.any():
        return -1.0
    total = 0.0
    for v in values[present].tolist():
        total += v
    return total / float(int(present.sum()))


class Match:
    """What Learner.CompareCover returns.  Integers, exact: truth_best [G] int32 (-1: unmatched), truth_overlap [G] and
    truth_size [G] uint32; detected_best [K] int32, detected_overlap [K] uint32, detected_size [K] int64; skipped (the
    members >= N); overlap [G, K] uint32 or None.  Float64, derived on the host: f1_truth_each [G], f1_detected_each
    [K] (0 for an unmatched community), jaccard_truth_each, jaccard_detected_each; f1_truth, f1_detected (the means over
    the non-empty communities) and avg_f1, each -1 where its mean is over nothing."""

    def __init__(self, threshold, truth_best, truth_overlap, truth_size, detected_best, detected_overlap, detected_size,
                 skipped, overlap=None):
        self.threshold = float(threshold)
        self.truth_best = np.ascontiguousarray(truth_best, dtype=np.int32)
        self.truth_overlap = np.ascontiguousarray(truth_overlap, dtype=np.uint32)
        self.truth_size = np.ascontiguousarray(truth_size, dtype=np.uint32)
        self.detected_best = np.ascontiguousarray(detected_best, dtype=np.int32)
        self.detected_overlap = np.ascontiguousarray(detected_overlap, dtype=np.uint32)
        self.detected_size = np.ascontiguousarray(detected_size, dtype=np.int64)
        self.skipped = int(skipped)
        self.overlap = overlap
        ts, ds = self.truth_size.astype(np.int64), self.detected_size
        self.f1_truth_each = f1(self.truth_overlap, ts, _other(self.truth_best, ds))
        self.f1_detected_each = f1(self.detected_overlap, ds, _other(self.detected_best, ts))
        self.jaccard_truth_each = jaccard(self.truth_overlap, ts, _other(self.truth_best, ds))
        self.jaccard_detected_each = jaccard(self.detected_overlap, ds, _other(self.detected_best, ts))
        self.f1_truth = _mean_over(self.f1_truth_each, ts > 0)
        self.f1_detected = _mean_over(self.f1_detected_each, ds > 0)
        self.avg_f1 = (self.f1_truth + self.f1_detected) / 2.0 if self.f1_truth >= 0 and self.f1_detected >= 0 else -1.0

    def __repr__(self):
        return "Match(G=%d, K=%d, skipped=%d, f1_truth=%.6g, f1_detected=%.6g, avg_f1=%.6g)" % (
            self.truth_best.size, self.detected_best.size, self.skipped, self.f1_truth, self.f1_detected, self.avg_f1)


def unmatched(threshold, G, detected_size, truth_size=None):
    """the Match of a call with nothing to compare (G == 0 or M == 0): every community unmatched"""
    K = np.asarray(detected_size).size
    return Match(threshold, np.full(G, -1, np.int32), np.zeros(G, np.uint32),
                 np.zeros(G, np.uint32) if truth_size is None else truth_size, np.full(K, -1, np.int32),
                 np.zeros(K, np.uint32), detected_size, 0)


# ---------------------------------------------------------------------------------------------- the SNAP cmty format
def read_cover(path, id_map=None):
    """A SNAP `cmty` file: one community per line, whitespace-separated non-negative ids; lines that start with `#` and
    blank lines are ignored.  id_map: {file id: node id}; an id it does not hold is dropped and counted.  Members are
    sorted and de-duplicated.  -> (offsets [G + 1] uint64, members [M] uint32, dropped)"""
    lists, dropped = [], 0
    with open(path) as f:
        for no, line in enumerate(f, 1):
            line = line.strip()
            if not line or line.startswith("#"):
                continue
            try:
                ids = [int(w) for w in line.split()]
            except ValueError:
                raise AmmsbError("%s: line %d is not a list of ids" % (path, no))
            if ids and min(ids) < 0:
                raise AmmsbError("%s: line %d holds a negative id" % (path, no))
            if id_map is not None:
                kept = [id_map[i] for i in ids if i in id_map]
                dropped += len(ids) - len(kept)
                ids = kept
            if ids and max(ids) > 0xFFFFFFFF:
                raise AmmsbError("%s: line %d holds an id past 2^32 - 1" % (path, no))
            lists.append(np.unique(np.array(ids, dtype=np.int64)))
    offsets, members = check_cover(lists)
    return offsets, members, dropped


def write_cover(path, offsets, members):
    """the same format: one line per community, ids separated by one blank (an empty community is an empty line, which
    read_cover skips: write no empty communities into a file whose line numbers matter)"""
    offsets, members = check_cover((offsets, members))
    with open(path, "w") as f:
        for g in range(offsets.size - 1):
            f.write(" ".join("%d" % a for a in members[int(offsets[g]):int(offsets[g + 1])]) + "\n")


# ---------------------------------------------------------------------------------------------- the cover-match file
def write_cover_match(path, N, m):
    """A Match as a text file, byte for byte what mcmc::Learner::WriteCoverMatch writes: `# N K G threshold skipped
    f1_truth f1_detected avg_f1`, then the G lines `t g size best overlap f1` and the K lines `d k size best overlap f1`.  Floats
    are printed with %.9g."""
    G, K = m.truth_best.size, m.detected_best.size
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d %s %s %s\n" % (N, K, G, _g9(np.float32(m.threshold)), m.skipped, _g9(m.f1_truth),
                                                 _g9(m.f1_detected), _g9(m.avg_f1)))
        for g in range(G):
            f.write("t %d %d %d %d %s\n" % (g, m.truth_size[g], m.truth_best[g], m.truth_overlap[g],
                                            _g9(m.f1_truth_each[g])))
        for k in range(K):
            f.write("d %d %d %d %d %s\n" % (k, m.detected_size[k], m.detected_best[k], m.detected_overlap[k],
                                            _g9(m.f1_detected_each[k])))


def read_cover_match(path):
    """-> (N, Match, (f1_truth, f1_detected, avg_f1, f1_truth_each, f1_detected_each) as the file prints them)"""
    bad = AmmsbError("%s: not a cover-match file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 9 or head[0] != "#":
            raise bad
        try:
            N, K, G, skipped = int(head[1]), int(head[2]), int(head[3]), int(head[5])
            thr = float(np.float32(head[4]))
            means = [float(v) for v in head[6:]]
        except ValueError:
            raise bad
        if min(N, K, G, skipped) < 0:
            raise bad
        rows = {"t": [], "d": []}
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                ints, fl = [int(v) for v in w[1:5]], float(w[5])
            except (ValueError, IndexError):
                ints, fl = [], 0.0
            want = "t" if len(rows["t"]) < G else "d"
            if len(w) != 6 or w[0] != want or len(ints) != 4 or ints[0] != len(rows[want]) or ints[1] < 0 or \
                    ints[2] < -1 or ints[3] < 0 or len(rows["d"]) >= K:
                raise AmmsbError("%s: malformed line %d" % (path, no))
            rows[want].append(ints[1:] + [fl])
    if len(rows["t"]) != G or len(rows["d"]) != K:
        raise AmmsbError("%s: %d + %d lines for %d + %d communities" % (path, len(rows["t"]), len(rows["d"]), G, K))
    t = np.array(rows["t"], dtype=np.float64).reshape(G, 4)
    d = np.array(rows["d"], dtype=np.float64).reshape(K, 4)
    ti = np.array([r[:3] for r in rows["t"]], dtype=np.int64).reshape(G, 3)
    di = np.array([r[:3] for r in rows["d"]], dtype=np.int64).reshape(K, 3)
    m = Match(thr, ti[:, 1], ti[:, 2], ti[:, 0], di[:, 1], di[:, 2], di[:, 0], skipped)
    return N, m, (means[0], means[1], means[2], t[:, 3].copy(), d[:, 3].copy())
