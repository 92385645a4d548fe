"""ctypes view of libammsb_nmi.so (include/ammsb_nmi.h): the pair pass of the overlapping NMI of the detected cover
against a ground-truth cover -- and the host-side helpers that need no device: the check that a cover is made of sets,
the two scores from the entropies, and the cover-NMI text file.  A signature table of its own: _capi.SIGNATURES mirrors
include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _cover
from ._capi import AmmsbError, PostfitLibrary, _g17

MAX_COLS = 8192    # AMMSB_NMI_MAX_COLS

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_nmi_begin": (C.c_int, [_u64, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_nmi_accumulate": (C.c_int, [_vp, _u64, _u64, _u64, _vp, _u64, _vp, _u32, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_nmi_last_kernel_name": (C.c_char_p, []),
    "ammsb_nmi_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_nmi.hip can launch
KERNEL_FORMS = ("nmi_begin", "nmi_fast", "nmi_generic")

_LIBRARY = PostfitLibrary("nmi", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_sets(offsets, members):
    """NMI is defined on sets: ValueError if a community of the cover lists a node twice"""
    _cover.check_sets(offsets, members, "cover NMI", "NMI")


# ---------------------------------------------------------------------------------------------- the two scores
def conditional(H, c):
    """-> float64: H(X_g | Y) = min(c_g, H(X_g)); a community no pair qualifies for (+inf) keeps its own entropy"""
    return np.minimum(np.asarray(c, dtype=np.float64), np.asarray(H, dtype=np.float64))


def _sum(values):
    """added in index order, as mcmc::Learner::CoverNMI adds them (numpy's sum adds pairwise): the two writers print
    the same bytes"""
    total = 0.0
    for v in values.tolist():
        total += v
    return total


def scores(H_truth, h_truth, H_detected, h_detected):
    """-> (nmi_lfk, nmi_max) as include/ammsb_nmi.h states them, float64, sums in index order"""
    sides, sums = [], []
    for H, h in ((np.asarray(H_truth, np.float64), np.asarray(h_truth, np.float64)),
                 (np.asarray(H_detected, np.float64), np.asarray(h_detected, np.float64))):
        ok = H > 0
        sides.append(_sum(h[ok] / H[ok]) / float(int(ok.sum())) if ok.any() else None)
        sums.append((_sum(H), _sum(h)))
    lfk = -1.0 if None in sides else 1.0 - 0.5 * (sides[0] + sides[1])
    (HX, hX), (HY, hY) = sums
    den = max(HX, HY)
    mx = 0.5 * (HX - hX + HY - hY) / den if den > 0 else -1.0
    return lfk, mx


class NMI:
    """What Learner.CoverNMI returns.  From the device, float64: H_truth [G] = H(X_g), H_detected [K] = H(Y_k), and
    h_truth [G] = H(X_g | Y), h_detected [K] = H(Y_k | X) after the fallback min(c, H).  Integers: truth_size [G]
    uint32, detected_size [K] int64, skipped (the members >= N).  On the host: nmi_lfk and nmi_max (-1 where
    undefined)."""

    def __init__(self, threshold, truth_size, detected_size, skipped, H_truth, c_truth, H_detected, c_detected):
        self.threshold = float(threshold)
        self.truth_size = np.ascontiguousarray(truth_size, dtype=np.uint32)
        self.detected_size = np.ascontiguousarray(detected_size, dtype=np.int64)
        self.skipped = int(skipped)
        self.H_truth = np.ascontiguousarray(H_truth, dtype=np.float64)
        self.H_detected = np.ascontiguousarray(H_detected, dtype=np.float64)
        self.h_truth = conditional(self.H_truth, c_truth)
        self.h_detected = conditional(self.H_detected, c_detected)
        self.nmi_lfk, self.nmi_max = scores(self.H_truth, self.h_truth, self.H_detected, self.h_detected)

    def __repr__(self):
        return "NMI(G=%d, K=%d, skipped=%d, nmi_lfk=%.6g, nmi_max=%.6g)" % (
            self.H_truth.size, self.H_detected.size, self.skipped, self.nmi_lfk, self.nmi_max)


# ---------------------------------------------------------------------------------------------- the cover-NMI file
def write_cover_nmi(path, N, r):
    """An NMI as a text file, byte for byte what mcmc::Learner::WriteCoverNMI writes: `# N K G threshold skipped nmi_lfk
    nmi_max`, then the G lines `t g size H h` and the K lines `d k size H h`.  Floats are printed with %.17g, which
    parses back to the same bits."""
    G, K = r.H_truth.size, r.H_detected.size
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d %s %s\n" % (N, K, G, _g17(np.float32(r.threshold)), r.skipped, _g17(r.nmi_lfk),
                                              _g17(r.nmi_max)))
        for g in range(G):
            f.write("t %d %d %s %s\n" % (g, r.truth_size[g], _g17(r.H_truth[g]), _g17(r.h_truth[g])))
        for k in range(K):
            f.write("d %d %d %s %s\n" % (k, r.detected_size[k], _g17(r.H_detected[k]), _g17(r.h_detected[k])))


def read_cover_nmi(path):
    """-> (N, NMI, (nmi_lfk, nmi_max) as the file prints them)"""
    bad = AmmsbError("%s: not a cover-NMI file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 8 or head[0] != "#":
            raise bad
        try:
            N, K, G, skipped = int(head[1]), int(head[2]), int(head[3]), int(head[5])
            thr = float(np.float32(float(head[4])))
            printed = (float(head[6]), float(head[7]))
        except ValueError:
            raise bad
        if min(N, K, G, skipped) < 0:
            raise bad
        rows = {"t": [], "d": []}
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            want = "t" if len(rows["t"]) < G else "d"
            try:
                idx, size, H, h = int(w[1]), int(w[2]), float(w[3]), float(w[4])
            except (ValueError, IndexError):
                idx = -1
            if len(w) != 5 or w[0] != want or idx != len(rows[want]) or size < 0 or len(rows["d"]) >= K:
                raise AmmsbError("%s: malformed line %d" % (path, no))
            rows[want].append((size, H, h))
    if len(rows["t"]) != G or len(rows["d"]) != K:
        raise AmmsbError("%s: %d + %d lines for %d + %d communities" % (path, len(rows["t"]), len(rows["d"]), G, K))
    col = lambda side, i, dt: np.array([r[i] for r in rows[side]], dtype=dt)   # noqa: E731
    # (the file holds the conditional entropies after the fallback; min(h, H) == h gives them back)
    r = NMI(thr, col("t", 0, np.uint32), col("d", 0, np.int64), skipped, col("t", 1, np.float64),
            col("t", 2, np.float64), col("d", 1, np.float64), col("d", 2, np.float64))
    return N, r, printed
