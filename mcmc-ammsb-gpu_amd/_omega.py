"""ctypes view of libammsb_omega.so (include/ammsb_omega.h): the node-pair pass of the Omega index of the detected cover
against a ground-truth cover -- and the host-side helpers that need no device: the universe of nodes, the check that a
cover is made of sets, the score from the three histograms in exact integers, and the cover-Omega text file.  A
signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C
import math

import numpy as np

from . import _cover
from ._capi import AmmsbError, PostfitLibrary, Rpm, _g17

MAX_COLS = 8192                  # AMMSB_OMEGA_MAX_COLS
MAX_TRUTH = 65536                # AMMSB_OMEGA_MAX_TRUTH
MAX_LEVELS = 4096                # AMMSB_OMEGA_MAX_LEVELS
TILE = 128                       # AMMSB_OMEGA_TILE
MAX_LAUNCH_TILES = 1 << 26       # AMMSB_OMEGA_MAX_LAUNCH_TILES

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_omega_detected_bits": (C.c_int, [C.POINTER(Rpm), _f32, _vp, _u64, _vp, _vp, _vp]),
    "ammsb_omega_truth_bits": (C.c_int, [_vp, _u64, _vp, _u64, _u64, _vp, _u64, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_omega_pairs": (C.c_int, [_vp, _u32, _vp, _u64, _u64, _u32, _u64, _u64, _vp, _vp]),
    "ammsb_omega_last_kernel_name": (C.c_char_p, []),
    "ammsb_omega_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_omega.hip can launch
KERNEL_FORMS = ("omega_bits_fast", "omega_bits_generic", "omega_truth_scatter", "omega_truth_count", "omega_pairs")

_LIBRARY = PostfitLibrary("omega", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def tiles(n):
    """tiles of the upper triangle, diagonal included, of n positions"""
    R = (int(n) + TILE - 1) // TILE
    return R * (R + 1) // 2


def check_sets(offsets, members):
    """The Omega index is defined on sets: ValueError if a community of the cover lists a node twice"""
    _cover.check_sets(offsets, members, "cover omega", "the Omega index")


def check_universe(universe, N, members):
    """-> U [n] uint32, ascending and distinct: "all" = every node, "covered" = the nodes with at least one valid
    ground-truth membership (members < N), or an array of ids, which is checked: ascending, distinct, < N"""
    N = int(N)
    if isinstance(universe, str):
        if universe == "all":
            return np.arange(N, dtype=np.uint32)
        if universe == "covered":
            members = np.asarray(members, dtype=np.uint32)
            return np.unique(members[members < N]).astype(np.uint32)
        raise AmmsbError("cover omega: universe must be \"all\", \"covered\" or an array of node ids, not %r" % (universe,))
    ids = np.asarray(universe)
    if ids.ndim != 1 or (ids.size and ids.dtype.kind not in "iu"):
        raise AmmsbError("cover omega: the universe must be a 1-d integer array of node ids")
    ids = ids.astype(np.int64)
    if ids.size and (int(ids.min()) < 0 or int(ids.max()) >= N):
        raise AmmsbError("cover omega: a universe id outside 0..N - 1 (N = %d)" % N)
    if ids.size > 1 and (np.diff(ids) <= 0).any():
        raise AmmsbError("cover omega: the universe ids must ascend and be distinct")
    return np.ascontiguousarray(ids, dtype=np.uint32)


# ---------------------------------------------------------------------------------------------- the score
def _to_float(num, den):
    """the exact quotient of two integers rounded to binary64 once: Python's int / int is correctly rounded"""
    return num / den


def scores(agree, detected, truth, n):
    """-> (omega, omega_unadjusted, P) as include/ammsb_omega.h states them: Sa = sum agree, Se = sum detected truth,
    omega = (Sa P - Se) / (P^2 - Se) with numerator and denominator exact Python ints; NaN when n < 2 or P^2 == Se"""
    n = int(n)
    P = n * (n - 1) // 2
    if n < 2:
        return math.nan, math.nan, P
    Sa = sum(int(v) for v in np.asarray(agree).tolist())
    Se = sum(int(d) * int(t) for d, t in zip(np.asarray(detected).tolist(), np.asarray(truth).tolist()))
    den = P * P - Se
    omega = math.nan if den == 0 else _to_float(Sa * P - Se, den)
    return omega, _to_float(Sa, P), P


class Omega:
    """What Learner.CoverOmega returns.  Integers, exact: agree [L], detected [L], truth [L] int64 (pairs of the
    universe by the number of communities they share: in both covers alike, in the detected cover, in the ground truth),
    nodes = n, pairs = n (n - 1) / 2, skipped (the members >= N), outside (the valid members that are not in the
    universe).  On the host: omega and omega_unadjusted (NaN where undefined)."""

    def __init__(self, threshold, nodes, agree, detected, truth, skipped, outside, K=0, G=0):
        self.threshold = float(threshold)
        self.nodes = int(nodes)
        self.agree = np.ascontiguousarray(agree, dtype=np.int64)
        self.detected = np.ascontiguousarray(detected, dtype=np.int64)
        self.truth = np.ascontiguousarray(truth, dtype=np.int64)
        if not (self.agree.shape == self.detected.shape == self.truth.shape) or self.agree.ndim != 1:
            raise AmmsbError("cover omega: the three histograms must have one length")
        self.skipped, self.outside, self.K, self.G = int(skipped), int(outside), int(K), int(G)
        self.omega, self.omega_unadjusted, self.pairs = scores(self.agree, self.detected, self.truth, self.nodes)

    def __repr__(self):
        return "Omega(n=%d, L=%d, skipped=%d, outside=%d, omega=%.6g, omega_unadjusted=%.6g)" % (
            self.nodes, self.agree.size, self.skipped, self.outside, self.omega, self.omega_unadjusted)


# ---------------------------------------------------------------------------------------------- the cover-Omega file
def write_cover_omega(path, N, r):
    """An Omega as a text file, byte for byte what mcmc::Learner::WriteCoverOmega writes: `# N K G threshold universe_n
    skipped outside omega omega_unadjusted`, then the L lines `j agree detected truth`.  Floats are printed with %.17g,
    which parses back to the same bits; NaN as `nan`."""
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d %d %d %s %s\n" % (N, r.K, r.G, _g17(np.float32(r.threshold)), r.nodes, r.skipped,
                                                    r.outside, _g17(r.omega), _g17(r.omega_unadjusted)))
        for j in range(r.agree.size):
            f.write("%d %d %d %d\n" % (j, r.agree[j], r.detected[j], r.truth[j]))


def read_cover_omega(path):
    """-> (N, Omega, (omega, omega_unadjusted) as the file prints them)"""
    bad = AmmsbError("%s: not a cover-omega file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 10 or head[0] != "#":
            raise bad
        try:
            N, K, G, n, skipped, outside = (int(head[i]) for i in (1, 2, 3, 5, 6, 7))
            thr = float(np.float32(float(head[4])))
            printed = (float(head[8]), float(head[9]))
        except ValueError:
            raise bad
        if min(N, K, G, n, skipped, outside) < 0:
            raise bad
        rows = []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                ints = [int(v) for v in w]
            except ValueError:
                ints = []
            if len(ints) != 4 or ints[0] != len(rows) or min(ints) < 0:
                raise AmmsbError("%s: malformed line %d" % (path, no))
            rows.append(ints[1:])
    if not rows:
        raise AmmsbError("%s: no histogram lines" % path)
    h = np.array(rows, dtype=np.int64).reshape(-1, 3)
    return N, Omega(thr, n, h[:, 0], h[:, 1], h[:, 2], skipped, outside, K, G), printed
