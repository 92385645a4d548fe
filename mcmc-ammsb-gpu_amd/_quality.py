"""ctypes view of libammsb_quality.so (include/ammsb_quality.h): per community the links inside it and the links that
leave it, from one membership bit per (node, community) -- and the host-side helpers that need no device: the derived
measures (conductance, density, coverage) and the community-quality text file.  A signature table of its own:
_capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, Rpm, _g9

MAX_COLS = 8192    # AMMSB_QUALITY_MAX_COLS

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_quality_mask_bytes": (_u64, [_u64, _u32]),
    "ammsb_quality_mask": (C.c_int, [_P(Rpm), _f32, _vp, _vp]),
    "ammsb_quality_edges": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _vp]),
    "ammsb_quality_last_kernel_name": (C.c_char_p, []),
    "ammsb_quality_last_error": (C.c_char_p, []),
}

# every kernel form the dispatchers of csrc/ammsb_quality.hip can select
KERNEL_FORMS = ("quality_mask_fast", "quality_mask_generic", "quality_edges_w1", "quality_edges_w2")

_LIBRARY = PostfitLibrary("quality", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "community quality")


def conductance(internal, boundary, links):
    """-> [K] float64: boundary / min(vol, 2 links - vol) with vol = 2 internal + boundary; -1 where the minimum is 0"""
    internal, boundary = np.asarray(internal, dtype=np.int64), np.asarray(boundary, dtype=np.int64)
    vol = 2 * internal + boundary
    low = np.minimum(vol, 2 * int(links) - vol)
    out = np.full(internal.shape, -1.0)
    np.divide(boundary.astype(np.float64), low.astype(np.float64), out=out, where=low > 0)
    return out


def density(size, internal):
    """-> [K] float64: internal / (size (size - 1) / 2); -1 where size < 2"""
    size, internal = np.asarray(size, dtype=np.int64), np.asarray(internal, dtype=np.int64)
    pairs = size.astype(np.float64) * (size.astype(np.float64) - 1.0) / 2.0
    out = np.full(size.shape, -1.0)
    np.divide(internal.astype(np.float64), pairs, out=out, where=size >= 2)
    return out


def coverage(uncovered, links):
    """-> 1 - uncovered / links; -1 with no links"""
    return 1.0 - float(uncovered) / float(links) if int(links) > 0 else -1.0


class Quality:
    """What Learner.CommunityQuality returns: size, internal, boundary [K] int64 host arrays; links (the valid edges),
    uncovered and skipped as ints; conductance and density [K] float64; coverage, and the threshold they were made at."""

    def __init__(self, threshold, size, internal, boundary, links, uncovered, skipped):
        self.threshold = float(threshold)
        self.size = np.ascontiguousarray(size, dtype=np.int64)
        self.internal = np.ascontiguousarray(internal, dtype=np.int64)
        self.boundary = np.ascontiguousarray(boundary, dtype=np.int64)
        self.links, self.uncovered, self.skipped = int(links), int(uncovered), int(skipped)
        self.conductance = conductance(self.internal, self.boundary, self.links)
        self.density = density(self.size, self.internal)
        self.coverage = coverage(self.uncovered, self.links)

    def __repr__(self):
        return "Quality(K=%d, links=%d, uncovered=%d, skipped=%d, coverage=%.6g)" % (
            self.size.size, self.links, self.uncovered, self.skipped, self.coverage)


def write_community_quality(path, N, threshold, size, internal, boundary, links, uncovered):
    """The text file `ammsb_main --community-quality-out` writes: `# N K E threshold uncovered` (E = the links), then one
    line `k size internal boundary conductance density` per community.  Floats are printed with %.9g."""
    size, internal, boundary = (np.asarray(x, dtype=np.int64).reshape(-1) for x in (size, internal, boundary))
    cond, dens = conductance(internal, boundary, links), density(size, internal)
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d\n" % (N, size.size, links, _g9(np.float32(threshold)), uncovered))
        for k in range(size.size):
            f.write("%d %d %d %d %s %s\n" % (k, size[k], internal[k], boundary[k], _g9(cond[k]), _g9(dens[k])))


def read_community_quality(path):
    """-> (N, K, E, threshold, uncovered, size [K] int64, internal [K] int64, boundary [K] int64,
    conductance [K] float64, density [K] float64), the floats as the file prints them"""
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 6 or head[0] != "#":
            raise AmmsbError("%s: not a community-quality file" % path)
        try:
            N, K, E, thr, unc = int(head[1]), int(head[2]), int(head[3]), float(np.float32(head[4])), int(head[5])
        except ValueError:
            raise AmmsbError("%s: not a community-quality file" % path)
        ints, floats = [], []
        for line in f:
            w = line.split()
            if not w:
                continue
            try:
                row = [int(v) for v in w[:4]]
                fl = [float(v) for v in w[4:]]
            except ValueError:
                row, fl = [], []
            if len(w) != 6 or len(row) != 4 or row[0] != len(ints) or min(row) < 0:
                raise AmmsbError("%s: malformed line %d" % (path, len(ints) + 2))
            ints.append(row[1:])
            floats.append(fl)
    if len(ints) != K:
        raise AmmsbError("%s: %d lines for %d communities" % (path, len(ints), K))
    ints = np.array(ints, dtype=np.int64).reshape(K, 3)
    floats = np.array(floats, dtype=np.float64).reshape(K, 2)
    return (N, K, E, thr, unc, ints[:, 0].copy(), ints[:, 1].copy(), ints[:, 2].copy(), floats[:, 0].copy(),
            floats[:, 1].copy())
