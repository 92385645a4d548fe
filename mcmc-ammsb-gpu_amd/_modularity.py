"""ctypes view of libammsb_modularity.so (include/ammsb_modularity.h): the overlapping modularity (EQ of Shen et al.) of the
detected cover against an edge list, from 128-bit fixed-point sums the device adds as integers -- and the host-side
helpers that need no device: the derived measures, and the modularity text file.  A signature table of its own:
_capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C
import math

import numpy as np

from . import _capi
from ._capi import AmmsbError, PostfitLibrary, _g9

MAX_COLS = 8192          # AMMSB_MODULARITY_MAX_COLS
W1_MAX_COLS = 4096       # AMMSB_MODULARITY_W1_MAX_COLS
FRAC_BITS = 62           # AMMSB_MODULARITY_FRAC_BITS
MAX_EDGES = 2 ** 31      # AMMSB_MODULARITY_MAX_EDGES

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_modularity_edges": (C.c_int, [_vp, _u64, _u32, _vp, _u64, _vp, _vp, _vp, _vp]),
    "ammsb_modularity_nodes": (C.c_int, [_vp, _u64, _u32, _vp, _vp, _vp]),
    "ammsb_modularity_last_kernel_name": (C.c_char_p, []),
    "ammsb_modularity_last_error": (C.c_char_p, []),
}

# every kernel the dispatchers of csrc/ammsb_modularity.hip can launch
KERNEL_FORMS = ("modularity_edges_w1", "modularity_edges_w2", "modularity_nodes_w1", "modularity_nodes_w2")

_LIBRARY = PostfitLibrary("modularity", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_threshold(threshold):
    """-> the threshold as the library takes it: a finite binary32 >= 0"""
    return _capi.check_threshold(threshold, "modularity")


def check_keys(n):
    """-> n, the number of keys of an edge list, which must stay below 2^31 (a degree is a uint32)"""
    n = int(n)
    if not 0 <= n < MAX_EDGES:
        raise AmmsbError("modularity: an edge list of %d keys; the library takes fewer than 2^31" % n)
    return n


def wide(words):
    """[2 K] uint64 (low word, high word per community) -> [K] object array of Python ints: the 128-bit values"""
    words = np.ascontiguousarray(words).view(np.uint64).reshape(-1, 2)
    out = np.empty(words.shape[0], dtype=object)
    for k, (lo, hi) in enumerate(words.tolist()):
        out[k] = (hi << 64) | lo
    return out


def derive(internal, volume, links):
    """-> (q, q_each [K], in_each [K], s_each [K]) in float64 from the 128-bit integers IN and SV and m = links, as the
    header states them: one round-to-nearest-even conversion of each integer, an exact scaling by 2^-62, then
    q_k = (2 in_k - s_k s_k / (2m)) / (2m) in this association and q = the sum in index order; -1 when m = 0"""
    K = len(internal)
    in_each = np.array([math.ldexp(float(int(v)), -FRAC_BITS) for v in internal], dtype=np.float64).reshape(K)
    s_each = np.array([math.ldexp(float(int(v)), -FRAC_BITS) for v in volume], dtype=np.float64).reshape(K)
    if links == 0:
        return -1.0, np.full(K, -1.0, dtype=np.float64), in_each, s_each
    two_m = float(2 * int(links))
    q_each = np.empty(K, dtype=np.float64)
    q = 0.0
    for k in range(K):
        i, s = float(in_each[k]), float(s_each[k])
        q_each[k] = (2.0 * i - (s * s) / two_m) / two_m
        q += float(q_each[k])
    return q, q_each, in_each, s_each


class Modularity:
    """What Learner.Modularity returns.  Integers, exact: internal and volume, [K] object arrays of Python ints (the raw
    128-bit sums IN and SV of the header, in units of 2^-62), links (the valid keys, m) and skipped (the keys with an end
    >= N); degree [N] uint32 where it was asked for, else None.  In float64 on the host: in_each, s_each, q_each [K] and
    q, -1 where m = 0."""

    def __init__(self, threshold, internal, volume, links, skipped, degree=None, N=0):
        self.threshold, self.N = float(threshold), int(N)
        self.links, self.skipped = int(links), int(skipped)
        if len(internal) != len(volume):
            raise AmmsbError("modularity: internal [K] and volume [K] do not fit")
        self.internal, self.volume = np.empty(len(internal), dtype=object), np.empty(len(volume), dtype=object)
        self.internal[:] = [int(v) for v in internal]
        self.volume[:] = [int(v) for v in volume]
        if min(self.links, self.skipped) < 0 or any(not 0 <= v < 2 ** 128 for v in self.internal) or \
                any(not 0 <= v < 2 ** 128 for v in self.volume):
            raise AmmsbError("modularity: a count is negative or a sum is outside 128 bits")
        self.degree = None if degree is None else np.ascontiguousarray(degree, dtype=np.uint32)
        self.q, self.q_each, self.in_each, self.s_each = derive(self.internal, self.volume, self.links)

    def __repr__(self):
        return "Modularity(K=%d, threshold=%s, links=%d, q=%.6g)" % (self.internal.size, _g9(np.float32(self.threshold)),
                                                                   self.links, self.q)


# ---------------------------------------------------------------------------------------------- the text file
def write_modularity(path, N, r):
    """A Modularity as a text file, byte for byte what mcmc::Learner::WriteModularity writes: `# N K E threshold skipped q`
    (E keys in the edge list, `skipped` of them with an end >= N), then per community `k q_k in_k s_k internal volume`:
    the float64 values with 17 significant digits, the 128-bit sums as 32 hexadecimal digits."""
    with open(path, "w") as f:
        f.write("# %d %d %d %s %d %.17g\n" % (N, r.internal.size, r.links + r.skipped, _g9(np.float32(r.threshold)), r.skipped,
                                             r.q))
        for k in range(r.internal.size):
            f.write("%d %.17g %.17g %.17g %032x %032x\n" % (k, r.q_each[k], r.in_each[k], r.s_each[k], r.internal[k],
                                                           r.volume[k]))


def read_modularity(path):
    """-> (N, Modularity); the float64 columns are derived again from the integers and must be those of the file"""
    bad = AmmsbError("%s: not a modularity file" % path)
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 7 or head[0] != "#":
            raise bad
        try:
            N, K, E, skipped = (int(head[i]) for i in (1, 2, 3, 5))
            thr = float(np.float32(float(head[4])))
            q = float(head[6])
        except ValueError:
            raise bad
        if min(N, K, E, skipped) < 0 or skipped > E:
            raise bad
        internal, volume, floats = [], [], []
        for no, line in enumerate(f, 2):
            w = line.split()
            if not w:
                continue
            try:
                if len(w) != 6 or len(w[4]) != 32 or len(w[5]) != 32 or int(w[0]) != len(internal) or len(internal) >= K:
                    raise ValueError
                floats.append(tuple(float(v) for v in w[1:4]))
                internal.append(int(w[4], 16))
                volume.append(int(w[5], 16))
            except ValueError:
                raise AmmsbError("%s: malformed line %d" % (path, no))
    if len(internal) != K:
        raise AmmsbError("%s: %d community lines, the header says %d" % (path, len(internal), K))
    r = Modularity(thr, internal, volume, E - skipped, skipped, N=N)
    if q != r.q or any(got != (r.q_each[k], r.in_each[k], r.s_each[k]) for k, got in enumerate(floats)):
        raise AmmsbError("%s: the float64 columns are not those of the integers" % path)
    return N, r
