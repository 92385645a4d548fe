"""ctypes view of libammsb_linkcomm.so (include/ammsb_linkcomm.h): per link the communities that explain it -- the T
largest terms (pi[a,k] * pi[b,k]) * beta_k of its probability -- and the host-side helpers that need no device (the
link-communities text file).  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from ._capi import AmmsbError, PostfitLibrary, Rpm, _g9

MAX_TOP = 16       # AMMSB_LINKCOMM_MAX_TOP
MAX_COLS = 8192    # AMMSB_LINKCOMM_MAX_COLS
NONE = 0xFFFFFFFF  # AMMSB_LINKCOMM_NONE

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_linkcomm_edges": (C.c_int, [_P(Rpm), _vp, _f32, _vp, _u64, _u32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_linkcomm_last_kernel_name": (C.c_char_p, []),
    "ammsb_linkcomm_last_error": (C.c_char_p, []),
}

# every kernel form the dispatcher of csrc/ammsb_linkcomm.hip can select
KERNEL_FORMS = ("linkcomm_fast_v1", "linkcomm_fast_v2", "linkcomm_fast_v4", "linkcomm_fast_v4_chunked",
                "linkcomm_generic")

_LIBRARY = PostfitLibrary("linkcomm", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_args(top, min_term):
    """-> (top, min_term) as the library takes them: top in 1..16, min_term a finite binary32 >= 0"""
    top = int(top)
    if not 1 <= top <= MAX_TOP:
        raise AmmsbError("link communities: top must be in 1..%d, not %d" % (MAX_TOP, top))
    min_term = float(min_term)
    if not (0.0 <= min_term <= float(np.finfo(np.float32).max)):   # (a NaN fails both comparisons)
        raise AmmsbError("link communities: min_term must be finite and >= 0, not %r" % (min_term,))
    return top, float(np.float32(min_term))


def write_link_communities(path, N, K, top, min_term, edges, prob, ids, terms):
    """The text file `ammsb_main --link-communities-out` writes: `# N K E top min_term`, then one line per link in the
    order of `edges` (the training links in ascending key order): `a b p n k0 t0 k1 t1 ...`, n = its filled slots.
    Floats are printed with %.9g: they parse back to the same binary32."""
    edges = np.ascontiguousarray(edges).view(np.uint64).reshape(-1)
    ids = np.ascontiguousarray(ids).view(np.uint32).reshape(edges.size, int(top))
    terms = np.ascontiguousarray(terms, dtype=np.float32).reshape(edges.size, int(top))
    prob = np.ascontiguousarray(prob, dtype=np.float32).reshape(-1)
    with open(path, "w") as f:
        f.write("# %d %d %d %d %s\n" % (N, K, edges.size, top, _g9(np.float32(min_term))))
        for e, p, row, tr in zip(edges, prob, ids, terms):
            keep = row != NONE
            words = ["%d %d %s %d" % (int(e) >> 32, int(e) & NONE, _g9(p), int(keep.sum()))]
            words += ["%d %s" % (int(k), _g9(t)) for k, t in zip(row[keep], tr[keep])]
            f.write(" ".join(words) + "\n")


def read_link_communities(path):
    """-> (N, K, top, min_term, edges [E] uint64, prob [E] float32, ids [E, top] uint32 (NONE = empty),
    terms [E, top] float32)"""
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 6 or head[0] != "#":
            raise AmmsbError("%s: not a link-communities file" % path)
        N, K, E, top, min_term = int(head[1]), int(head[2]), int(head[3]), int(head[4]), np.float32(head[5])
        edges, prob, ids, terms = [], [], [], []
        for line in f:
            w = line.split()
            if not w:
                continue
            n = int(w[3]) if len(w) >= 4 else -1
            if n < 0 or len(w) != 4 + 2 * n or n > top:
                raise AmmsbError("%s: malformed line of link %s" % (path, " ".join(w[:2])))
            row = np.full(top, NONE, dtype=np.uint32)
            tr = np.zeros(top, dtype=np.float32)
            row[:n] = [int(v) for v in w[4::2]]
            tr[:n] = [np.float32(v) for v in w[5::2]]
            edges.append((int(w[0]) << 32) | int(w[1]))
            prob.append(np.float32(w[2]))
            ids.append(row)
            terms.append(tr)
    if len(edges) != E:
        raise AmmsbError("%s: %d lines for %d links" % (path, len(edges), E))
    return (N, K, top, float(min_term), np.array(edges, dtype=np.uint64), np.array(prob, dtype=np.float32),
            np.array(ids, dtype=np.uint32).reshape(E, top), np.array(terms, dtype=np.float32).reshape(E, top))
