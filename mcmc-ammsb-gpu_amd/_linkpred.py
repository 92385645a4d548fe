"""ctypes view of libammsb_linkpred.so (include/ammsb_linkpred.h): link probabilities and the T most probable links per
node from a fitted (pi, beta) on the device, and the host-side helpers that need no device (the AUC rank statistic, the
predicted-links text file).  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from ._capi import AmmsbError, PostfitLibrary, Rpm, SetDesc

MAX_TOP = 64       # AMMSB_LINKPRED_MAX_TOP
MAX_COLS = 8192    # AMMSB_LINKPRED_MAX_COLS
NONE = 0xFFFFFFFF  # AMMSB_LINKPRED_NONE
EXCLUDE_NAMES = ("training", "heldout")

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_linkpred_block": (C.c_int, [_P(Rpm), _vp, _f32, _vp, _u32, _u64, _u64, _vp, _vp]),
    "ammsb_linkpred_top": (C.c_int, [_P(Rpm), _vp, _f32, _vp, _u32, _u32, _P(SetDesc), _P(SetDesc), _u64, _u64, _vp,
                                     _vp, _vp, _u64, _vp]),
    "ammsb_linkpred_top_workspace_bytes": (_u64, [_u32, _u32, _u64, _u64]),
    "ammsb_linkpred_pairs": (C.c_int, [_P(Rpm), _vp, _f32, _vp, _u64, _vp, _vp]),
    "ammsb_linkpred_last_kernel_name": (C.c_char_p, []),
    "ammsb_linkpred_last_error": (C.c_char_p, []),
}

# every kernel form the dispatchers of csrc/ammsb_linkpred.hip can select
KERNEL_FORMS = tuple("linkpred_%s_mfma_%s_%s" % (e, q, v) for e in ("block", "top") for q in ("q128", "q32")
                     for v in ("v4", "v1")) + ("linkpred_pairs_v4", "linkpred_pairs_v1")

_LIBRARY = PostfitLibrary("linkpred", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_top(top):
    top = int(top)
    if not 1 <= top <= MAX_TOP:
        raise AmmsbError("link prediction: top must be in 1..%d, not %d" % (MAX_TOP, top))
    return top


def check_exclude(exclude):
    """-> the subset of EXCLUDE_NAMES asked for, in that order"""
    if isinstance(exclude, str):
        exclude = (exclude,)
    exclude = tuple(exclude or ())
    for name in exclude:
        if name not in EXCLUDE_NAMES:
            raise AmmsbError("link prediction: exclude takes %s, not %r" % (" / ".join(EXCLUDE_NAMES), name))
    return tuple(n for n in EXCLUDE_NAMES if n in exclude)


def auc(scores, labels):
    """Area under the ROC curve by the rank statistic: (sum of the ranks of the positives - n1 (n1 + 1) / 2) / (n1 n0),
    ranks 1-based over all scores ascending, tied scores sharing the average of their ranks; float64 throughout.  It is
    the fraction of (positive, negative) pairs the scores order correctly, a tie counting one half."""
    s = np.asarray(scores, dtype=np.float64).reshape(-1)
    y = np.asarray(labels).reshape(-1).astype(bool)
    if s.size != y.size:
        raise AmmsbError("auc: %d scores for %d labels" % (s.size, y.size))
    n1 = int(y.sum())
    n0 = int(y.size) - n1
    if n1 == 0 or n0 == 0:
        raise AmmsbError("auc: the list needs links and non-links (%d and %d)" % (n1, n0))
    order = np.argsort(s, kind="stable")
    ss = s[order]
    first = np.concatenate(([True], ss[1:] != ss[:-1]))
    start = np.flatnonzero(first)                      # first index of each run of equal scores
    length = np.diff(np.concatenate((start, [s.size])))
    avg = start + (length + 1) / 2.0                   # average 1-based rank of the run
    ranks = np.empty(s.size, dtype=np.float64)
    ranks[order] = np.repeat(avg, length)
    return float((ranks[y].sum() - n1 * (n1 + 1) / 2.0) / (float(n1) * float(n0)))


def write_links(path, N, K, top, exclude, nodes, ids, scores):
    """The text file `ammsb_main --links-out` writes: `# N K top exclude`, then `a n b0 s0 b1 s1 ...` per query node a
    (n = its non-empty slots).  Scores are printed with %.9g: they parse back to the same binary32."""
    ids = np.ascontiguousarray(ids).view(np.uint32)
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    with open(path, "w") as f:
        f.write("# %d %d %d %s\n" % (N, K, top, exclude))
        for a, row, sc in zip(np.asarray(nodes).reshape(-1), ids, scores):
            keep = row != NONE
            words = ["%d %d" % (int(a), int(keep.sum()))]
            words += ["%d %.9g" % (int(b), float(s)) for b, s in zip(row[keep], sc[keep])]
            f.write(" ".join(words) + "\n")


def read_links(path):
    """-> (N, K, top, exclude, nodes [Q] uint32, ids [Q, top] uint32 (NONE = empty), scores [Q, top] float32)"""
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 5 or head[0] != "#":
            raise AmmsbError("%s: not a links file" % path)
        N, K, top, exclude = int(head[1]), int(head[2]), int(head[3]), head[4]
        nodes, ids, scores = [], [], []
        for line in f:
            w = line.split()
            if not w:
                continue
            n = int(w[1])
            if len(w) != 2 + 2 * n or n > top:
                raise AmmsbError("%s: malformed line of node %s" % (path, w[0]))
            row = np.full(top, NONE, dtype=np.uint32)
            sc = np.zeros(top, dtype=np.float32)
            row[:n] = [int(v) for v in w[2::2]]
            sc[:n] = [np.float32(v) for v in w[3::2]]
            nodes.append(int(w[0]))
            ids.append(row)
            scores.append(sc)
    Q = len(nodes)
    return (N, K, top, exclude, np.array(nodes, dtype=np.uint32),
            np.array(ids, dtype=np.uint32).reshape(Q, top), np.array(scores, dtype=np.float32).reshape(Q, top))
