"""ctypes view of libammsb_readout.so (include/ammsb_readout.h): memberships and community sizes read out of pi on the
device, and the host-side helpers that need no device (the community CSR built from an ids table, the communities text
file).  A signature table of its own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

import numpy as np

from ._capi import AmmsbError, PostfitLibrary, Rpm

MAX_TOP = 16       # AMMSB_READOUT_MAX_TOP
MAX_COLS = 8192    # AMMSB_READOUT_MAX_COLS
NONE = 0xFFFFFFFF  # AMMSB_READOUT_NONE

_vp, _u32, _u64, _f32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_float
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_readout_top": (C.c_int, [_P(Rpm), _vp, _u64, _u64, _u32, _f32, _vp, _vp, _vp, _vp, _vp]),
    "ammsb_readout_last_kernel_name": (C.c_char_p, []),
    "ammsb_readout_last_error": (C.c_char_p, []),
}

_LIBRARY = PostfitLibrary("readout", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def check_args(top, threshold):
    """The argument rules every layer shares (the library enforces them again)."""
    top, threshold = int(top), float(threshold)
    if not 1 <= top <= MAX_TOP:
        raise AmmsbError("read-out: top must be in 1..%d, not %d" % (MAX_TOP, top))
    if not threshold >= 0.0:
        raise AmmsbError("read-out: the threshold must be >= 0, not %r" % threshold)
    return top, threshold


def communities_csr(ids, K, nodes=None):
    """(offsets [K+1] int64, members int32) from an ids table [n, T] (uint32, NONE = empty slot): community k's members
    are members[offsets[k]:offsets[k+1]], ascending.  Row i stands for node nodes[i] (default: i)."""
    ids = np.ascontiguousarray(ids).view(np.uint32)
    if ids.ndim != 2:
        raise AmmsbError("communities_csr: ids must be [n, T]")
    n, T = ids.shape
    who = np.arange(n, dtype=np.int64) if nodes is None else np.asarray(nodes, dtype=np.int64)
    flat = ids.reshape(-1)
    keep = flat != NONE
    comm = flat[keep].astype(np.int64)
    if comm.size and comm.max() >= K:
        raise AmmsbError("communities_csr: an id >= K")
    node = np.repeat(who, T)[keep]
    order = np.lexsort((node, comm))
    offsets = np.zeros(K + 1, dtype=np.int64)
    np.cumsum(np.bincount(comm, minlength=K), out=offsets[1:])
    return offsets, node[order].astype(np.int32)


def write_communities(path, N, K, top, threshold, sizes, offsets, members):
    """The text file `ammsb_main --communities-out` writes: `# N K top threshold`, then `k size n0 n1 ...` per
    community (size = the uncapped sizes[k], members ascending)."""
    with open(path, "w") as f:
        f.write("# %d %d %d %.9g\n" % (N, K, top, threshold))
        for k in range(K):
            m = members[offsets[k]:offsets[k + 1]]
            f.write(" ".join(["%d %d" % (k, int(sizes[k]))] + ["%d" % v for v in m]) + "\n")


def read_communities(path):
    """-> (N, K, top, threshold, sizes [K] int64, offsets [K+1] int64, members int32)"""
    with open(path) as f:
        head = f.readline().split()
        if len(head) != 5 or head[0] != "#":
            raise AmmsbError("%s: not a communities file" % path)
        N, K, top, thr = int(head[1]), int(head[2]), int(head[3]), float(head[4])
        sizes, offsets, members = np.zeros(K, dtype=np.int64), np.zeros(K + 1, dtype=np.int64), []
        for k in range(K):
            w = f.readline().split()
            if len(w) < 2 or int(w[0]) != k:
                raise AmmsbError("%s: line of community %d missing" % (path, k))
            sizes[k] = int(w[1])
            members.append(np.array(w[2:], dtype=np.int32))
            offsets[k + 1] = offsets[k] + len(w) - 2
    return N, K, top, thr, sizes, offsets, (np.concatenate(members) if members else np.zeros(0, np.int32))
