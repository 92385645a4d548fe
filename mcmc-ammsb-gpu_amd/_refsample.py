"""ctypes view of libammsb_refsample.so (include/ammsb_refsample.h): the reference's rand_r mini-batch stream on the
device, and the host helpers it rests on (rand_r jump-ahead, the unordered_set epoch table).  A signature table of its
own: _capi.SIGNATURES mirrors include/ammsb.h and nothing else."""
import ctypes as C

from ._capi import AmmsbError, PostfitLibrary, SetDesc

STRATEGIES = {"Node": 0, "NodeLink": 1, "NodeNonLink": 2}

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64
_P = C.POINTER


class Result(C.Structure):  # ammsb_refsample_result
    _fields_ = [("n_edges", _u32), ("n_nodes", _u32), ("consumed", _u32), ("shortfall", _u32)]


# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_refsample_rand_r": (_u32, [_P(_u32)]),
    "ammsb_refsample_jump": (_u32, [_u32, _u64]),
    "ammsb_refsample_epochs": (_u32, [_u64, _P(_u64), _P(_u64), _u32]),
    "ammsb_refsample_host_order": (_u64, [_vp, _u64, _vp]),
    "ammsb_refsample_choose": (C.c_int, [C.c_int, _u64, _vp, _P(_u32), _P(_u32), _P(_u32)]),
    "ammsb_refsample_create": (C.c_int, [C.c_int, _u64, _u32, _u32, _u32, _P(_vp)]),
    "ammsb_refsample_destroy": (None, [_vp]),
    "ammsb_refsample_last_error": (C.c_char_p, [_vp]),
    "ammsb_refsample_num_epochs": (_u32, [_vp]),
    "ammsb_refsample_result_ptr": (_P(Result), [_vp]),
    "ammsb_refsample_nonlink": (C.c_int, [_vp, _u32, _u32, _u32, _P(SetDesc), _P(SetDesc), _vp, _vp, _vp]),
    "ammsb_refsample_link": (C.c_int, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
}

_LIBRARY = PostfitLibrary("refsample", SIGNATURES)   # (no check / last_kernel_name: its errors belong to a sampler handle)
LIB_PATH, load = _LIBRARY.path, _LIBRARY.load


def rand_r(state):
    """(value, new state) of one glibc rand_r call."""
    s = _u32(state)
    v = load().ammsb_refsample_rand_r(C.byref(s))
    return int(v), int(s.value)


def jump(state, calls):
    """rand_r state after `calls` further calls."""
    return int(load().ammsb_refsample_jump(int(state), int(calls)))


def epochs(max_items):
    """[(end, buckets)]: insert positions [previous end, end) of an unordered_set happen under `buckets` buckets."""
    lib = load()
    n = lib.ammsb_refsample_epochs(int(max_items), None, None, 0)
    ends, bks = (_u64 * max(n, 1))(), (_u64 * max(n, 1))()
    lib.ammsb_refsample_epochs(int(max_items), ends, bks, n)
    return [(int(ends[i]), int(bks[i])) for i in range(n)]


def host_order(keys):
    """Iteration order of a std::unordered_set that received `keys` in order, by the epoch procedure (host form)."""
    import numpy as np
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    out = np.zeros(max(keys.size, 1), dtype=np.uint64)
    n = load().ammsb_refsample_host_order(keys.ctypes.data, keys.size, out.ctypes.data)
    return out[:n].copy()
