"""ctypes view of libammsb_average.so (include/ammsb_average.h): the lazy running mean of pi over the chain and the binary64
mean of beta.  A signature table of its own, like the other post-fit libraries."""
import ctypes as C

from ._capi import PostfitLibrary, Rpm

MAX_COLS = 8192    # AMMSB_AVERAGE_MAX_COLS
KERNEL_FORMS = ("average_rows_v4", "average_rows_s1", "average_vector", "average_round")

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_average_rows": (C.c_int, [_P(Rpm), _P(Rpm), _vp, _vp, _u64, _u64, _u32, _vp]),
    "ammsb_average_vector": (C.c_int, [_vp, _vp, _u64, _u32, _vp]),
    "ammsb_average_round": (C.c_int, [_vp, _vp, _u64, _vp]),
    "ammsb_average_last_kernel_name": (C.c_char_p, []),
    "ammsb_average_last_error": (C.c_char_p, []),
}

_LIBRARY = PostfitLibrary("average", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name


def group_lanes(K):
    """lanes that own a row: the smallest power of two >= ceil(K / 4), at most 64"""
    g = 1
    while g < (int(K) + 3) // 4 and g < 64:
        g *= 2
    return g
