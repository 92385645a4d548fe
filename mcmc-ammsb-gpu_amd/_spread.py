"""ctypes view of libammsb_spread.so (include/ammsb_spread.h): the lazy running mean and variance of pi over the chain,
Welford's binary64 moments of beta, the credible bound mean + z sd and a row's total variance.  A signature table of its
own, like the other post-fit libraries."""
import ctypes as C

from ._average import group_lanes  # noqa: F401  (the same geometry)
from ._capi import PostfitLibrary, Rpm

MAX_COLS = 8192    # AMMSB_SPREAD_MAX_COLS
KERNEL_FORMS = ("spread_rows_v4", "spread_rows_s1", "spread_vector", "spread_bound_v4", "spread_bound_s1", "spread_rowsum")

_vp, _u32, _u64 = C.c_void_p, C.c_uint32, C.c_uint64
_P = C.POINTER

# name -> (restype, argtypes)
SIGNATURES = {
    "ammsb_spread_rows": (C.c_int, [_P(Rpm), _P(Rpm), _P(Rpm), _vp, _vp, _u64, _u64, _u32, _vp]),
    "ammsb_spread_vector": (C.c_int, [_vp, _vp, _vp, _u64, _u32, _vp]),
    "ammsb_spread_bound": (C.c_int, [_P(Rpm), _P(Rpm), _P(Rpm), C.c_float, _u64, _u64, _vp]),
    "ammsb_spread_rowsum": (C.c_int, [_P(Rpm), _vp, _u64, _u64, _vp]),
    "ammsb_spread_last_kernel_name": (C.c_char_p, []),
    "ammsb_spread_last_error": (C.c_char_p, []),
}

_LIBRARY = PostfitLibrary("spread", SIGNATURES)
LIB_PATH, load, check, last_kernel_name = _LIBRARY.path, _LIBRARY.load, _LIBRARY.check, _LIBRARY.last_kernel_name
