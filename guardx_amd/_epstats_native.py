"""ctypes binding of libguardx_epstats.so (include/guardx_epstats.h): the learners' episode bookkeeping on the device.

load / check / GxtError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXT_OK, GXT_ERR_ARG, GXT_ERR_UNSUPPORTED, GXT_ERR_HIP = 0, 1, 2, 4
# the rows of d_moments (gxt_key)
GXT_KEY_EP_RET, GXT_KEY_EP_COST, GXT_KEY_EP_LEN, GXT_KEY_EP_COST_RET, GXT_KEY_MAX_RET, GXT_KEY_VVALS, GXT_KEY_COST_SUM = range(7)
GXT_KEYS = 7

_FP = C.c_void_p  # device pointers travel as integers
_I32 = C.c_int32
# every symbol include/guardx_epstats.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxt_last_error": (C.c_char_p, []),
    "gxt_build_id": (C.c_char_p, []),
    "gxt_work_bytes": (C.c_int64, [_I32, _I32]),
    "gxt_episode_stats": (C.c_int, [_I32, _I32, _I32, _I32] + [_FP] * 19 + [C.c_void_p]),
    "gxt_moments": (C.c_int, [_I32, _I32, _I32, _FP, _FP, C.c_void_p]),
}

_side = _sidelib.Binding("epstats", "gxt", SYMBOLS, GXT_OK, "epstats")
LIB_PATH, load, check, GxtError = _side.path, _side.load, _side.check, _side.Error
