"""ctypes binding of libguardx_linesearch.so (include/guardx_linesearch.h): the TRPO family's backtracking line search on
the device.

load / check / GxbError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXB_OK, GXB_ERR_ARG, GXB_ERR_UNSUPPORTED, GXB_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers; so do the float64 ones, device and host
_I32 = C.c_int32
# every symbol include/guardx_linesearch.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxb_last_error": (C.c_char_p, []),
    "gxb_build_id": (C.c_char_p, []),
    "gxb_param_count": (C.c_int64, [_I32, _I32, _I32]),
    "gxb_default_workgroups": (C.c_int32, [_I32, _I32]),
    "gxb_work_bytes": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "gxb_evaluate": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _I32, C.c_void_p, _I32,
                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "gxb_search": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _FP, _I32, C.c_void_p,
                             C.c_void_p, _I32, C.c_void_p, _FP, _FP, C.c_void_p, C.c_void_p, C.c_void_p]),
}

_side = _sidelib.Binding("linesearch", "gxb", SYMBOLS, GXB_OK, "linesearch")
LIB_PATH, load, check, GxbError = _side.path, _side.load, _side.check, _side.Error
