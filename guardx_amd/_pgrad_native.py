"""ctypes binding of libguardx_pgrad.so (include/guardx_pgrad.h): the surrogate gradients g and b of the TRPO family's
update() and CPO's step direction on the device.

load / check / GxgError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXG_OK, GXG_ERR_ARG, GXG_ERR_UNSUPPORTED, GXG_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers; so do the float64 ones
_I32 = C.c_int32
# every symbol include/guardx_pgrad.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxg_last_error": (C.c_char_p, []),
    "gxg_build_id": (C.c_char_p, []),
    "gxg_param_count": (C.c_int64, [_I32, _I32, _I32]),
    "gxg_default_workgroups": (C.c_int32, [_I32]),
    "gxg_work_bytes": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "gxg_gradient": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, _FP, _FP, _FP, _I32, C.c_void_p, _FP, _FP, C.c_void_p,
                               C.c_void_p]),
    "gxg_cpo_direction": (C.c_int, [_I32, _FP, _FP, _FP, _FP, _FP, C.c_void_p, _FP, _FP, C.c_void_p, C.c_void_p]),
    "gxg_trpo_direction": (C.c_int, [_I32, _FP, _FP, C.c_void_p, _FP, C.c_void_p]),
}

_side = _sidelib.Binding("pgrad", "gxg", SYMBOLS, GXG_OK, "pgrad")
LIB_PATH, load, check, GxgError = _side.path, _side.load, _side.check, _side.Error
