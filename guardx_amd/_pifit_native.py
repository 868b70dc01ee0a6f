"""ctypes binding of libguardx_pifit.so (include/guardx_pifit.h): the first-order learners' fit of the actor (Adam on the
clipped surrogate, with the early stop on kl) on the device.

load / check / GxaError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXA_OK, GXA_ERR_ARG, GXA_ERR_UNSUPPORTED, GXA_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers; so do the float64 and int64 ones, device and host
_I32 = C.c_int32
# every symbol include/guardx_pifit.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxa_last_error": (C.c_char_p, []),
    "gxa_build_id": (C.c_char_p, []),
    "gxa_param_count": (C.c_int64, [_I32, _I32, _I32]),
    "gxa_default_workgroups": (C.c_int32, [_I32]),
    "gxa_work_bytes": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "gxa_tanh_act": (C.c_int, [_I32, _FP, _FP, C.c_void_p]),
    "gxa_gradient": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, _FP, _FP, _I32, C.c_void_p, _I32, C.c_void_p, _FP,
                               C.c_void_p, C.c_void_p]),
    "gxa_fit": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, C.c_void_p, _FP, _FP, _FP, _FP, _I32, _I32, C.c_void_p,
                          C.c_void_p, _I32, _I32, C.c_void_p, C.c_void_p, _FP, C.c_void_p, C.c_void_p]),
}

_side = _sidelib.Binding("pifit", "gxa", SYMBOLS, GXA_OK, "pifit")
LIB_PATH, load, check, GxaError = _side.path, _side.load, _side.check, _side.Error
