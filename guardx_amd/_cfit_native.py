"""ctypes binding of libguardx_cfit.so (include/guardx_cfit.h): the fit of the safety critics (usl / lpg's c_net, scpo's
v_net, safelayer's g_net) by Adam on a row-weighted squared loss, on the device.

load / check / GxqError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXQ_OK, GXQ_ERR_ARG, GXQ_ERR_UNSUPPORTED, GXQ_ERR_HIP = 0, 1, 2, 4
GXQ_HEAD_IDENTITY, GXQ_HEAD_SOFTPLUS, GXQ_HEAD_DOT = 0, 1, 2

_FP = C.c_void_p  # device pointers travel as integers; so do the float64 ones, device and host
_I32 = C.c_int32
# every symbol include/guardx_cfit.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxq_last_error": (C.c_char_p, []),
    "gxq_build_id": (C.c_char_p, []),
    "gxq_param_count": (C.c_int64, [_I32, _I32, _I32]),
    "gxq_default_workgroups": (C.c_int32, [_I32]),
    "gxq_work_bytes": (C.c_int64, [_I32, _I32, _I32, _I32, _I32]),
    "gxq_softplus_probe": (C.c_int, [_I32, _FP, _FP, _FP, C.c_void_p]),
    "gxq_gradient": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _FP, _FP, _FP, _FP, _FP, _FP, _I32, C.c_void_p, _FP, _FP,
                               C.c_void_p, C.c_void_p]),
    "gxq_fit": (C.c_int, [_I32, _I32, _I32, _I32, _I32, _FP, _FP, _FP, C.c_int64, _FP, _FP, _FP, C.c_int64, _FP, _FP, _I32,
                          C.c_void_p, _I32, C.c_void_p, _FP, C.c_void_p, C.c_void_p]),
}

_side = _sidelib.Binding("cfit", "gxq", SYMBOLS, GXQ_OK, "cfit")
LIB_PATH, load, check, GxqError = _side.path, _side.load, _side.check, _side.Error
