"""ctypes binding of libguardx_vfit.so (include/guardx_vfit.h): the learners' fit of the value critics (Adam on the MSE
loss) on the device.

load / check / GxvError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXV_OK, GXV_ERR_ARG, GXV_ERR_UNSUPPORTED, GXV_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers; so do the float64 ones, device and host
_I32 = C.c_int32
# every symbol include/guardx_vfit.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxv_last_error": (C.c_char_p, []),
    "gxv_build_id": (C.c_char_p, []),
    "gxv_param_count": (C.c_int64, [_I32, _I32]),
    "gxv_default_workgroups": (C.c_int32, [_I32]),
    "gxv_work_bytes": (C.c_int64, [_I32, _I32, _I32]),
    "gxv_tanh_act": (C.c_int, [_I32, _FP, _FP, C.c_void_p]),
    "gxv_gradient": (C.c_int, [_I32, _I32, _I32, _FP, _FP, _FP, _I32, C.c_void_p, _FP, _FP, C.c_void_p]),
    "gxv_adam_step": (C.c_int, [_I32, _FP, _FP, _FP, _FP, C.c_void_p, C.c_void_p]),
    "gxv_fit": (C.c_int, [_I32, _I32, _I32, _FP, _FP, _FP, C.c_int64, _FP, _FP, _I32, C.c_void_p, _I32, C.c_void_p, _FP,
                          C.c_void_p]),
}

_side = _sidelib.Binding("vfit", "gxv", SYMBOLS, GXV_OK, "vfit")
LIB_PATH, load, check, GxvError = _side.path, _side.load, _side.check, _side.Error
