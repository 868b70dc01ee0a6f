"""ctypes binding of libguardx_fisher.so (include/guardx_fisher.h): the TRPO family's Fisher-vector product and cg on the
device.

load / check / GxfError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXF_OK, GXF_ERR_ARG, GXF_ERR_UNSUPPORTED, GXF_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers
_I32 = C.c_int32
# every symbol include/guardx_fisher.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxf_last_error": (C.c_char_p, []),
    "gxf_build_id": (C.c_char_p, []),
    "gxf_param_count": (C.c_int64, [_I32, _I32, _I32]),
    "gxf_default_workgroups": (C.c_int32, [_I32]),
    "gxf_work_bytes": (C.c_int64, [_I32, _I32, _I32, _I32]),
    "gxf_fvp": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, C.c_float, C.c_float, _I32, C.c_void_p, _FP, C.c_void_p]),
    "gxf_cg": (C.c_int, [_I32, _I32, _I32, _I32, _FP, _FP, _FP, C.c_float, C.c_float, _I32, _I32, C.c_void_p, _FP, _FP, _FP,
                         _FP, C.c_void_p]),
    "gxf_tanh_act": (C.c_int, [_I32, _FP, _FP, C.c_void_p]),      # test infrastructure: the product's activation alone
}

_side = _sidelib.Binding("fisher", "gxf", SYMBOLS, GXF_OK, "fisher")
LIB_PATH, load, check, GxfError = _side.path, _side.load, _side.check, _side.Error
