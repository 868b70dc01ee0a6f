"""ctypes binding of libguardx_mathprobe.so (include/guardx_mathprobe.h): the fp32 device primitives one by one.
Test infrastructure: tests/test_gpu_math64.py calls it, nothing in the product does.

load / check / GxmError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXM_OK, GXM_ERR_ARG, GXM_ERR_UNSUPPORTED, GXM_ERR_HIP = 0, 1, 2, 4

# gxm_fn
(GXM_FN_SINCOS, GXM_FN_SINCOS_FINITE, GXM_FN_ATAN2, GXM_FN_EXP, GXM_FN_LOG, GXM_FN_TANH, GXM_FN_RCP_UNSCALED,
 GXM_FN_DIV_BIN16, GXM_FN_DIV, GXM_FN_RCP, GXM_FN_SQRT, GXM_FN_COUNT) = range(12)
# gxm_pair
GXM_PAIR_RCP, GXM_PAIR_TANH, GXM_PAIR_SINCOS, GXM_PAIR_DIV_BIN16, GXM_PAIR_COUNT = range(5)
GXM_REPORT_LOWEST = 16


class GxmSweepReport(C.Structure):
    """gxm_sweep_report, field for field"""
    _fields_ = [("mismatches", C.c_uint64), ("lowest", C.c_uint32 * GXM_REPORT_LOWEST), ("reserved", C.c_uint32 * 2)]


_FP = C.c_void_p  # device pointers travel as integers
# every symbol include/guardx_mathprobe.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxm_last_error": (C.c_char_p, []),
    "gxm_build_id": (C.c_char_p, []),
    "gxm_eval": (C.c_int, [C.c_int32, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]),
    "gxm_normal_pair": (C.c_int, [C.c_uint32, C.c_uint32, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]),
    "gxm_sweep": (C.c_int, [C.c_int32, C.c_uint32, C.c_uint64, _FP, C.c_void_p]),
}

_side = _sidelib.Binding("mathprobe", "gxm", SYMBOLS, GXM_OK, "mathprobe")
LIB_PATH, load, check, GxmError = _side.path, _side.load, _side.check, _side.Error
