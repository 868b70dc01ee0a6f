"""ctypes binding of libguardx_critic.so (include/guardx_critic.h): the batched cost critic.

load / check / GxcError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXC_OK, GXC_ERR_ARG, GXC_ERR_UNSUPPORTED, GXC_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers
# every symbol include/guardx_critic.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxc_last_error": (C.c_char_p, []),
    "gxc_build_id": (C.c_char_p, []),
    "gxc_critic_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "gxc_critic_work_floats": (C.c_int64, [C.c_int32, C.c_int32]),
    "gxc_critic_values": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, _FP, C.c_void_p]),
}

_side = _sidelib.Binding("critic", "gxc", SYMBOLS, GXC_OK, "critic")
LIB_PATH, load, check, GxcError = _side.path, _side.load, _side.check, _side.Error
