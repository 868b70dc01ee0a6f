"""ctypes binding of libguardx_statewise.so (include/guardx_statewise.h): the state-wise (SCPO) policy step.

load / check / GxsError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXS_OK, GXS_ERR_ARG, GXS_ERR_UNSUPPORTED, GXS_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers


class GxsStepArgs(C.Structure):
    """gxs_step_args, field for field"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("N", C.c_int32), ("D_aug", C.c_int32), ("A", C.c_int32),
        ("hidden", C.c_int32), ("vc_hidden", C.c_int32), ("env_offset", C.c_int32), ("T", C.c_int32), ("t", C.c_int32),
        ("seed", C.c_uint32 * 2), ("step0", C.c_uint32),
        ("d_params", _FP), ("d_vc_params", _FP), ("d_work", _FP), ("d_obs0", _FP), ("d_obs_rd", _FP),
        ("d_rew_in", _FP), ("d_cost_in", _FP), ("d_done_in", _FP), ("d_M", _FP), ("d_first", _FP),
        ("d_obs", _FP), ("d_act", _FP), ("d_mu", _FP), ("d_logp", _FP), ("d_val", _FP), ("d_vc", _FP),
        ("d_rew", _FP), ("d_cost", _FP), ("d_done", _FP), ("d_cost_inc", _FP), ("d_M_after", _FP),
        ("d_obs_last", _FP), ("d_val_last", _FP), ("d_vc_last", _FP), ("d_logstd", _FP),
    ]


# every symbol include/guardx_statewise.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxs_last_error": (C.c_char_p, []),
    "gxs_build_id": (C.c_char_p, []),
    "gxs_params_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxs_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gxs_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "gxs_policy_step": (C.c_int, [C.POINTER(GxsStepArgs), C.c_void_p]),
    "gxs_softplus_probe": (C.c_int, [C.c_int32, _FP, _FP, C.c_void_p]),
}

_side = _sidelib.Binding("statewise", "gxs", SYMBOLS, GXS_OK, "statewise")
LIB_PATH, load, check, GxsError = _side.path, _side.load, _side.check, _side.Error
