"""ctypes binding of libguardx_safelayer.so (include/guardx_safelayer.h): the safety-layer policy step.

load / check / GxlError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXL_OK, GXL_ERR_ARG, GXL_ERR_UNSUPPORTED, GXL_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers


class GxlStepArgs(C.Structure):
    """gxl_step_args, field for field"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("N", C.c_int32), ("D", C.c_int32), ("A", C.c_int32),
        ("hidden", C.c_int32), ("g_hidden", C.c_int32), ("env_offset", C.c_int32), ("T", C.c_int32), ("t", C.c_int32),
        ("correct", C.c_int32), ("seed", C.c_uint32 * 2), ("step0", C.c_uint32), ("delta", C.c_float),
        ("d_params", _FP), ("d_g_params", _FP), ("d_work", _FP), ("d_obs0", _FP), ("d_obs_rd", _FP),
        ("d_rew_in", _FP), ("d_cost_in", _FP), ("d_done_in", _FP), ("d_prev_c", _FP),
        ("d_obs", _FP), ("d_act", _FP), ("d_act_safe", _FP), ("d_mu", _FP), ("d_g", _FP), ("d_logp", _FP),
        ("d_val", _FP), ("d_rew", _FP), ("d_cost", _FP), ("d_done", _FP), ("d_prev_cost", _FP),
        ("d_obs_last", _FP), ("d_val_last", _FP), ("d_logstd", _FP),
    ]


# every symbol include/guardx_safelayer.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxl_last_error": (C.c_char_p, []),
    "gxl_build_id": (C.c_char_p, []),
    "gxl_params_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxl_g_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxl_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gxl_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "gxl_policy_step": (C.c_int, [C.POINTER(GxlStepArgs), C.c_void_p]),
    "gxl_correction_probe": (C.c_int, [C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_float, _FP, C.c_void_p]),
}

# the one-episode entries, declared in the same header under the library's full name (not part of the gxl_ set above)
EPISODE_SYMBOLS = {
    "guardx_safelayer_policy_step_episode": (C.c_int, [C.POINTER(GxlStepArgs), _FP, C.c_void_p]),   # (args, gx_first_done_state*, stream)
    "guardx_safelayer_tail_probe": (C.c_int, [C.c_int32] * 5 + [_FP] * 6 + [C.c_void_p]),
}

_side = _sidelib.Binding("safelayer", "gxl", {**SYMBOLS, **EPISODE_SYMBOLS}, GXL_OK, "safelayer")
LIB_PATH, load, check, GxlError = _side.path, _side.load, _side.check, _side.Error
