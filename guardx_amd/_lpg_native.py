"""ctypes binding of libguardx_lpg.so (include/guardx_lpg.h): the LPG policy step and its projection probe.

load / check / GxpError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXP_OK, GXP_ERR_ARG, GXP_ERR_UNSUPPORTED, GXP_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers


class GxpStepArgs(C.Structure):
    """gxp_step_args, field for field"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("N", C.c_int32), ("D", C.c_int32), ("A", C.c_int32),
        ("hidden", C.c_int32), ("c_hidden", C.c_int32), ("env_offset", C.c_int32), ("T", C.c_int32), ("t", C.c_int32),
        ("correct", C.c_int32), ("store_init", C.c_int32), ("seed", C.c_uint32 * 2), ("step0", C.c_uint32),
        ("delta", C.c_float), ("grad_scale", C.c_float), ("step_sign", C.c_float),
        ("d_params", _FP), ("d_c_params", _FP), ("d_work", _FP), ("d_obs0", _FP), ("d_obs_rd", _FP),
        ("d_rew_in", _FP), ("d_cost_in", _FP), ("d_done_in", _FP), ("d_q_init", _FP),
        ("d_obs", _FP), ("d_act", _FP), ("d_act_safe", _FP), ("d_mu", _FP), ("d_logp", _FP),
        ("d_val", _FP), ("d_qc", _FP), ("d_lam", _FP), ("d_rew", _FP), ("d_cost", _FP), ("d_done", _FP),
        ("d_obs_last", _FP), ("d_val_last", _FP), ("d_logstd", _FP),
    ]


# every symbol include/guardx_lpg.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxp_last_error": (C.c_char_p, []),
    "gxp_build_id": (C.c_char_p, []),
    "gxp_params_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxp_q_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxp_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gxp_probe_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxp_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "gxp_policy_step": (C.c_int, [C.POINTER(GxpStepArgs), C.c_void_p]),
    "gxp_projection_probe": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, _FP, _FP, C.c_float,
                                       C.c_float, C.c_float, _FP, _FP, _FP, _FP, _FP, C.c_void_p]),
}

# the one-episode entries, declared in the same header under the library's full name (not part of the gxp_ set above)
EPISODE_SYMBOLS = {
    "guardx_lpg_policy_step_episode": (C.c_int, [C.POINTER(GxpStepArgs), _FP, C.c_void_p]),   # (args, gx_first_done_state*, stream)
    "guardx_lpg_tail_probe": (C.c_int, [C.c_int32] * 5 + [_FP] * 6 + [C.c_void_p]),
}

_side = _sidelib.Binding("lpg", "gxp", {**SYMBOLS, **EPISODE_SYMBOLS}, GXP_OK, "lpg")
LIB_PATH, load, check, GxpError = _side.path, _side.load, _side.check, _side.Error
