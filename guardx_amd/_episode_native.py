"""ctypes binding of libguardx_episode.so (include/guardx_episode.h): the one-episode policy step and the one-episode
buffer's finish_path + get.

load / check / GxeError: guardx_amd/_sidelib.py (no CPU fallback; a library built from other sources is refused).
"""
import ctypes as C

from . import _sidelib

GXE_OK, GXE_ERR_ARG, GXE_ERR_UNSUPPORTED, GXE_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers


class GxeStepArgs(C.Structure):
    """gxe_step_args, field for field"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("N", C.c_int32), ("D", C.c_int32), ("A", C.c_int32),
        ("hidden", C.c_int32), ("vc_hidden", C.c_int32), ("has_vc", C.c_int32), ("env_offset", C.c_int32),
        ("T", C.c_int32), ("t", C.c_int32), ("t_base", C.c_int32), ("seed", C.c_uint32 * 2), ("step0", C.c_uint32),
        ("d_params", _FP), ("d_vc_params", _FP), ("d_work", _FP), ("d_obs0", _FP), ("d_obs_rd", _FP),
        ("d_rew_in", _FP), ("d_cost_in", _FP), ("d_done_in", _FP),
        ("d_first_done", _FP), ("d_ep_ret", _FP), ("d_ep_cost", _FP), ("d_ep_len", _FP),
        ("d_obs", _FP), ("d_act", _FP), ("d_mu", _FP), ("d_logp", _FP), ("d_val", _FP), ("d_vc", _FP),
        ("d_rew", _FP), ("d_cost", _FP), ("d_done", _FP),
        ("d_obs_last", _FP), ("d_val_last", _FP), ("d_vc_last", _FP), ("d_logstd", _FP),
    ]


class GxeFinishCol(C.Structure):
    """gxe_finish_col, field for field"""
    _fields_ = [("d_src", _FP), ("d_dst", _FP), ("width", C.c_int32)]


FINISH_MAX_COLS = 4  # GXE_FINISH_MAX_COLS

_I = C.c_int32
# every symbol include/guardx_episode.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxe_last_error": (C.c_char_p, []),
    "gxe_build_id": (C.c_char_p, []),
    "gxe_params_floats": (C.c_int64, [_I, _I, _I]),
    "gxe_vc_floats": (C.c_int64, [_I, _I]),
    "gxe_work_floats": (C.c_int64, [_I, _I, _I, _I]),
    "gxe_prepare": (C.c_int, [_I, _I, _I, _I, _FP, _FP, _FP, C.c_void_p]),
    "gxe_policy_step": (C.c_int, [C.POINTER(GxeStepArgs), C.c_void_p]),
    "gxe_tail_probe": (C.c_int, [_I] * 6 + [_FP] * 7 + [C.c_void_p]),
    "gxe_finish_work_floats": (C.c_int64, [_I, _I]),
    "gxe_finish": (C.c_int, [_I, _I, _I, _I, C.c_float, C.c_float] + [_FP] * 21 + [C.c_void_p]),
}
# gxe_finish with extra columns, declared in the same header under the library's full name (not part of the gxe_ set
# above): (..., n_cols, gxe_finish_col*, d_qc, d_qcost, d_targetc, d_n_valid, stream)
COLS_SYMBOLS = {
    "guardx_episode_finish_cols": (C.c_int, [_I, _I, _I, _I, C.c_float, C.c_float] + [_FP] * 20 + [_I] + [_FP] * 5 + [C.c_void_p]),
}

_side = _sidelib.Binding("episode", "gxe", {**SYMBOLS, **COLS_SYMBOLS}, GXE_OK, "episode")
LIB_PATH, load, check, GxeError = _side.path, _side.load, _side.check, _side.Error
