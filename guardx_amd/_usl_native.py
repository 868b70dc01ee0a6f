"""ctypes binding of libguardx_usl.so (include/guardx_usl.h): the USL policy step and its correction probe.

Like _native, _critic_native, _statewise_native and _safelayer_native, there is no CPU fallback: a missing library is built in place with
hipcc, and a library built from other sources than the tree's is refused.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libguardx_usl.so")

GXU_OK, GXU_ERR_ARG, GXU_ERR_UNSUPPORTED, GXU_ERR_HIP = 0, 1, 2, 4

_FP = C.c_void_p  # device pointers travel as integers


class GxuStepArgs(C.Structure):
    """gxu_step_args, field for field"""
    _fields_ = [
        ("struct_size", C.c_uint32), ("N", C.c_int32), ("D", C.c_int32), ("A", C.c_int32),
        ("hidden", C.c_int32), ("c_hidden", C.c_int32), ("env_offset", C.c_int32), ("T", C.c_int32), ("t", C.c_int32),
        ("correct", C.c_int32), ("niter", C.c_int32), ("seed", C.c_uint32 * 2), ("step0", C.c_uint32),
        ("delta", C.c_float), ("eta", C.c_float), ("grad_scale", C.c_float),
        ("d_params", _FP), ("d_c_params", _FP), ("d_work", _FP), ("d_obs0", _FP), ("d_obs_rd", _FP),
        ("d_rew_in", _FP), ("d_cost_in", _FP), ("d_done_in", _FP),
        ("d_obs", _FP), ("d_act", _FP), ("d_act_safe", _FP), ("d_mu", _FP), ("d_logp", _FP),
        ("d_val", _FP), ("d_qc", _FP), ("d_iters", _FP), ("d_rew", _FP), ("d_cost", _FP), ("d_done", _FP),
        ("d_obs_last", _FP), ("d_val_last", _FP), ("d_logstd", _FP),
    ]


# every symbol include/guardx_usl.h declares: name -> (restype, argtypes)
SYMBOLS = {
    "gxu_last_error": (C.c_char_p, []),
    "gxu_build_id": (C.c_char_p, []),
    "gxu_params_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxu_q_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxu_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32, C.c_int32]),
    "gxu_probe_work_floats": (C.c_int64, [C.c_int32, C.c_int32, C.c_int32]),
    "gxu_prepare": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, C.c_void_p]),
    "gxu_policy_step": (C.c_int, [C.POINTER(GxuStepArgs), C.c_void_p]),
    "gxu_correction_probe": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int32, _FP, _FP, _FP, _FP, C.c_float,
                                       C.c_int32, C.c_float, C.c_float, _FP, _FP, _FP, _FP, _FP, C.c_void_p]),
}

_lib = None


def load():
    """Load libguardx_usl.so; raises (never falls back) when it is unavailable or was built from other sources."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as _build
    want = _build.usl_source_hash()
    if _build.usl_needs_build():
        try:
            _build.build(force=False)
        except Exception as exc:  # noqa: BLE001
            raise ImportError(
                f"{LIB_PATH} is missing or stale (sources {want}, library {_build.built_usl_id()}) and could not "
                f"be built with hipcc ({exc}); run `python -m guardx_amd.build`") from exc
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    got = lib.gxu_build_id().decode()
    if got != want:
        raise ImportError(f"{LIB_PATH} was built from other sources (library {got}, tree {want}); "
                          "run `python -m guardx_amd.build`")
    _lib = lib
    return lib


class GxuError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"guardx usl status {status}: {msg}")
        self.status = status


def check(status):
    if status != GXU_OK:
        msg = load().gxu_last_error()
        raise GxuError(status, msg.decode() if msg else "")
