"""ctypes binding of libguardx_critic.so (include/guardx_critic.h): the batched cost critic.

Like _native, there is no CPU fallback: a missing library is built in place with hipcc, and a library built from other
sources than the tree's is refused.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libguardx_critic.so")

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

_lib = None


def load():
    """Load libguardx_critic.so; raises (never falls back) when it is unavailable or was built from other sources."""
    global _lib
    if _lib is not None:
        return _lib
    from . import build as _build
    want = _build.critic_source_hash()
    if _build.critic_needs_build():
        try:
            _build.build(force=False)
        except Exception as exc:  # noqa: BLE001
            raise ImportError(
                f"{LIB_PATH} is missing or stale (sources {want}, library {_build.built_critic_id()}) and could not be "
                f"built with hipcc ({exc}); run `python -m guardx_amd.build`") from exc
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the ABI drifted
        fn.restype = res
        fn.argtypes = args
    got = lib.gxc_build_id().decode()
    if got != want:
        raise ImportError(f"{LIB_PATH} was built from other sources (library {got}, tree {want}); "
                          "run `python -m guardx_amd.build`")
    _lib = lib
    return lib


class GxcError(RuntimeError):
    def __init__(self, status, msg):
        super().__init__(f"guardx critic status {status}: {msg}")
        self.status = status


def check(status):
    if status != GXC_OK:
        msg = load().gxc_last_error()
        raise GxcError(status, msg.decode() if msg else "")
