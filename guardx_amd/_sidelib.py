"""What the ctypes bindings of the side libraries (guardx_amd/build.py:LIBRARIES and POST_LIBRARIES) share: load(), check() and the error
class.  Like _native, there is no CPU fallback: a missing library is built in place with hipcc, and a library built from
other sources than the tree's is refused.
"""
import ctypes as C

from . import build as _build


class FirstDoneState(C.Structure):
    """gx_first_done_state (include/guardx_safelayer.h, guardx_usl.h, guardx_lpg.h), field for field: the bookkeeping argument of the
    guardx_<library>_policy_step_episode entries"""
    _fields_ = [("struct_size", C.c_uint32), ("t_base", C.c_int32), ("d_first_done", C.c_void_p),
                ("d_ep_len", C.c_void_p), ("d_ep_ret", C.c_void_p), ("d_ep_cost", C.c_void_p)]


class Binding:
    """load / check / Error of LIBRARIES[key] (or POST_LIBRARIES[key]).  `prefix`: that of its C symbols ("gxu"); `symbols`: name -> (restype,
    argtypes); `ok`: its OK status; `label`: its name in the error text ("usl")."""

    def __init__(self, key, prefix, symbols, ok, label):
        side = _build.LIBRARIES[key] if key in _build.LIBRARIES else _build.POST_LIBRARIES[key]
        self.side, self.prefix, self.symbols, self.ok = side, prefix, symbols, ok
        self.path = self.side.lib
        self._lib = None

        class Error(RuntimeError):
            def __init__(self, status, msg):
                super().__init__(f"guardx {label} status {status}: {msg}")
                self.status = status

        Error.__name__ = Error.__qualname__ = prefix.capitalize() + "Error"
        self.Error = Error

    def load(self):
        """Load the library; raises (never falls back) when it is unavailable or was built from other sources."""
        if self._lib is not None:
            return self._lib
        side, path = self.side, self.path
        want = side.source_hash()
        if side.needs_build():
            try:
                _build.build(force=False)
            except Exception as exc:  # noqa: BLE001
                raise ImportError(
                    f"{path} is missing or stale (sources {want}, library {side.built_id()}) and could not "
                    f"be built with hipcc ({exc}); run `python -m guardx_amd.build`") from exc
        lib = C.CDLL(path)
        for name, (res, args) in self.symbols.items():
            fn = getattr(lib, name)  # AttributeError if the ABI drifted
            fn.restype = res
            fn.argtypes = args
        got = getattr(lib, self.prefix + "_build_id")().decode()
        if got != want:
            raise ImportError(f"{path} was built from other sources (library {got}, tree {want}); "
                              "run `python -m guardx_amd.build`")
        self._lib = lib
        return lib

    def check(self, status):
        if status != self.ok:
            msg = getattr(self.load(), self.prefix + "_last_error")()
            raise self.Error(status, msg.decode() if msg else "")
