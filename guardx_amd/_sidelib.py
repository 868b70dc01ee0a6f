"""What the ctypes bindings of the libraries (guardx_amd/build.py: actor_libraries() and what safety_libraries() adds to
it) share: load(), check() and
the error class.  There is no CPU fallback: a missing library is built in place with hipcc, and a library built from
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
    """load / check / Error of one library of guardx_amd/build.py.  `key`: its key there; `prefix`: that of its C
    symbols ("gxu"); `symbols`: name -> (restype, argtypes); `ok`: its OK status; `label`: its name in the error text
    ("usl", None for the main library).  Two hooks, for the main library: `other_path()` may name another file to load,
    whose build id is then not checked; `loaded(lib)` runs once on the library that passed."""

    def __init__(self, key, prefix, symbols, ok, label, other_path=None, loaded=None):
        self.side = {lib.key: lib for lib in _build.safety_libraries()}[key]
        self.prefix, self.symbols, self.ok = prefix, symbols, ok
        self.path = self.side.lib
        self.other_path, self.loaded = other_path, loaded
        self._lib = None
        where = f"guardx {label} status" if label else "guardx status"

        class Error(RuntimeError):
            def __init__(self, status, msg):
                super().__init__(f"{where} {status}: {msg}")
                self.status = status

        Error.__name__ = Error.__qualname__ = prefix.capitalize() + "Error"
        self.Error = Error

        def check(status):   # a closure: when the status is OK a call costs one comparison
            if status != ok:
                msg = getattr(self.load(), prefix + "_last_error")()
                raise Error(status, msg.decode() if msg else "")

        self.check = check

    def load(self):
        """Load the library; raises (never falls back) when it is unavailable or was built from other sources.

        The library carries the hash of the sources it was built from (gx?_build_id).  If the file is missing or the
        hash on disk differs from the sources in the tree it is rebuilt in place with hipcc (one process at a time:
        guardx_amd.build takes a file lock and renames the finished file into place); a library whose embedded id does
        not match after that is refused."""
        if self._lib is not None:
            return self._lib
        side = self.side
        want = side.source_hash()
        if side.needs_build():
            try:
                _build.build(force=False)
            except Exception as exc:  # noqa: BLE001
                raise ImportError(
                    f"{self.path} is missing or stale (sources {want}, library {side.built_id()}) and could not be "
                    f"built with hipcc ({exc}); run `python -m guardx_amd.build` (guardx_amd has no CPU fallback)") from exc
        path = self.other_path and self.other_path() or self.path
        lib = C.CDLL(path)
        for name, (res, args) in self.symbols.items():
            fn = getattr(lib, name)  # AttributeError if the ABI drifted
            fn.restype = res
            fn.argtypes = args
        got = getattr(lib, self.prefix + "_build_id")().decode()
        if got != want and path == self.path:
            raise ImportError(f"{path} was built from other sources (library {got}, tree {want}); "
                              "run `python -m guardx_amd.build`")
        if self.loaded:
            self.loaded(lib)
        self._lib = lib
        return lib
