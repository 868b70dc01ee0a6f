"""The C header of a side library (include/guardx_<key>.h, prefix gx?_) parsed into ctypes prototypes, and the
comparison of the library's binding (guardx_amd/_<key>_native.py) with it (tests/test_build_identity.py)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header(key):
    text = open(os.path.join(ROOT, "include", "guardx_%s.h" % key)).read()
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _ctype(decl, prefix, step_args):
    base = {"int32_t": C.c_int32, "uint32_t": C.c_uint32, "int64_t": C.c_int64, prefix + "_status": C.c_int,
            "float": C.c_float, "const char*": C.c_char_p, "void*": C.c_void_p, "const float*": C.c_void_p,
            "float*": C.c_void_p, "int32_t*": C.c_void_p,
            # the mathprobe library's: counters, a 64-bit count, its report (a device address like every d_ argument)
            "uint64_t": C.c_uint64, "const uint32_t*": C.c_void_p, prefix + "_sweep_report*": C.c_void_p}
    t = re.sub(r"\s+", " ", decl.strip())
    t = re.sub(r"\s*\*\s*", "* ", t).strip()
    t = re.sub(r"\s+[A-Za-z_][A-Za-z_0-9]*$", "", t) if not t.endswith("*") and " " in t else t
    t = t.strip()
    return C.POINTER(step_args) if t == "const %s_step_args*" % prefix else base[t]


def prototypes(key, prefix, step_args):
    """{name: (restype, [argtypes])} of every gx?_ function the header declares"""
    protos = {}
    for ret, name, args in re.findall(r"([A-Za-z_0-9 ]+?\*?)\s*\b(%s_[a-z_0-9]+)\s*\(([^)]*)\)\s*;" % prefix, header(key)):
        args = args.strip()
        argt = [] if args in ("", "void") else [_ctype(a, prefix, step_args) for a in args.split(",")]
        ret = ret.strip()
        protos[name] = (_ctype(ret if ret.endswith("*") else ret + " x", prefix, step_args), argt)
    return protos


def struct_fields(key, prefix):
    """the fields of gx?_step_args in the header, in order, as ctypes"""
    body = re.search(r"typedef struct %s_step_args \{(.*?)\} %s_step_args;" % (prefix, prefix), header(key), flags=re.S).group(1)
    base = {"const float*": C.c_void_p, "float*": C.c_void_p, "int32_t*": C.c_void_p, "uint32_t": C.c_uint32,
            "int32_t": C.c_int32, "float": C.c_float}
    fields = []
    for stmt in body.split(";"):
        stmt = stmt.strip()
        if not stmt:
            continue
        m = re.match(r"(const float\*|float\*|int32_t\*|uint32_t|int32_t|float)\s+(.*)", stmt)
        for nm in m.group(2).split(","):
            nm = nm.strip()
            arr = re.match(r"(\w+)\[(\d+)\]", nm)
            fields.append((arr.group(1), base[m.group(1)] * int(arr.group(2))) if arr else (nm, base[m.group(1)]))
    return fields


def assert_binding_matches_the_header(key, prefix, n, step_args, count, values=4):
    """the `count` prototypes, the fields of gx?_step_args in order (if the library has one) and the `values`
    enumerators, the four status values among them, of binding module `n`"""
    protos = prototypes(key, prefix, step_args)
    assert sorted(protos) == sorted(n.SYMBOLS) and len(protos) == count
    for name, (res, args) in protos.items():
        assert n.SYMBOLS[name] == (res, args), name
    if step_args is not None:
        assert [(f[0], f[1]) for f in step_args._fields_] == struct_fields(key, prefix)
    P = prefix.upper()
    have = {k: int(v) for k, v in re.findall(r"\b(%s_[A-Z_0-9]+) = (\d+)" % P, header(key))}
    assert len(have) == values and have == {k: getattr(n, k) for k in have}
    assert {k: have[P + "_" + k] for k in ("OK", "ERR_ARG", "ERR_UNSUPPORTED", "ERR_HIP")} == \
        {"OK": 0, "ERR_ARG": 1, "ERR_UNSUPPORTED": 2, "ERR_HIP": 4}
