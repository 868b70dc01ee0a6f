"""Build identity and C ABI of the nine libraries (guardx_amd/build.py: MAIN and LIBRARIES), one case per library: what
each is declared to be built from, that its id covers exactly the files it includes, the recorded ids
(tests/build_ids.py), and that its binding, its header and its export list agree.  No GPU: hipcc cross-compiles."""
import ctypes as C
import hashlib
import importlib
import os
import re
import subprocess

import pytest

from build_ids import IDS, ROWS
import side_abi
from guardx_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = list(ROWS)
SIDE_KEYS = KEYS[1:]


def _library(key):
    return build.MAIN if key == "hip" else build.LIBRARIES[key]


def _native(key):
    return importlib.import_module("guardx_amd._native" if key == "hip" else "guardx_amd._%s_native" % key)


def _norm(name):
    return os.path.normpath(os.path.join(build.CSRC, name))


def _hashed(key):
    lib = _library(key)
    return {_norm(n) for n in lib.sources + lib.headers}


def _closure(key):
    """every file the library's sources reach through #include "...", themselves included"""
    seen, todo = set(), [_norm(s) for s in _library(key).sources]
    while todo:
        path = todo.pop()
        if path not in seen:
            seen.add(path)
            todo += [os.path.normpath(os.path.join(os.path.dirname(path), i))
                     for i in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)]
    return seen


def _declared(key):
    """the functions the library's header declares: under its prefix, and under its full name"""
    text = side_abi.header(key) if key != "hip" else \
        re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "guardx.h")).read(), flags=re.S)
    return set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % ROWS[key].prefix, text)), \
        set(re.findall(r"\b(guardx_%s_[a-z_0-9]+)\s*\(" % key, text))


def _recorded():
    return open(os.path.join(ROOT, "profiles", "r05_build_id.txt")).read().split(None, 1)


# ---------------------------------------------------------------------------------------------------------------------
# what each library is declared to be, and what its id covers
# ---------------------------------------------------------------------------------------------------------------------
def test_one_registry_in_build_order():
    assert KEYS == ["hip", "critic", "statewise", "safelayer", "usl", "lpg", "episode", "mathprobe", "epstats"] == list(IDS)
    assert build.MAIN.key == "hip" and list(build.LIBRARIES) == SIDE_KEYS and not hasattr(build, "POST_LIBRARIES")
    assert (build.LIB, build.SOURCES, build.HEADERS) == (build.MAIN.lib, build.MAIN.sources, build.MAIN.headers)
    assert build.MAIN.per_source_flags is build.PER_SOURCE_FLAGS and len(build.SOURCES) == 12
    sources = [s for key in KEYS for s in _library(key).sources]
    assert len(set(sources)) == len(sources)                      # no source file belongs to two libraries


@pytest.mark.parametrize("key", KEYS)
def test_declaration(key):
    lib, n = _library(key), _native(key)
    assert lib.macro == ROWS[key].macro == ROWS[key].prefix.upper() + "_BUILD_ID"
    assert os.path.basename(lib.lib) == "libguardx_%s.so" % key and n.LIB_PATH == lib.lib
    if key != "hip":
        assert lib.sources == ["gx_%s.hip" % key] and lib.obj_dir is None and lib.per_source_flags is None
    id_file = "BUILD_ID" if key == "hip" else key.upper() + "_BUILD_ID"
    assert lib.build_id_file == os.path.join(build.LIB_DIR, id_file)
    assert "guardx_amd/lib/" + id_file in open(os.path.join(ROOT, ".gitignore")).read().split()


@pytest.mark.parametrize("key", KEYS)
def test_the_id_covers_exactly_what_the_library_includes(key):
    lib = _library(key)
    assert len(lib.sources + lib.headers) == len(_hashed(key))
    assert _hashed(key) == _closure(key)
    # source_hash() restated over that closure: the names as the registry spells them, then the flags
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure(key)):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr((build.FLAGS, sorted(build.PER_SOURCE_FLAGS.items())) if key == "hip" else build.FLAGS).encode())
    assert lib.source_hash() == h.hexdigest()[:24]


def test_what_the_libraries_share_and_what_they_do_not():
    by = {key: {os.path.basename(p) for p in _hashed(key)} for key in KEYS}
    users = lambda name: [key for key in KEYS if name in by[key]]   # noqa: E731
    assert users("gx_qstep.h") == users("gx_qcritic.h") == ["usl", "lpg"]
    assert users("gx_step.h") == ["statewise", "safelayer", "usl", "lpg", "episode"]    # not the main library, not critic
    assert users("gx_device.h") == users("gx_policy.h") == [k for k in KEYS if k != "epstats"]
    assert by["epstats"] == {"gx_epstats.hip", "guardx_epstats.h"}
    assert by["critic"] == {"gx_critic.hip", "gx_device.h", "gx_policy.h", "guardx_critic.h"} \
        and by["mathprobe"] == {"gx_mathprobe.hip", "gx_device.h", "gx_policy.h", "guardx_mathprobe.h"}
    for key in KEYS:                                              # a library's source and public header are its own
        own = set(_library(key).sources) | {"guardx.h" if key == "hip" else "guardx_%s.h" % key}
        assert own <= by[key] and not any(own & by[other] for other in KEYS if other != key), key


@pytest.mark.parametrize("key", KEYS)
def test_the_id_is_the_recorded_one(key):
    got = _library(key).source_hash()
    assert re.fullmatch(r"[0-9a-f]{24}", got)
    recorded, compiler = _recorded()
    if key == "hip":
        assert got == recorded == IDS["hip"]
    elif build.compiler_id() in compiler:
        assert got == IDS[key]


def test_the_ids_are_distinct():
    assert len({_library(key).source_hash() for key in KEYS}) == 9 == len(set(IDS.values()))


@pytest.mark.parametrize("key", KEYS)
def test_the_hash_changes_with_each_of_its_files(key, monkeypatch, tmp_path):
    lib = _library(key)
    before = lib.source_hash()
    csrc = tmp_path / "guardx_amd" / "csrc"
    for name in lib.sources + lib.headers:
        copy = csrc / name
        copy.parent.mkdir(parents=True, exist_ok=True)
        copy.write_bytes(open(os.path.join(build.CSRC, name), "rb").read())
    monkeypatch.setattr(build, "CSRC", str(csrc))
    assert lib.source_hash() == before                            # the copy is the tree
    for name in lib.sources + lib.headers:
        text = (csrc / name).read_bytes()
        (csrc / name).write_bytes(text + b"\n")
        assert lib.source_hash() != before, name
        (csrc / name).write_bytes(text)
    assert lib.source_hash() == before


# ---------------------------------------------------------------------------------------------------------------------
# binding, header and export list
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", SIDE_KEYS)      # the main library's: tests/test_native_abi.py
def test_the_binding_matches_the_header(key):
    row, n = ROWS[key], _native(key)
    side_abi.assert_binding_matches_the_header(key, row.prefix, n, row.step_args and getattr(n, row.step_args),
                                               row.protos, row.values)
    extra = getattr(n, row.extra) if row.extra else {}
    assert set(extra) == _declared(key)[1] and n._side.symbols == {**n.SYMBOLS, **extra}


def test_the_mathprobe_report_matches_the_header():
    from guardx_amd import _mathprobe_native as n
    hdr = side_abi.header("mathprobe")
    assert int(re.search(r"#define GXM_REPORT_LOWEST (\d+)", hdr).group(1)) == n.GXM_REPORT_LOWEST == 16
    body = re.search(r"typedef struct gxm_sweep_report \{(.*?)\} gxm_sweep_report;", hdr, flags=re.S).group(1)
    base = {"uint64_t": C.c_uint64, "uint32_t": C.c_uint32}
    want = [(nm, base[t] * (n.GXM_REPORT_LOWEST if k == "GXM_REPORT_LOWEST" else int(k)) if k else base[t])
            for t, nm, k in re.findall(r"(uint64_t|uint32_t)\s+(\w+)(?:\[(\w+)\])?;", body)]
    assert [(f[0], f[1]) for f in n.GxmSweepReport._fields_] == want and C.sizeof(n.GxmSweepReport) == 80


@pytest.fixture(scope="module")
def defined():
    """{key: {symbol: type}} of what each built library defines (nm -D)"""
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    out = {}
    for key in KEYS:
        nm = subprocess.run(["nm", "-D", "--defined-only", _library(key).lib], capture_output=True, text=True, check=True).stdout
        out[key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


@pytest.mark.parametrize("key", KEYS)
def test_the_export_list_is_the_header_and_nobody_elses(key, defined):
    n = _native(key)
    declared = set.union(*_declared(key))
    assert len(_declared(key)[0]) == ROWS[key].protos
    assert {s for s, t in defined[key].items() if t == "T" and s.startswith(("gx", "guardx_"))} == declared == set(n._side.symbols)
    for other in KEYS:
        assert other == key or not declared & set(defined[other]), other


@pytest.mark.parametrize("key", KEYS)
def test_the_build_id_round_trip(key, defined):
    lib = _native(key).load()          # refuses a library whose build id is not the tree's
    embedded = getattr(lib, ROWS[key].prefix + "_build_id")().decode()
    assert embedded == _library(key).source_hash() == _library(key).built_id()


@pytest.mark.parametrize("key", KEYS)
def test_a_foreign_build_id_is_refused(key, defined, monkeypatch):
    n = _native(key)
    monkeypatch.setattr(n._side, "_lib", None)
    monkeypatch.setattr(_library(key), "source_hash", lambda: "0" * 24)
    monkeypatch.setattr(_library(key), "needs_build", lambda: False)
    with pytest.raises(ImportError, match="built from other sources"):
        n.load()


def test_the_experimental_path_of_the_main_library_skips_the_id_check(defined, monkeypatch, tmp_path):
    """GX_LIB alone changes nothing; with GX_LIB_EXPERIMENT=1 that file is loaded, with a warning, whatever its id"""
    from guardx_amd import _native as n
    variant = str(tmp_path / "libguardx_hip_variant.so")
    os.symlink(build.LIB, variant)
    monkeypatch.setattr(n._side, "_lib", None)
    monkeypatch.setattr(build.MAIN, "source_hash", lambda: "0" * 24)
    monkeypatch.setattr(build.MAIN, "needs_build", lambda: False)
    monkeypatch.setenv("GX_LIB", variant)
    monkeypatch.delenv("GX_LIB_EXPERIMENT", raising=False)
    with pytest.raises(ImportError, match="built from other sources"):
        n.load()
    monkeypatch.setenv("GX_LIB_EXPERIMENT", "1")
    with pytest.warns(RuntimeWarning, match="EXPERIMENTAL library " + re.escape(variant)):
        assert n.load().gx_build_id().decode() == build.MAIN.built_id()
