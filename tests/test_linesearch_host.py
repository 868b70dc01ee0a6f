"""libguardx_linesearch.so without a GPU (hipcc cross-compiles): what tests/test_fisher_host.py asks of the tenth library,
asked of the eleventh -- where it is registered, what its id covers, that its binding, its header and its export list agree,
that a foreign build is refused, that it leaves the other libraries' ids alone -- and every refusal of
guardx_amd.linesearch and of the C entry points, none of which may reach a launch (on a machine without a GPU a launch
would come back as GXB_ERR_HIP, not as the status asserted here)."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fisher64 as f64
import side_abi
from guardx_amd import _linesearch_native as n
from guardx_amd import build, fisher, linesearch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "linesearch", "gxb"
LIB = build.UPDATE_LIBRARIES[KEY]
PROTOS = 7
MINE = ("gx_linesearch.hip", "guardx_linesearch.h")


def _norm(name):
    return os.path.normpath(os.path.join(build.CSRC, name))


def _closure():
    """every file the library's source reaches through #include "...", itself included"""
    seen, todo = set(), [_norm(s) for s in LIB.sources]
    while todo:
        path = todo.pop()
        if path not in seen:
            seen.add(path)
            todo += [os.path.normpath(os.path.join(os.path.dirname(path), i))
                     for i in re.findall(r'^\s*#\s*include\s+"([^"]+)"', open(path).read(), flags=re.M)]
    return seen


def _declared():
    return set(re.findall(r"\b(%s_[a-z_0-9]+)\s*\(" % PREFIX, side_abi.header(KEY)))


# ---------------------------------------------------------------------------------------------------------------------
# registration and identity
# ---------------------------------------------------------------------------------------------------------------------
def test_it_is_registered_in_the_third_mapping_only():
    assert list(build.UPDATE_LIBRARIES) == [KEY] and KEY not in build.LIBRARIES and KEY not in build.LEARNER_LIBRARIES
    assert LIB not in build.every_library()
    assert build.all_libraries() == build.every_library() + [LIB] and len(build.all_libraries()) == 11
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.LEARNER_LIBRARIES["fisher"])
    text = open(os.path.join(ROOT, "guardx_amd", "build.py")).read()
    assert "waits for a pull request that may touch" in text and "UPDATE_LIBRARIES" in text


def test_declaration():
    assert LIB.macro == "GXB_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_linesearch.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_linesearch.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "LINESEARCH_BUILD_ID")
    assert "guardx_amd/lib/LINESEARCH_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_linesearch.hip", "gx_device.h", "gx_policy.h", "guardx_linesearch.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = build.every_library()
    assert LIB.source_hash() not in {o.source_hash() for o in others}
    for o in others:                                              # its source and public header are its own
        assert not set(MINE) & {os.path.basename(x) for x in o.sources + o.headers}


def test_the_hash_changes_with_each_of_its_files(monkeypatch, tmp_path):
    before = LIB.source_hash()
    csrc = tmp_path / "guardx_amd" / "csrc"
    for name in LIB.sources + LIB.headers:
        copy = csrc / name
        copy.parent.mkdir(parents=True, exist_ok=True)
        copy.write_bytes(open(os.path.join(build.CSRC, name), "rb").read())
    monkeypatch.setattr(build, "CSRC", str(csrc))
    assert LIB.source_hash() == before
    for name in LIB.sources + LIB.headers:
        text = (csrc / name).read_bytes()
        (csrc / name).write_bytes(text + b"\n")
        assert LIB.source_hash() != before, name
        (csrc / name).write_bytes(text)
    assert LIB.source_hash() == before


def test_the_other_libraries_ids_do_not_depend_on_the_new_files(monkeypatch, tmp_path):
    """a copy of csrc and include without the two new files gives every other library the id it has in the tree: nothing
    an existing library hashes was touched, and none of them reaches the new files"""
    before = {lib.key: lib.source_hash() for lib in build.every_library()}
    shutil.copytree(build.CSRC, tmp_path / "guardx_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    os.remove(tmp_path / "guardx_amd" / "csrc" / MINE[0])
    os.remove(tmp_path / "include" / MINE[1])
    monkeypatch.setattr(build, "CSRC", str(tmp_path / "guardx_amd" / "csrc"))
    assert {lib.key: lib.source_hash() for lib in build.every_library()} == before
    with pytest.raises(OSError):
        LIB.source_hash()


def test_the_binding_matches_the_header():
    side_abi.assert_binding_matches_the_header(KEY, PREFIX, n, None, PROTOS, 4)
    assert n._side.symbols == n.SYMBOLS and len(_declared()) == PROTOS
    assert not re.search(r"\bdouble\b", side_abi.header(KEY))      # float64 data travels behind void*


@pytest.fixture(scope="module")
def defined():
    """{key: {symbol: type}} of what each built library defines (nm -D)"""
    build.build()
    out = {}
    for lib in build.all_libraries():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_build_builds_eleven_libraries(defined):
    assert len(defined) == 11 and all(os.path.exists(lib.lib) and not lib.needs_build() for lib in build.all_libraries())


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxb_build_id().decode() == LIB.source_hash() == LIB.built_id()


def test_a_foreign_build_id_is_refused(defined, monkeypatch):
    monkeypatch.setattr(n._side, "_lib", None)
    monkeypatch.setattr(LIB, "source_hash", lambda: "0" * 24)
    monkeypatch.setattr(LIB, "needs_build", lambda: False)
    with pytest.raises(ImportError, match="built from other sources"):
        n.load()


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points refuse before they launch
# ---------------------------------------------------------------------------------------------------------------------
PTR = 4096      # a non-null address that nothing may dereference on these paths
BATCH = ("obs", "act", "adv", "logp", "mu", "logstd")
_STEPS = (C.c_double * 4)(1.0, 0.8, 0.64, 0.512)
STEPS = C.cast(_STEPS, C.c_void_p)


def _evaluate(lib, B=64, D=43, A=2, h=64, theta=PTR, d=PTR, adc=None, n_steps=4, steps=STEPS, wg=0, work=PTR, out=PTR, **batch):
    b = [batch.get(k, PTR) for k in BATCH]
    return lib.gxb_evaluate(B, D, A, h, theta, d, *b, adc, n_steps, steps, wg, work, out, None)


def _search(lib, B=64, D=43, A=2, h=64, theta=PTR, d=PTR, adc=None, iters=4, steps=STEPS, crit=PTR, wg=0, work=PTR,
            new=2 * PTR, acc=PTR, means=PTR, trace=PTR, **batch):
    b = [batch.get(k, PTR) for k in BATCH]
    return lib.gxb_search(B, D, A, h, theta, d, *b, adc, iters, steps, crit, wg, work, new, acc, means, trace, None)


def test_sizes(defined):
    lib = n.load()
    for D, A in ((43, 2), (64, 8), (1, 2), (128, 16)):
        assert lib.gxb_param_count(D, A, 64) == f64.param_count(D, A, 64) == fisher.param_count(D, A)
    assert lib.gxb_param_count(43, 2, 8) == f64.param_count(43, 2, 8)
    assert lib.gxb_param_count(0, 2, 64) == lib.gxb_param_count(43, 0, 64) == lib.gxb_param_count(43, 2, 0) == -1
    rows = (0, 1, 64, 65, 256 * 64, 256 * 64 + 1, 512 * 64 + 1, 400000)
    assert [lib.gxb_default_workgroups(B, 43) for B in rows] == [0, 1, 1, 2, 256, 257, 512, 512]      # two workgroups to a CU
    assert [lib.gxb_default_workgroups(B, 64) for B in rows] == [0, 1, 1, 2, 256, 257, 512, 512]
    assert [lib.gxb_default_workgroups(B, 65) for B in rows] == [0, 1, 1, 2, 256, 256, 256, 256]      # one
    assert lib.gxb_default_workgroups(64, 0) == 0
    assert lib.gxb_work_bytes(65, 43, 2, 0) == 32 * 2 + 32 and lib.gxb_work_bytes(65, 43, 2, 5) == 32 * 5 + 32
    assert lib.gxb_work_bytes(400000, 43, 2, 0) == 32 * 512 + 32 and lib.gxb_work_bytes(400000, 70, 10, 0) == 32 * 256 + 32


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    nulls = [dict([(k, None)]) for k in ("theta", "d", "work") + BATCH]
    for kw in nulls + [dict(out=None), dict(steps=None), dict(n_steps=0), dict(n_steps=-1), dict(B=0), dict(B=-1), dict(D=0),
                       dict(A=0), dict(wg=-1), dict(wg=4097)]:
        assert _evaluate(lib, **kw) == n.GXB_ERR_ARG, kw
        assert b"gxb_evaluate" in lib.gxb_last_error()
    for kw in nulls + [dict(crit=None), dict(new=None), dict(acc=None), dict(means=None), dict(trace=None), dict(steps=None),
                       dict(iters=-1), dict(new=PTR), dict(B=0), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097)]:
        assert _search(lib, **kw) == n.GXB_ERR_ARG, kw
        assert b"gxb_search" in lib.gxb_last_error()
    with pytest.raises(n.GxbError, match="guardx linesearch status 1: gxb_search: null pointer") as e:
        n.check(_search(lib, obs=None))
    assert e.value.status == n.GXB_ERR_ARG
    for args in ((0, 43, 2, 0), (64, 0, 2, 0), (64, 43, 0, 0), (64, 43, 2, -1), (64, 43, 2, 4097)):
        assert lib.gxb_work_bytes(*args) == -1, args


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "observation width"),
                     (dict(A=3), "even action width"), (dict(A=18), "even action width"), (dict(A=1), "even action width")):
        assert _evaluate(lib, **kw) == n.GXB_ERR_UNSUPPORTED, kw
        assert word in lib.gxb_last_error().decode()
        assert _search(lib, **kw) == n.GXB_ERR_UNSUPPORTED, kw
    assert lib.gxb_work_bytes(64, 129, 2, 0) == lib.gxb_work_bytes(64, 43, 3, 0) == lib.gxb_work_bytes(64, 43, 18, 0) == -1
    assert lib.gxb_work_bytes(64, 128, 16, 0) > 0 and lib.gxb_work_bytes(1, 1, 2, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.linesearch refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(linesearch._n, "load", refuse)


def _data(B=8, D=43, A=2, **over):
    data = dict(obs=torch.zeros(B, D), act=torch.zeros(B, A), adv=torch.zeros(B), logp=torch.zeros(B), mu=torch.zeros(B, A),
                logstd=torch.zeros(B, A))
    data.update(over)
    return data


def test_actors_it_does_not_support_in_fishers_words(no_library):
    import test_fisher_host as tfh
    for make in (lambda: tfh._Actor(tfh._mods(layers=1), 2), lambda: tfh._Actor(tfh._mods(h=128), 2),
                 lambda: tfh._Actor(tfh._mods(A=3), 3), lambda: tfh._Actor(tfh._mods(D=129), 2), lambda: torch.nn.Linear(3, 2)):
        with pytest.raises(NotImplementedError) as theirs:
            fisher.FisherOperator(make(), torch.zeros(8, 43))
        with pytest.raises(NotImplementedError) as mine:
            linesearch.LineSearch(make(), _data())
        assert str(mine.value) == str(theirs.value).replace("FisherOperator", "LineSearch") and "LineSearch" in str(mine.value)


@pytest.mark.parametrize("over,words", [
    (dict(obs=np.zeros((8, 43), np.float32)), "LineSearch: obs must be a float32 tensor"),
    (dict(obs=torch.zeros(8, 44)), "LineSearch: obs must be (B, 43)"),
    (dict(obs=torch.zeros(8, 50)[:, :43]), "LineSearch: obs must be contiguous"),
    (dict(), "LineSearch: obs lives on cpu; it must be on a cuda device"),
])
def test_batches_it_does_not_accept(over, words, no_library):
    with pytest.raises(ValueError, match=re.escape(words)):
        linesearch.LineSearch(f64.make_actor(43, 2), _data(**over))


def test_a_batch_with_a_key_missing(no_library):
    data = _data()
    del data["mu"]
    with pytest.raises(ValueError, match="LineSearch: data has no 'mu'"):
        linesearch.LineSearch(f64.make_actor(43, 2), data)


def test_the_other_arrays_and_the_criteria(no_library):
    P, dev = fisher.param_count(43, 2), torch.device("cuda:0")
    for name, shape, v, words in (("act", (8, 2), torch.zeros(8, 3), "must be (8, 2)"), ("adv", (8,), torch.zeros(9), "must be (8,)"),
                                  ("logp", (8,), torch.zeros(8, dtype=torch.float64), "must be a float32 tensor"),
                                  ("mu", (8, 2), torch.zeros(8, 4)[:, :2], "must be contiguous"),
                                  ("adc", (8,), torch.zeros(8), "lives on cpu; it must be on cuda:0, where obs is"),
                                  ("x_direction", (P,), torch.zeros(P + 1), f"must be ({P},)")):
        with pytest.raises(ValueError, match=re.escape(f"LineSearch: {name} {words}")):
            linesearch._checked(name, v, shape, dev)
    LS = object.__new__(linesearch.LineSearch)
    LS.P, LS.device, LS.adc = P, dev, None
    with pytest.raises(ValueError, match="x_direction lives on cpu"):
        LS.search(torch.zeros(P), 0.01)
    with pytest.raises(ValueError, match="x_direction must be a float32 tensor"):
        LS.evaluate(np.zeros(P, np.float32), [1.0])
    # the other refusals of search and evaluate come before the direction is looked at
    d = torch.zeros(P)
    with pytest.raises(ValueError, match="iters must be a non-negative integer"):
        LS.search(d, 0.01, iters=-1)
    with pytest.raises(ValueError, match="cost_margin needs data"):
        LS.search(d, 0.01, cost_margin=0.0)
    with pytest.raises(ValueError, match="target_kl must be a number or a tensor of one element"):
        LS.search(d, torch.zeros(2))
    LS.adc = torch.zeros(8)
    with pytest.raises(ValueError, match="cost_margin must be given"):
        LS.search(d, 0.01)
    with pytest.raises(ValueError, match="steps must not be empty"):
        LS.evaluate(d, [])


def test_the_package_exports_it_and_assign_flat_params():
    import guardx_amd
    assert guardx_amd.linesearch is linesearch and guardx_amd.LineSearch is linesearch.LineSearch
    pi, other = f64.make_actor(43, 2, seed=0), f64.make_actor(43, 2, seed=1)
    theta = fisher.flat_params(other)
    assert not torch.equal(fisher.flat_params(pi), theta)
    linesearch.assign_flat_params(pi, theta)
    assert torch.equal(fisher.flat_params(pi), theta)
    with pytest.raises(ValueError, match="assign_flat_params: theta must be"):
        linesearch.assign_flat_params(pi, theta[:-1])
