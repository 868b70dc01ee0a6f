"""libguardx_pgrad.so without a GPU (hipcc cross-compiles): what tests/test_vfit_host.py asks of the twelfth library, asked of
the thirteenth -- where it is registered, what its id covers, that its binding, its header and its export list agree, that a
foreign build is refused, that it leaves the other libraries' ids alone -- and every refusal of guardx_amd.pgrad and of the C
entry points, none of which may reach a launch (on a machine without a GPU a launch would come back as GXG_ERR_HIP, not as
the status asserted here)."""
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
import test_fisher_host as tfh
from guardx_amd import _pgrad_native as n
from guardx_amd import build, fisher, pgrad

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "pgrad", "gxg"
LIB = build.GRAD_LIBRARIES[KEY]
PROTOS = 8
MINE = ("gx_pgrad.hip", "guardx_pgrad.h")


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
def test_it_is_registered_in_the_fifth_mapping_only():
    assert list(build.GRAD_LIBRARIES) == [KEY]
    assert all(KEY not in m for m in (build.LIBRARIES, build.LEARNER_LIBRARIES, build.UPDATE_LIBRARIES, build.FIT_LIBRARIES))
    assert LIB not in build.fit_libraries()
    assert build.grad_libraries() == build.fit_libraries() + [LIB] and len(build.grad_libraries()) == 13
    # the four functions and mappings before it keep their values
    assert list(build.FIT_LIBRARIES) == ["vfit"] and list(build.UPDATE_LIBRARIES) == ["linesearch"] and list(build.LEARNER_LIBRARIES) == ["fisher"]
    assert len(build.fit_libraries()) == 12 and len(build.all_libraries()) == 11 and len(build.every_library()) == 10
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.FIT_LIBRARIES["vfit"])
    text = open(os.path.join(ROOT, "guardx_amd", "build.py")).read()
    assert "GRAD_LIBRARIES" in text and "grad_libraries()" in text


def test_declaration():
    assert LIB.macro == "GXG_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_pgrad.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_pgrad.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "PGRAD_BUILD_ID")
    assert "guardx_amd/lib/PGRAD_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_pgrad.hip", "gx_device.h", "gx_policy.h", "guardx_pgrad.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = build.fit_libraries()
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
    an existing library hashes was touched, none of them reaches the new files, and so none shares a translation unit with
    the new library"""
    before = {lib.key: lib.source_hash() for lib in build.fit_libraries()}
    assert len(before) == 12
    shutil.copytree(build.CSRC, tmp_path / "guardx_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    os.remove(tmp_path / "guardx_amd" / "csrc" / MINE[0])
    os.remove(tmp_path / "include" / MINE[1])
    monkeypatch.setattr(build, "CSRC", str(tmp_path / "guardx_amd" / "csrc"))
    assert {lib.key: lib.source_hash() for lib in build.fit_libraries()} == before
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
    for lib in build.grad_libraries():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_build_builds_thirteen_libraries(defined):
    assert len(defined) == 13 and all(os.path.exists(lib.lib) and not lib.needs_build() for lib in build.grad_libraries())


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxg_build_id().decode() == LIB.source_hash() == LIB.built_id()


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


def _gradient(lib, B=64, D=43, A=2, h=64, theta=PTR, obs=PTR, act=PTR, adv=PTR, logp=PTR, adc=PTR, wg=0, work=PTR, g=PTR, b=PTR, info=PTR):
    return lib.gxg_gradient(B, D, A, h, theta, obs, act, adv, logp, adc, wg, work, g, b, info, None)


def _cpo(lib, P=100, b=PTR, hg=PTR, hb=PTR, ag=PTR, s=PTR, crit=PTR, x=PTR, case=PTR, out=PTR):
    return lib.gxg_cpo_direction(P, b, hg, hb, ag, s, crit, x, case, out, None)


def _trpo(lib, P=100, x_hat=PTR, s=PTR, tkl=PTR, x=PTR):
    return lib.gxg_trpo_direction(P, x_hat, s, tkl, x, None)


def test_sizes(defined):
    lib = n.load()
    for D, A in ((43, 2), (64, 8), (1, 16), (128, 2)):
        assert lib.gxg_param_count(D, A, 64) == f64.param_count(D, A, 64) == fisher.param_count(D, A)
    assert lib.gxg_param_count(43, 2, 8) == f64.param_count(43, 2, 8)
    assert lib.gxg_param_count(0, 2, 64) == lib.gxg_param_count(43, 0, 64) == lib.gxg_param_count(43, 2, 0) == -1
    rows = (0, -1, 1, 64, 65, 256 * 64, 256 * 64 + 1, 400000, 2 ** 31 - 1)
    assert [lib.gxg_default_workgroups(B) for B in rows] == [0, 0, 1, 1, 2, 256, 256, 256, 256]
    P = f64.param_count(43, 2, 64)
    # two partial vectors of P float32 and 36 float64 per workgroup, with and without adc
    assert lib.gxg_work_bytes(65, 43, 2, 0) == 4 * 2 * 2 * P + 8 * 36 * 2
    assert lib.gxg_work_bytes(65, 43, 2, 5) == 4 * 2 * 5 * P + 8 * 36 * 5
    assert lib.gxg_work_bytes(400000, 43, 2, 0) == 4 * 2 * 256 * P + 8 * 36 * 256


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    for kw in [dict([(k, None)]) for k in ("theta", "obs", "act", "adv", "logp", "work", "g", "info")] + \
            [dict(B=0), dict(B=-1), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097), dict(adc=None), dict(b=None)]:
        assert _gradient(lib, **kw) == n.GXG_ERR_ARG, kw
        assert b"gxg_gradient" in lib.gxg_last_error()
    for kw in [dict([(k, None)]) for k in ("b", "hg", "hb", "ag", "s", "crit", "x", "case", "out")] + [dict(P=0), dict(P=-1)]:
        assert _cpo(lib, **kw) == n.GXG_ERR_ARG, kw
        assert b"gxg_cpo_direction" in lib.gxg_last_error()
    for kw in [dict([(k, None)]) for k in ("x_hat", "s", "tkl", "x")] + [dict(P=0), dict(P=-1)]:
        assert _trpo(lib, **kw) == n.GXG_ERR_ARG, kw
        assert b"gxg_trpo_direction" in lib.gxg_last_error()
    with pytest.raises(n.GxgError, match="guardx pgrad status 1: gxg_gradient: null pointer") as e:
        n.check(_gradient(lib, obs=None))
    assert e.value.status == n.GXG_ERR_ARG
    for args in ((0, 43, 2, 0), (64, 0, 2, 0), (64, 43, 0, 0), (64, 43, 2, -1), (64, 43, 2, 4097)):
        assert lib.gxg_work_bytes(*args) == -1, args


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "observation width"),
                     (dict(A=3), "even action width"), (dict(A=18), "even action width")):
        assert _gradient(lib, **kw) == n.GXG_ERR_UNSUPPORTED, kw
        assert word in lib.gxg_last_error().decode()
        assert _gradient(lib, adc=None, b=None, **kw) == n.GXG_ERR_UNSUPPORTED, kw
    assert lib.gxg_work_bytes(64, 129, 2, 0) == lib.gxg_work_bytes(64, 43, 3, 0) == lib.gxg_work_bytes(64, 43, 18, 0) == -1
    assert lib.gxg_work_bytes(64, 128, 16, 0) > 0 and lib.gxg_work_bytes(1, 1, 2, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.pgrad refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(pgrad._n, "load", refuse)


def _data(B=8, D=43, A=2, **over):
    d = dict(obs=torch.zeros(B, D), act=torch.zeros(B, A), adv=torch.zeros(B), logp=torch.zeros(B), adc=torch.zeros(B))
    d.update(over)
    return d


def test_actors_it_does_not_support_in_fishers_words(no_library):
    for kw, A in ((dict(layers=1), 2), (dict(layers=3), 2), (dict(h=128), 2), (dict(h=32), 2), (dict(D=129), 2), (dict(act=torch.nn.ReLU), 2),
                  (dict(h2=32), 2), (dict(out_act=torch.nn.Softplus), 2), (dict(bias=False), 2), (dict(A=3), 3), (dict(A=18), 18)):
        with pytest.raises(NotImplementedError) as theirs:
            fisher.FisherOperator(tfh._Actor(tfh._mods(**kw), A), torch.zeros(8, 43))
        with pytest.raises(NotImplementedError) as mine:
            pgrad.SurrogateGradient(tfh._Actor(tfh._mods(**kw), A), _data())
        assert str(mine.value) == str(theirs.value).replace("FisherOperator", "SurrogateGradient"), kw
        assert "SurrogateGradient" in str(mine.value) and "FisherOperator" not in str(mine.value)
    for pi, words in ((torch.nn.Linear(3, 2), ".mu_net and .log_std"), (tfh._Actor(tfh._mods(), 2, extra=True), "parameters() are log_std, then"),
                      (tfh._Actor(tfh._mods(), 2, n_log_std=4), "log_std has 4 entries")):
        with pytest.raises(NotImplementedError, match=re.escape(words)):
            pgrad.SurrogateGradient(pi, _data())


@pytest.mark.parametrize("over,words", [
    (dict(obs=np.zeros((8, 43), np.float32)), "SurrogateGradient: obs must be a float32 tensor"),
    (dict(obs=torch.zeros(8, 44)), "SurrogateGradient: obs must be (B, 43)"),
    (dict(obs=torch.zeros(8, 50)[:, :43]), "SurrogateGradient: obs must be contiguous"),
    (dict(), "SurrogateGradient: obs lives on cpu; it must be on a cuda device"),
    (dict(obs=torch.zeros(8, 43, dtype=torch.float64)), "SurrogateGradient: obs must be a float32 tensor"),
])
def test_batches_it_does_not_accept(over, words, no_library):
    pi = f64.make_actor(43, 2)
    with pytest.raises(ValueError, match=re.escape(words)):
        pgrad.SurrogateGradient(pi, _data(**over))
    for key in ("obs", "act", "adv", "logp"):
        d = _data()
        del d[key]
        with pytest.raises(ValueError, match=f"SurrogateGradient: data has no '{key}'"):
            pgrad.SurrogateGradient(pi, d)


def test_the_rows_entries_and_the_scalars(no_library):
    dev = torch.device("cuda:0")
    for name, v, shape, words in (("act", torch.zeros(8, 3), (8, 2), "must be (8, 2)"), ("adv", torch.zeros(9), (8,), "must be (8,)"),
                                  ("logp", torch.zeros(8, dtype=torch.float64), (8,), "must be a float32 tensor"),
                                  ("adc", torch.zeros(16)[::2], (8,), "must be contiguous"),
                                  ("adv", torch.zeros(8), (8,), "lives on cpu; it must be on cuda:0, where obs is")):
        with pytest.raises(ValueError, match=re.escape(f"SurrogateGradient: {name} {words}")):
            pgrad._checked(name, v, shape, dev)
    with pytest.raises(ValueError, match=re.escape("cpo_direction: b must be a float32 tensor")):
        pgrad._direction_from(np.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(1), -1.0, 0.01)
    with pytest.raises(ValueError, match=re.escape("cpo_direction: b lives on cpu")):
        pgrad._direction_from(torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(4), torch.zeros(1), -1.0, 0.01)
    for v, words in ((torch.zeros(2), "must be a number or a tensor of one element"), (torch.zeros(()), "lives on cpu")):
        with pytest.raises(ValueError, match=re.escape(f"cpo_direction: c {words}")):
            pgrad._scalar("cpo_direction", "c", v, dev)
    for wg in (-1, 4097, 1.5):
        with pytest.raises(ValueError, match="SurrogateGradient: workgroups must be 0"):
            pgrad.SurrogateGradient(f64.make_actor(43, 2), _data(), workgroups=wg)


def test_the_package_exports_it():
    import guardx_amd
    assert guardx_amd.pgrad is pgrad and guardx_amd.SurrogateGradient is pgrad.SurrogateGradient
    assert guardx_amd.cpo_direction is pgrad.cpo_direction and guardx_amd.trpo_direction is pgrad.trpo_direction
    assert pgrad.DIRECTION == ("lam", "nu", "q", "r", "s", "A", "B") and pgrad.EPS == 1e-8
