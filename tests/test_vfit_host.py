"""libguardx_vfit.so without a GPU (hipcc cross-compiles): what tests/test_linesearch_host.py asks of the eleventh library,
asked of the twelfth -- where it is registered, what its id covers, that its binding, its header and its export list agree,
that a foreign build is refused, that it leaves the other libraries' ids alone -- and every refusal of guardx_amd.vfit and
of the C entry points, none of which may reach a launch (on a machine without a GPU a launch would come back as
GXV_ERR_HIP, not as the status asserted here)."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import side_abi
import vfit64 as v64
from guardx_amd import _vfit_native as n
from guardx_amd import build, vfit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "vfit", "gxv"
LIB = build.FIT_LIBRARIES[KEY]
PROTOS = 9
MINE = ("gx_vfit.hip", "guardx_vfit.h")


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
def test_it_is_registered_in_the_fourth_mapping_only():
    assert list(build.FIT_LIBRARIES) == [KEY]
    assert all(KEY not in m for m in (build.LIBRARIES, build.LEARNER_LIBRARIES, build.UPDATE_LIBRARIES))
    assert LIB not in build.all_libraries() and LIB not in build.every_library()
    assert build.fit_libraries() == build.all_libraries() + [LIB] and len(build.fit_libraries()) == 12
    # the three functions and mappings before it keep their values
    assert list(build.UPDATE_LIBRARIES) == ["linesearch"] and list(build.LEARNER_LIBRARIES) == ["fisher"]
    assert len(build.all_libraries()) == 11 and len(build.every_library()) == 10
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.UPDATE_LIBRARIES["linesearch"])
    text = open(os.path.join(ROOT, "guardx_amd", "build.py")).read()
    assert "waits for a pull request that may touch" in text and "FIT_LIBRARIES" in text and "fit_libraries()" in text


def test_declaration():
    assert LIB.macro == "GXV_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_vfit.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_vfit.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "VFIT_BUILD_ID")
    assert "guardx_amd/lib/VFIT_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_vfit.hip", "gx_device.h", "gx_policy.h", "guardx_vfit.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = build.all_libraries()
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
    before = {lib.key: lib.source_hash() for lib in build.all_libraries()}
    assert len(before) == 11
    shutil.copytree(build.CSRC, tmp_path / "guardx_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    os.remove(tmp_path / "guardx_amd" / "csrc" / MINE[0])
    os.remove(tmp_path / "include" / MINE[1])
    monkeypatch.setattr(build, "CSRC", str(tmp_path / "guardx_amd" / "csrc"))
    assert {lib.key: lib.source_hash() for lib in build.all_libraries()} == before
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
    for lib in build.fit_libraries():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_build_builds_twelve_libraries(defined):
    assert len(defined) == 12 and all(os.path.exists(lib.lib) and not lib.needs_build() for lib in build.fit_libraries())


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxv_build_id().decode() == LIB.source_hash() == LIB.built_id()


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
_HYPER = (C.c_double * 12)(1e-3, 0.9, 0.999, 1e-8, *[b ** t for t in (1, 2, 3, 4) for b in (0.9, 0.999)])
HYPER = C.cast(_HYPER, C.c_void_p)


def _gradient(lib, B=64, D=43, h=64, theta=PTR, obs=PTR, ret=PTR, wg=0, work=PTR, g=PTR, loss=PTR):
    return lib.gxv_gradient(B, D, h, theta, obs, ret, wg, work, g, loss, None)


def _fit(lib, B=64, D=43, h=64, theta=PTR, m=PTR, v=PTR, step0=0, obs=PTR, ret=PTR, iters=4, hyper=HYPER, wg=0, work=PTR, loss=PTR):
    return lib.gxv_fit(B, D, h, theta, m, v, step0, obs, ret, iters, hyper, wg, work, loss, None)


def _adam(lib, P=100, theta=PTR, m=PTR, v=PTR, g=PTR, hyper=HYPER):
    return lib.gxv_adam_step(P, theta, m, v, g, hyper, None)


def test_sizes(defined):
    lib = n.load()
    for D in (43, 64, 1, 128):
        assert lib.gxv_param_count(D, 64) == v64.param_count(D, 64) == vfit.param_count(D) == 64 * D + 64 + 4096 + 64 + 64 + 1
    assert lib.gxv_param_count(43, 8) == v64.param_count(43, 8)
    assert lib.gxv_param_count(0, 64) == lib.gxv_param_count(43, 0) == -1
    rows = (0, -1, 1, 64, 65, 256 * 64, 256 * 64 + 1, 400000, 2 ** 31 - 1)
    assert [lib.gxv_default_workgroups(B) for B in rows] == [0, 0, 1, 1, 2, 256, 256, 256, 256]
    P = v64.param_count(43)
    assert P % 2 == 1                                             # the partial vectors are rounded up to 8 bytes
    assert lib.gxv_work_bytes(65, 43, 0) == (4 * 2 * P + 7) // 8 * 8 + 8 * 2
    assert lib.gxv_work_bytes(65, 43, 5) == (4 * 5 * P + 7) // 8 * 8 + 8 * 5
    assert lib.gxv_work_bytes(400000, 43, 0) == (4 * 256 * P + 7) // 8 * 8 + 8 * 256


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    for kw in [dict([(k, None)]) for k in ("theta", "obs", "ret", "work", "g", "loss")] + \
            [dict(B=0), dict(B=-1), dict(D=0), dict(wg=-1), dict(wg=4097)]:
        assert _gradient(lib, **kw) == n.GXV_ERR_ARG, kw
        assert b"gxv_gradient" in lib.gxv_last_error()
    for kw in [dict([(k, None)]) for k in ("theta", "m", "v", "obs", "ret", "hyper", "work", "loss")] + \
            [dict(iters=-1), dict(step0=-1), dict(B=0), dict(D=0), dict(wg=-1), dict(wg=4097)]:
        assert _fit(lib, **kw) == n.GXV_ERR_ARG, kw
        assert b"gxv_fit" in lib.gxv_last_error()
    for kw in [dict([(k, None)]) for k in ("theta", "m", "v", "g", "hyper")] + [dict(P=0), dict(P=-1)]:
        assert _adam(lib, **kw) == n.GXV_ERR_ARG, kw
        assert b"gxv_adam_step" in lib.gxv_last_error()
    assert lib.gxv_tanh_act(4, None, PTR, None) == lib.gxv_tanh_act(4, PTR, None, None) == lib.gxv_tanh_act(-1, PTR, PTR, None) == n.GXV_ERR_ARG
    assert lib.gxv_tanh_act(0, PTR, PTR, None) == n.GXV_OK            # nothing to do, nothing launched
    assert _fit(lib, iters=0) == n.GXV_OK                             # legal, and launches nothing
    with pytest.raises(n.GxvError, match="guardx vfit status 1: gxv_fit: null pointer") as e:
        n.check(_fit(lib, obs=None))
    assert e.value.status == n.GXV_ERR_ARG
    for args in ((0, 43, 0), (64, 0, 0), (64, 43, -1), (64, 43, 4097)):
        assert lib.gxv_work_bytes(*args) == -1, args


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "observation width")):
        assert _gradient(lib, **kw) == n.GXV_ERR_UNSUPPORTED, kw
        assert word in lib.gxv_last_error().decode()
        assert _fit(lib, **kw) == n.GXV_ERR_UNSUPPORTED, kw
    assert lib.gxv_work_bytes(64, 129, 0) == -1
    assert lib.gxv_work_bytes(64, 128, 0) > 0 and lib.gxv_work_bytes(1, 1, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.vfit refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(vfit._n, "load", refuse)


class _Critic(torch.nn.Module):
    def __init__(self, mods, extra=False, name="v_net"):
        super().__init__()
        setattr(self, name, torch.nn.Sequential(*mods))
        if extra:                                   # parameters() is then no longer the flat vector
            self.more = torch.nn.Linear(1, 1)


def test_critics_it_does_not_support_in_fishers_words(no_library):
    """the same module lists under .mu_net give FisherOperator the same words (the ones both state: the shape of the net)"""
    import test_fisher_host as tfh
    from guardx_amd import fisher
    same = [dict(layers=1), dict(layers=3), dict(h=128), dict(h=32), dict(D=129), dict(act=torch.nn.ReLU), dict(h2=32),
            dict(out_act=torch.nn.Softplus), dict(bias=False)]
    for kw in same:
        with pytest.raises(NotImplementedError) as theirs:
            fisher.FisherOperator(tfh._Actor(tfh._mods(A=2, **kw), 2), torch.zeros(8, 43))
        with pytest.raises(NotImplementedError) as mine:
            vfit.ValueFit(_Critic(tfh._mods(A=1, **kw)), lr=1e-3)
        assert str(mine.value) == str(theirs.value).replace("FisherOperator", "ValueFit") and "ValueFit" in str(mine.value), kw
    for critic, words in ((torch.nn.Linear(3, 1), "a critic with .v_net"), (_Critic(tfh._mods(A=1), name="q_net"), "a critic with .v_net"),
                          (_Critic(tfh._mods(A=2)), "one output, not 2"), (_Critic(tfh._mods(A=1), extra=True), "whose parameters() are")):
        with pytest.raises(NotImplementedError, match=re.escape(words)):
            vfit.ValueFit(critic, lr=1e-3)
    # the reference's two critics: MLPCritic is served, SCPO's MLPMaxCostCritic (a softplus output) is not
    assert vfit.ValueFit(v64.make_critic(43), lr=1e-3).D == 43
    with pytest.raises(NotImplementedError, match="a linear output only"):
        vfit.ValueFit(v64.make_critic(43, out_act=torch.nn.Softplus), lr=1e-3)


def test_optimizers_it_does_not_support(no_library):
    critic = v64.make_critic(43)
    for kw in (dict(weight_decay=1e-2), dict(amsgrad=True)):
        with pytest.raises(NotImplementedError, match="without weight_decay and amsgrad"):
            vfit.ValueFit(critic, lr=1e-3, **kw)
    for kw in (dict(lr=-1.0), dict(lr=1e-3, betas=(1.0, 0.999)), dict(lr=1e-3, eps=-1e-8)):
        with pytest.raises(ValueError, match="ValueFit: lr and eps"):
            vfit.ValueFit(critic, **kw)
    for wg in (-1, 4097, 1.5):
        with pytest.raises(ValueError, match="workgroups must be 0"):
            vfit.ValueFit(critic, lr=1e-3, workgroups=wg)
    VF = vfit.ValueFit(critic, lr=3e-4, betas=(0.8, 0.99), eps=1e-6, workgroups=7)
    assert (VF.lr, VF.betas, VF.eps, VF.workgroups, VF.step, VF.P) == (3e-4, (0.8, 0.99), 1e-6, 7, 0, v64.param_count(43))


@pytest.mark.parametrize("obs,ret,words", [
    (np.zeros((8, 43), np.float32), torch.zeros(8), "ValueFit: obs must be a float32 tensor"),
    (torch.zeros(8, 44), torch.zeros(8), "ValueFit: obs must be (B, 43)"),
    (torch.zeros(8, 50)[:, :43], torch.zeros(8), "ValueFit: obs must be contiguous"),
    (torch.zeros(8, 43), torch.zeros(8), "ValueFit: obs lives on cpu; it must be on a cuda device"),
    (torch.zeros(8, 43, dtype=torch.float64), torch.zeros(8), "ValueFit: obs must be a float32 tensor"),
])
def test_batches_it_does_not_accept(obs, ret, words, no_library):
    VF = vfit.ValueFit(v64.make_critic(43), lr=1e-3)
    for call in (lambda: VF.fit(obs, ret), lambda: VF.gradient(obs, ret), lambda: VF.fit(obs, ret, iters=0)):
        with pytest.raises(ValueError, match=re.escape(words)):
            call()
    assert VF.step == 0 and VF.m is None


def test_ret_and_iters(no_library):
    dev = torch.device("cuda:0")
    for v, words in ((torch.zeros(9), "must be (8,)"), (torch.zeros(8, 1), "must be (8,)"),
                     (torch.zeros(8, dtype=torch.float64), "must be a float32 tensor"), (torch.zeros(16)[::2], "must be contiguous"),
                     (torch.zeros(8), "lives on cpu; it must be on cuda:0, where obs is")):
        with pytest.raises(ValueError, match=re.escape(f"ValueFit: ret {words}")):
            vfit._checked("ret", v, (8,), dev)
    VF = vfit.ValueFit(v64.make_critic(43), lr=1e-3)
    for iters in (-1, 1.5):
        with pytest.raises(ValueError, match="iters must be a non-negative integer"):      # before the batch is looked at
            VF.fit(torch.zeros(8, 43), torch.zeros(8), iters=iters)


def test_the_bias_corrections_are_python_floats_step_by_step():
    got = vfit.bias_corrections((0.9, 0.999), 5, 3)
    assert got == [0.9 ** 6, 0.999 ** 6, 0.9 ** 7, 0.999 ** 7, 0.9 ** 8, 0.999 ** 8] and all(type(x) is float for x in got)
    assert vfit.bias_corrections((0.9, 0.999), 0, 0) == []
    # what adam64 raises itself
    assert [1.0 - x for x in got[:2]] == [1.0 - 0.9 ** 6, 1.0 - 0.999 ** 6]


def test_the_package_exports_it():
    import guardx_amd
    assert guardx_amd.vfit is vfit and guardx_amd.ValueFit is vfit.ValueFit
