"""libguardx_pifit.so without a GPU (hipcc cross-compiles): what tests/test_pgrad_host.py asks of the thirteenth library, asked
of the fourteenth -- where it is registered, what its id covers, that its binding, its header and its export list agree, that a
foreign build is refused, that it leaves the other libraries' ids alone -- the table of bias corrections, and every refusal of
guardx_amd.pifit and of the C entry points, none of which may reach a launch (on a machine without a GPU a launch would come
back as GXA_ERR_HIP, not as the status asserted here)."""
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
import test_fisher_host as tfh
from guardx_amd import _pifit_native as n
from guardx_amd import build, fisher, pifit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "pifit", "gxa"
LIB = build.ACTOR_LIBRARIES[KEY]
PROTOS = 8
MINE = ("gx_pifit.hip", "guardx_pifit.h")


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
def test_it_is_registered_in_the_sixth_mapping_only():
    assert list(build.ACTOR_LIBRARIES) == [KEY]
    assert all(KEY not in m for m in (build.LIBRARIES, build.LEARNER_LIBRARIES, build.UPDATE_LIBRARIES, build.FIT_LIBRARIES,
                                      build.GRAD_LIBRARIES))
    assert LIB not in build.grad_libraries()
    assert build.actor_libraries() == build.grad_libraries() + [LIB] and len(build.actor_libraries()) == 14
    # the five functions and mappings before it keep their values
    assert list(build.GRAD_LIBRARIES) == ["pgrad"] and list(build.FIT_LIBRARIES) == ["vfit"]
    assert list(build.UPDATE_LIBRARIES) == ["linesearch"] and list(build.LEARNER_LIBRARIES) == ["fisher"]
    assert [len(f()) for f in (build.grad_libraries, build.fit_libraries, build.all_libraries, build.every_library)] == [13, 12, 11, 10]
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.GRAD_LIBRARIES["pgrad"])
    text = open(os.path.join(ROOT, "guardx_amd", "build.py")).read()
    assert "ACTOR_LIBRARIES" in text and "actor_libraries()" in text
    assert "actor_libraries()" in open(os.path.join(ROOT, "guardx_amd", "_sidelib.py")).read()


def test_declaration():
    assert LIB.macro == "GXA_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_pifit.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_pifit.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "PIFIT_BUILD_ID")
    assert "guardx_amd/lib/PIFIT_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_pifit.hip", "gx_device.h", "gx_policy.h", "guardx_pifit.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = build.grad_libraries()
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


def test_the_thirteen_libraries_before_it_keep_their_source_hashes_without_the_new_files(monkeypatch, tmp_path):
    """a copy of csrc and include without the two new files gives every other library the id it has in the tree: nothing
    an existing library hashes was touched, none of them reaches the new files, and so none shares a translation unit with
    the new library"""
    before = {lib.key: lib.source_hash() for lib in build.grad_libraries()}
    assert len(before) == 13
    shutil.copytree(build.CSRC, tmp_path / "guardx_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    os.remove(tmp_path / "guardx_amd" / "csrc" / MINE[0])
    os.remove(tmp_path / "include" / MINE[1])
    monkeypatch.setattr(build, "CSRC", str(tmp_path / "guardx_amd" / "csrc"))
    assert {lib.key: lib.source_hash() for lib in build.grad_libraries()} == before
    with pytest.raises(OSError):
        LIB.source_hash()


def test_the_binding_matches_the_header():
    side_abi.assert_binding_matches_the_header(KEY, PREFIX, n, None, PROTOS, 4)
    assert n._side.symbols == n.SYMBOLS and len(_declared()) == PROTOS
    assert not re.search(r"\bdouble\b", side_abi.header(KEY))      # float64 data travels behind void*
    assert set(n.SYMBOLS) == {"gxa_fit", "gxa_gradient", "gxa_work_bytes", "gxa_param_count", "gxa_default_workgroups",
                              "gxa_tanh_act", "gxa_build_id", "gxa_last_error"}


@pytest.fixture(scope="module")
def defined():
    """{key: {symbol: type}} of what each built library defines (nm -D)"""
    build.build()
    out = {}
    for lib in build.actor_libraries():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_build_builds_fourteen_libraries(defined):
    assert len(defined) == 14 and all(os.path.exists(lib.lib) and not lib.needs_build() for lib in build.actor_libraries())


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxa_build_id().decode() == LIB.source_hash() == LIB.built_id()


def test_a_foreign_build_id_is_refused(defined, monkeypatch):
    monkeypatch.setattr(n._side, "_lib", None)
    monkeypatch.setattr(LIB, "source_hash", lambda: "0" * 24)
    monkeypatch.setattr(LIB, "needs_build", lambda: False)
    with pytest.raises(ImportError, match="built from other sources"):
        n.load()


# ---------------------------------------------------------------------------------------------------------------------
# the table of bias corrections
# ---------------------------------------------------------------------------------------------------------------------
def test_the_table_is_b_to_the_t_bit_for_bit_and_t_sat_is_where_it_says():
    b1, b2 = 0.9, 0.999
    table, t_sat = pifit.bias_table((b1, b2))
    assert len(table) == 2 * t_sat and 37000 < t_sat < 38000
    for t in list(range(1, 200)) + [1000, 5000, 20000, t_sat - 1, t_sat]:
        assert table[2 * (t - 1)].hex() == (b1 ** t).hex() and table[2 * (t - 1) + 1].hex() == (b2 ** t).hex(), t
    assert all(table[2 * (t - 1)] == b1 ** t and table[2 * (t - 1) + 1] == b2 ** t for t in range(1, t_sat + 1))
    sat = lambda t: 1.0 - b1 ** t == 1.0 and 1.0 - b2 ** t == 1.0     # noqa: E731
    assert sat(t_sat) and not sat(t_sat - 1) and not any(sat(t) for t in range(1, t_sat))
    assert all(sat(t) for t in (t_sat + 1, 2 * t_sat, 10 ** 6))     # past it both corrections are exactly 1: the last entry serves
    # the corrections the kernel forms from an entry are vfit's: lr / (1 - b1^t) and sqrt(1 - b2^t)
    assert pifit.bias_table((0.0, 0.0)) == ([0.0, 0.0], 1)
    assert pifit.bias_table((0.5, 0.0))[1] == 54 and pifit.bias_table((0.0, 0.5))[1] == 54       # 0.5 ** 54 is half an ulp of 1
    PF = pifit.PolicyFit(f64.make_actor(43, 2), lr=3e-4)
    assert PF.t_sat == t_sat and PF.table == table


def test_betas_whose_table_would_pass_two_to_the_twenty_are_refused():
    for betas in ((0.9, 0.99999), (0.99999, 0.999), (0.9, 1.0 - 2.0 ** -40)):
        with pytest.raises(NotImplementedError, match=re.escape("reach 1 within 2^20 steps")):
            pifit.PolicyFit(f64.make_actor(43, 2), lr=3e-4, betas=betas)
    slow = 1.0 - 37.0 / 2 ** 20                                   # the slowest kind that still fits
    assert pifit.bias_table((0.9, 0.9999))[1] < pifit.TABLE_LIMIT == 2 ** 20
    assert 1.0 - slow ** (2 ** 20) != 1.0
    with pytest.raises(NotImplementedError):
        pifit.bias_table((0.9, slow))


# ---------------------------------------------------------------------------------------------------------------------
# the C entry points refuse before they launch
# ---------------------------------------------------------------------------------------------------------------------
PTR = 4096      # a non-null address that nothing may dereference on these paths


def _host(*values):
    arr = (C.c_double * len(values))(*values)
    return arr, C.cast(arr, C.c_void_p)


NAN = float("nan")


def _gradient(lib, B=64, D=43, A=2, h=64, theta=PTR, obs=PTR, act=PTR, adv=PTR, logp=PTR, loss=0, clip=0.2, hyper=True, wg=0, work=PTR,
              g=PTR, info=PTR):
    keep, ptr = _host(clip)
    return lib.gxa_gradient(B, D, A, h, theta, obs, act, adv, logp, loss, ptr if hyper else None, wg, work, g, info, None)


def _fit(lib, B=64, D=43, A=2, h=64, theta=PTR, m=PTR, v=PTR, count=PTR, obs=PTR, act=PTR, adv=PTR, logp=PTR, iters=3, loss=0,
         clip=0.2, target=0.01, hyper=True, table=PTR, t_sat=100, wg=0, work=PTR, trace=PTR, ctl=PTR, last=PTR):
    keep, ptr = _host(3e-4, 0.9, 0.999, 1e-8, target, clip)
    return lib.gxa_fit(B, D, A, h, theta, m, v, count, obs, act, adv, logp, iters, loss, ptr if hyper else None, table, t_sat, wg,
                       work, trace, ctl, last, None)


def test_sizes(defined):
    lib = n.load()
    for D, A in ((43, 2), (64, 8), (1, 16), (128, 2)):
        assert lib.gxa_param_count(D, A, 64) == f64.param_count(D, A, 64) == fisher.param_count(D, A)
    assert lib.gxa_param_count(43, 2, 8) == f64.param_count(43, 2, 8)
    assert lib.gxa_param_count(0, 2, 64) == lib.gxa_param_count(43, 0, 64) == lib.gxa_param_count(43, 2, 0) == -1
    rows = (0, -1, 1, 64, 65, 256 * 64, 256 * 64 + 1, 400000, 2 ** 31 - 1)
    assert [lib.gxa_default_workgroups(B) for B in rows] == [0, 0, 1, 1, 2, 256, 256, 256, 256]
    P = f64.param_count(43, 2, 64)
    # one partial vector of P float32 and 20 float64 per workgroup
    assert lib.gxa_work_bytes(65, 43, 2, 0) == 4 * 2 * P + 8 * 20 * 2
    assert lib.gxa_work_bytes(65, 43, 2, 5) == (4 * 5 * P + 7) // 8 * 8 + 8 * 20 * 5
    assert lib.gxa_work_bytes(400000, 43, 2, 0) == 4 * 256 * P + 8 * 20 * 256


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    for kw in [dict([(k, None)]) for k in ("theta", "obs", "act", "adv", "logp", "work", "g", "info")] + \
            [dict(hyper=False), dict(B=0), dict(B=-1), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097), dict(loss=2), dict(loss=-1),
             dict(loss=1), dict(clip=-0.1)]:
        assert _gradient(lib, **kw) == n.GXA_ERR_ARG, kw
        assert b"gxa_gradient" in lib.gxa_last_error()
    for kw in [dict([(k, None)]) for k in ("theta", "m", "v", "count", "obs", "act", "adv", "logp", "table", "work", "trace", "ctl", "last")] + \
            [dict(hyper=False), dict(B=0), dict(D=0), dict(A=-2), dict(wg=-1), dict(wg=4097), dict(iters=-1), dict(t_sat=0), dict(loss=2),
             dict(loss=1), dict(clip=-1.0)]:
        assert _fit(lib, **kw) == n.GXA_ERR_ARG, kw
        assert b"gxa_fit" in lib.gxa_last_error()
    with pytest.raises(n.GxaError, match="guardx pifit status 1: gxa_gradient: null pointer") as e:
        n.check(_gradient(lib, obs=None))
    assert e.value.status == n.GXA_ERR_ARG
    assert lib.gxa_tanh_act(-1, PTR, PTR, None) == lib.gxa_tanh_act(4, None, PTR, None) == n.GXA_ERR_ARG
    assert lib.gxa_tanh_act(0, PTR, PTR, None) == n.GXA_OK
    for args in ((0, 43, 2, 0), (64, 0, 2, 0), (64, 43, 0, 0), (64, 43, 2, -1), (64, 43, 2, 4097)):
        assert lib.gxa_work_bytes(*args) == -1, args
    # zero iterations launch nothing, whatever the loss
    assert _fit(lib, iters=0) == _fit(lib, iters=0, clip=NAN) == _fit(lib, iters=0, loss=1, clip=NAN, target=NAN) == n.GXA_OK


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "observation width"),
                     (dict(A=3), "even action width"), (dict(A=18), "even action width")):
        assert _gradient(lib, **kw) == n.GXA_ERR_UNSUPPORTED, kw
        assert word in lib.gxa_last_error().decode()
        assert _fit(lib, **kw) == n.GXA_ERR_UNSUPPORTED, kw
        assert word in lib.gxa_last_error().decode()
    assert lib.gxa_work_bytes(64, 129, 2, 0) == lib.gxa_work_bytes(64, 43, 3, 0) == lib.gxa_work_bytes(64, 43, 18, 0) == -1
    assert lib.gxa_work_bytes(64, 128, 16, 0) > 0 and lib.gxa_work_bytes(1, 1, 2, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.pifit refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(pifit._n, "load", refuse)


def _data(B=8, D=43, A=2, **over):
    d = dict(obs=torch.zeros(B, D), act=torch.zeros(B, A), adv=torch.zeros(B), logp=torch.zeros(B))
    d.update(over)
    return d


def test_actors_it_does_not_support_in_fishers_words(no_library):
    for kw, A in ((dict(layers=1), 2), (dict(layers=3), 2), (dict(h=128), 2), (dict(h=32), 2), (dict(D=129), 2), (dict(act=torch.nn.ReLU), 2),
                  (dict(h2=32), 2), (dict(out_act=torch.nn.Softplus), 2), (dict(bias=False), 2), (dict(A=3), 3), (dict(A=18), 18)):
        with pytest.raises(NotImplementedError) as theirs:
            fisher.FisherOperator(tfh._Actor(tfh._mods(**kw), A), torch.zeros(8, 43))
        with pytest.raises(NotImplementedError) as mine:
            pifit.PolicyFit(tfh._Actor(tfh._mods(**kw), A), lr=3e-4)
        assert str(mine.value) == str(theirs.value).replace("FisherOperator", "PolicyFit"), kw
        assert "PolicyFit" in str(mine.value) and "FisherOperator" not in str(mine.value)
    for pi, words in ((torch.nn.Linear(3, 2), ".mu_net and .log_std"), (tfh._Actor(tfh._mods(), 2, extra=True), "parameters() are log_std, then"),
                      (tfh._Actor(tfh._mods(), 2, n_log_std=4), "log_std has 4 entries")):
        with pytest.raises(NotImplementedError, match=re.escape(words)):
            pifit.PolicyFit(pi, lr=3e-4)


def test_optimizers_it_does_not_support(no_library):
    pi = f64.make_actor(43, 2)
    for kw in (dict(weight_decay=1e-4), dict(amsgrad=True)):
        with pytest.raises(NotImplementedError, match="PolicyFit supports Adam without weight_decay and amsgrad"):
            pifit.PolicyFit(pi, lr=3e-4, **kw)
    for kw in (dict(lr=-1.0), dict(lr=3e-4, eps=-1e-8), dict(lr=3e-4, betas=(1.0, 0.999)), dict(lr=3e-4, betas=(0.9, -0.1))):
        with pytest.raises(ValueError, match="PolicyFit: lr and eps must not be negative"):
            pifit.PolicyFit(pi, **kw)
    for wg in (-1, 4097, 1.5):
        with pytest.raises(ValueError, match="PolicyFit: workgroups must be 0"):
            pifit.PolicyFit(pi, lr=3e-4, workgroups=wg)


@pytest.mark.parametrize("over,words", [
    (dict(obs=np.zeros((8, 43), np.float32)), "PolicyFit: obs must be a float32 tensor"),
    (dict(obs=torch.zeros(8, 44)), "PolicyFit: obs must be (B, 43)"),
    (dict(obs=torch.zeros(8, 50)[:, :43]), "PolicyFit: obs must be contiguous"),
    (dict(), "PolicyFit: obs lives on cpu; it must be on a cuda device"),
    (dict(obs=torch.zeros(8, 43, dtype=torch.float64)), "PolicyFit: obs must be a float32 tensor"),
])
def test_batches_it_does_not_accept(over, words, no_library):
    PF = pifit.PolicyFit(f64.make_actor(43, 2), lr=3e-4)
    for call in (PF.fit, PF.gradient):
        with pytest.raises(ValueError, match=re.escape(words)):
            call(_data(**over))
        for key in ("obs", "act", "adv", "logp"):
            d = _data()
            del d[key]
            with pytest.raises(ValueError, match=f"PolicyFit: data has no '{key}'"):
                call(d)


def test_the_rows_entries_and_the_fit_arguments(no_library):
    dev = torch.device("cuda:0")
    for name, v, shape, words in (("act", torch.zeros(8, 3), (8, 2), "must be (8, 2)"), ("adv", torch.zeros(9), (8,), "must be (8,)"),
                                  ("logp", torch.zeros(8, dtype=torch.float64), (8,), "must be a float32 tensor"),
                                  ("adv", torch.zeros(16)[::2], (8,), "must be contiguous"),
                                  ("adv", torch.zeros(8), (8,), "lives on cpu; it must be on cuda:0, where obs is")):
        with pytest.raises(ValueError, match=re.escape(f"PolicyFit: {name} {words}")):
            pifit._checked(name, v, shape, dev)
    PF = pifit.PolicyFit(f64.make_actor(43, 2), lr=3e-4)
    for kw, words in ((dict(iters=-1), "iters must be a non-negative integer"), (dict(iters=1.5), "iters must be a non-negative integer"),
                      (dict(loss="clip"), "loss must be 'ratio' or 'logp'"), (dict(loss="logp"), "loss='logp' takes clip_ratio=None"),
                      (dict(clip_ratio=-0.2), "clip_ratio must be None or a number that is not negative"),
                      (dict(target_kl=float("nan")), "target_kl must be None or a Python number"),
                      (dict(target_kl=torch.zeros(())), "target_kl must be None or a Python number")):
        with pytest.raises(ValueError, match=re.escape(f"PolicyFit.fit: {words}")):
            PF.fit(_data(), **kw)
    with pytest.raises(ValueError, match=re.escape("PolicyFit.gradient: loss='logp' takes clip_ratio=None")):
        PF.gradient(_data(), loss="logp")


def test_the_package_exports_it():
    import guardx_amd
    assert guardx_amd.pifit is pifit and guardx_amd.PolicyFit is pifit.PolicyFit
    assert pifit.LOSSES == ("ratio", "logp") and pifit.TABLE_LIMIT == 2 ** 20
