"""libguardx_fisher.so without a GPU (hipcc cross-compiles): what tests/test_build_identity.py asks of the nine libraries,
asked of the tenth -- where it is registered, what its id covers, that its binding, its header and its export list agree,
that a foreign build is refused -- and every refusal of guardx_amd.fisher and of the C entry points, none of which may
reach a launch (on a machine without a GPU a launch would come back as GXF_ERR_HIP, not as the status asserted here)."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import fisher64 as f64
import side_abi
from guardx_amd import _fisher_native as n
from guardx_amd import build, fisher

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "fisher", "gxf"
LIB = build.LEARNER_LIBRARIES[KEY]
PROTOS = 8


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
def test_it_is_a_learner_library_built_after_the_nine():
    assert list(build.LEARNER_LIBRARIES) == [KEY] and KEY not in build.LIBRARIES and len(build.LIBRARIES) == 8
    assert build.every_library() == [build.MAIN] + list(build.LIBRARIES.values()) + [LIB]
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.LIBRARIES["epstats"])
    assert "waits for a pull request that may touch" in open(os.path.join(ROOT, "guardx_amd", "build.py")).read()


def test_declaration():
    assert LIB.macro == "GXF_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_fisher.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_fisher.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "FISHER_BUILD_ID")
    assert "guardx_amd/lib/FISHER_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_fisher.hip", "gx_device.h", "gx_policy.h", "guardx_fisher.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = [build.MAIN] + list(build.LIBRARIES.values())
    assert LIB.source_hash() not in {o.source_hash() for o in others}
    for o in others:                                              # its source and public header are its own
        assert not {"gx_fisher.hip", "guardx_fisher.h"} & {os.path.basename(x) for x in o.sources + o.headers}


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


def test_the_binding_matches_the_header():
    side_abi.assert_binding_matches_the_header(KEY, PREFIX, n, None, PROTOS, 4)
    assert n._side.symbols == n.SYMBOLS and len(_declared()) == PROTOS
    assert not re.search(r"\bdouble\b", side_abi.header(KEY))      # eps and damping travel as float


@pytest.fixture(scope="module")
def defined():
    """{key: {symbol: type}} of what each built library defines (nm -D)"""
    build.build()
    out = {}
    for lib in build.every_library():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxf_build_id().decode() == LIB.source_hash() == LIB.built_id()


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


def _fvp(lib, B=64, D=43, A=2, h=64, obs=PTR, theta=PTR, x=PTR, wg=0, work=PTR, y=2 * PTR):
    return lib.gxf_fvp(B, D, A, h, obs, theta, x, 1e-8, 0.0, wg, work, y, None)


def _cg(lib, B=64, D=43, A=2, h=64, obs=PTR, theta=PTR, g=PTR, iters=10, wg=0, work=PTR, xh=PTR, s=PTR, rd=PTR, it=PTR):
    return lib.gxf_cg(B, D, A, h, obs, theta, g, 1e-8, 0.0, iters, wg, work, xh, s, rd, it, None)


def test_sizes(defined):
    lib = n.load()
    for D, A in ((43, 2), (64, 8), (1, 2), (128, 16)):
        assert lib.gxf_param_count(D, A, 64) == f64.param_count(D, A, 64) == fisher.param_count(D, A)
    assert lib.gxf_param_count(43, 2, 8) == f64.param_count(43, 2, 8)
    assert lib.gxf_param_count(0, 2, 64) == lib.gxf_param_count(43, 0, 64) == lib.gxf_param_count(43, 2, 0) == -1
    assert [lib.gxf_default_workgroups(B) for B in (0, 1, 64, 65, 256 * 64, 256 * 64 + 1, 400000)] == [0, 1, 1, 2, 256, 256, 256]
    P = f64.param_count(43, 2, 64)
    state = 16
    assert lib.gxf_work_bytes(65, 43, 2, 0) == 4 * (2 * P + 3 * P) + state
    assert lib.gxf_work_bytes(65, 43, 2, 5) == 4 * (5 * P + 3 * P) + state
    assert lib.gxf_work_bytes(400000, 43, 2, 0) == 4 * (256 * P + 3 * P) + state
    assert lib.gxf_work_bytes(65, 43, 2, 0) % 8 == 0


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    for kw in (dict(obs=None), dict(theta=None), dict(x=None), dict(work=None), dict(y=None), dict(y=PTR),
               dict(B=0), dict(B=-1), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097)):
        assert _fvp(lib, **kw) == n.GXF_ERR_ARG, kw
        assert lib.gxf_last_error()
    for kw in (dict(obs=None), dict(theta=None), dict(g=None), dict(work=None), dict(xh=None), dict(s=None), dict(rd=None),
               dict(it=None), dict(iters=-1), dict(B=0), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097)):
        assert _cg(lib, **kw) == n.GXF_ERR_ARG, kw
    for args in ((-1, PTR, 2 * PTR), (4, None, 2 * PTR), (4, PTR, None)):
        assert lib.gxf_tanh_act(*args, None) == n.GXF_ERR_ARG, args
        assert b"gxf_tanh_act" in lib.gxf_last_error()
    with pytest.raises(n.GxfError, match="guardx fisher status 1: gxf_fvp: null pointer") as e:
        n.check(_fvp(lib, obs=None))
    assert e.value.status == n.GXF_ERR_ARG
    for args in ((0, 43, 2, 0), (64, 0, 2, 0), (64, 43, 0, 0), (64, 43, 2, -1), (64, 43, 2, 4097)):
        assert lib.gxf_work_bytes(*args) == -1, args


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "observation width"),
                     (dict(A=3), "even action width"), (dict(A=18), "even action width"), (dict(A=1), "even action width")):
        assert _fvp(lib, **kw) == n.GXF_ERR_UNSUPPORTED, kw
        assert word in lib.gxf_last_error().decode()
        assert _cg(lib, **kw) == n.GXF_ERR_UNSUPPORTED, kw
    assert lib.gxf_work_bytes(64, 129, 2, 0) == lib.gxf_work_bytes(64, 43, 3, 0) == lib.gxf_work_bytes(64, 43, 18, 0) == -1
    assert lib.gxf_work_bytes(64, 128, 16, 0) > 0 and lib.gxf_work_bytes(1, 1, 2, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.fisher refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
class _Actor(torch.nn.Module):
    def __init__(self, mods, A, extra=False, n_log_std=None):
        super().__init__()
        self.log_std = torch.nn.Parameter(torch.zeros(A if n_log_std is None else n_log_std))
        self.mu_net = torch.nn.Sequential(*mods)
        if extra:                                   # parameters() is then no longer the learners' flat vector
            self.more = torch.nn.Linear(1, 1)


def _mods(D=43, h=64, A=2, act=torch.nn.Tanh, h2=None, layers=2, out_act=torch.nn.Identity, bias=True):
    L = torch.nn.Linear
    h2 = h if h2 is None else h2
    mods = [L(D, h, bias=bias), act()]
    for _ in range(layers - 1):
        mods += [L(h, h2), act()]
    return mods + [L(h2, A), out_act()]


@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(fisher._n, "load", refuse)


@pytest.mark.parametrize("make,words", [
    (lambda: _Actor(_mods(layers=1), 2), "two hidden layers"),
    (lambda: _Actor(_mods(layers=3), 2), "two hidden layers"),
    (lambda: _Actor(_mods(act=torch.nn.ReLU), 2), "Tanh hidden activations"),
    (lambda: _Actor(_mods(out_act=torch.nn.Tanh), 2), "Tanh hidden activations"),
    (lambda: _Actor(_mods(h2=32), 2), "two hidden layers of equal width"),
    (lambda: _Actor(_mods(h=100), 2), "hidden widths"),
    (lambda: _Actor(_mods(h=128), 2), "hidden width 64"),
    (lambda: _Actor(_mods(D=129), 2), "observation width <= 128"),
    (lambda: _Actor(_mods(A=3), 3), "even action width <= 16"),
    (lambda: _Actor(_mods(A=18), 18), "even action width <= 16"),
    (lambda: _Actor(_mods(), 2, n_log_std=4), "log_std has 4 entries"),
    (lambda: _Actor(_mods(), 2, extra=True), "parameters() are log_std, then"),
    (lambda: _Actor(_mods(bias=False), 2), "with a bias"),
    (lambda: torch.nn.Linear(3, 2), ".mu_net and .log_std"),
])
def test_actors_it_does_not_support(make, words, no_library):
    with pytest.raises(NotImplementedError, match=re.escape(words)):
        fisher.FisherOperator(make(), torch.zeros(8, 43))


def test_the_refusals_speak_two_tanh_layers_words(no_library):
    from guardx_amd import _closed_loop
    for mods in (_mods(layers=1), _mods(act=torch.nn.ReLU), _mods(h2=32), _mods(h=100)):
        with pytest.raises(NotImplementedError) as mine:
            fisher.FisherOperator(_Actor(mods, 2), torch.zeros(8, 43))
        with pytest.raises(NotImplementedError) as theirs:
            _closed_loop.two_tanh_layers([m for m in mods if not isinstance(m, torch.nn.Identity)], "FisherOperator", tanh_tail=(
                " and a linear output only (activation=nn.Tanh, output_activation=nn.Identity)"))
        assert str(mine.value) == str(theirs.value)


@pytest.mark.parametrize("obs,words", [
    (np.zeros((8, 43), np.float32), "obs must be a float32 tensor"),
    (torch.zeros(8, 43, dtype=torch.float64), "obs must be a float32 tensor"),
    (torch.zeros(8, 44), "obs must be (B, 43)"),
    (torch.zeros(8 * 43), "obs must be (B, 43)"),
    (torch.zeros(8, 50)[:, :43], "obs must be contiguous"),
    (torch.zeros(43, 8).t(), "obs must be contiguous"),
    (torch.zeros(8, 43), "obs lives on cpu; it must be on a cuda device"),
])
def test_obs_it_does_not_accept(obs, words, no_library):
    with pytest.raises(ValueError, match=re.escape(words)):
        fisher.FisherOperator(_Actor(_mods(), 2), obs)


def test_vectors_it_does_not_accept(no_library):
    P, dev = fisher.param_count(43, 2), torch.device("cuda:0")
    for name in ("x", "g"):
        for v, words in ((np.zeros(P, np.float64), "must be a float32 tensor"), (torch.zeros(P, dtype=torch.float64), "must be a float32 tensor"),
                         (torch.zeros(P + 1), f"must be ({P},)"), (torch.zeros(P, 1), f"must be ({P},)"),
                         (torch.zeros(2 * P)[::2], "must be contiguous"), (torch.zeros(P), "lives on cpu; it must be on cuda:0, where obs is")):
            with pytest.raises(ValueError, match=re.escape(f"FisherOperator: {name} {words}")):
                fisher._checked(name, v, (P,), dev)
    # the operator's own entry points go through the same check, before anything else
    F = object.__new__(fisher.FisherOperator)
    F.P, F.device = P, dev
    with pytest.raises(ValueError, match="x must be a float32 tensor"):
        F(torch.zeros(P, dtype=torch.float64))
    with pytest.raises(ValueError, match=re.escape(f"x must be ({P},)")):
        F(np.zeros(P + 1, np.float32))
    with pytest.raises(ValueError, match="g lives on cpu"):
        F.solve(torch.zeros(P))


def test_the_package_exports_it():
    import guardx_amd
    assert guardx_amd.fisher is fisher and guardx_amd.FisherOperator is fisher.FisherOperator
    pi = f64.make_actor(43, 2)
    flat = fisher.flat_params(pi)
    assert flat.dtype == torch.float32 and tuple(flat.shape) == (fisher.param_count(43, 2),)
    assert torch.equal(flat, torch.cat([p.flatten() for p in pi.parameters()]).detach())
