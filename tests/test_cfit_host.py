"""libguardx_cfit.so without a GPU (hipcc cross-compiles): what tests/test_pifit_host.py asks of the fourteenth library, asked
of the fifteenth -- where it is registered, what its id covers, that its binding, its header and its export list agree, that a
foreign build is refused, that it leaves the other libraries' ids alone -- and every refusal of guardx_amd.cfit and of the C
entry points, none of which may reach a launch (on a machine without a GPU a launch would come back as GXQ_ERR_HIP, not as
the status asserted here)."""
import ctypes as C
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import cfit64 as c64
import side_abi
from guardx_amd import _cfit_native as n
from guardx_amd import build, cfit

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY, PREFIX = "cfit", "gxq"
LIB = build.SAFETY_LIBRARIES[KEY]
PROTOS = 8
MINE = ("gx_cfit.hip", "guardx_cfit.h")


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
def test_it_is_registered_in_the_seventh_mapping_only():
    assert list(build.SAFETY_LIBRARIES) == [KEY]
    assert all(KEY not in m for m in (build.LIBRARIES, build.LEARNER_LIBRARIES, build.UPDATE_LIBRARIES, build.FIT_LIBRARIES,
                                      build.GRAD_LIBRARIES, build.ACTOR_LIBRARIES))
    assert LIB not in build.actor_libraries()
    assert build.safety_libraries() == build.actor_libraries() + [LIB] and len(build.safety_libraries()) == 15
    # the six mappings and five functions before it keep their values
    assert list(build.ACTOR_LIBRARIES) == ["pifit"] and list(build.GRAD_LIBRARIES) == ["pgrad"] and list(build.FIT_LIBRARIES) == ["vfit"]
    assert list(build.UPDATE_LIBRARIES) == ["linesearch"] and list(build.LEARNER_LIBRARIES) == ["fisher"] and len(build.LIBRARIES) == 8
    assert [len(f()) for f in (build.actor_libraries, build.grad_libraries, build.fit_libraries, build.all_libraries,
                               build.every_library)] == [14, 13, 12, 11, 10]
    assert isinstance(LIB, build.Library) and type(LIB) is type(build.ACTOR_LIBRARIES["pifit"])
    text = open(os.path.join(ROOT, "guardx_amd", "build.py")).read()
    assert "SAFETY_LIBRARIES" in text and "safety_libraries()" in text
    side = open(os.path.join(ROOT, "guardx_amd", "_sidelib.py")).read()
    assert "safety_libraries()" in side and "actor_libraries()" in side


def test_declaration():
    assert LIB.macro == "GXQ_BUILD_ID" and os.path.basename(LIB.lib) == "libguardx_cfit.so" and n.LIB_PATH == LIB.lib
    assert LIB.sources == ["gx_cfit.hip"] and LIB.obj_dir is None and LIB.per_source_flags is None
    assert LIB.build_id_file == os.path.join(build.LIB_DIR, "CFIT_BUILD_ID")
    assert "guardx_amd/lib/CFIT_BUILD_ID" in open(os.path.join(ROOT, ".gitignore")).read().split()
    assert n._side.side is LIB and n._side.prefix == PREFIX


def test_the_id_covers_exactly_what_the_library_includes():
    hashed = {_norm(x) for x in LIB.sources + LIB.headers}
    assert len(LIB.sources + LIB.headers) == len(hashed) and hashed == _closure()
    assert {os.path.basename(p) for p in hashed} == {"gx_cfit.hip", "gx_device.h", "gx_policy.h", "guardx_cfit.h"}
    h = hashlib.sha256()
    h.update(build.compiler_id().encode() + b"\0")
    for name in sorted(os.path.relpath(p, build.CSRC) for p in _closure()):
        h.update(name.encode() + b"\0" + open(os.path.join(build.CSRC, name), "rb").read())
    h.update(repr(build.FLAGS).encode())
    assert LIB.source_hash() == h.hexdigest()[:24] and re.fullmatch(r"[0-9a-f]{24}", LIB.source_hash())
    others = build.actor_libraries()
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


def test_the_fourteen_libraries_before_it_keep_their_source_hashes_without_the_new_files(monkeypatch, tmp_path):
    """a copy of csrc and include without the two new files gives every other library the id it has in the tree: nothing
    an existing library hashes was touched, none of them reaches the new files, and so none shares a translation unit with
    the new library"""
    before = {lib.key: lib.source_hash() for lib in build.actor_libraries()}
    assert len(before) == 14
    shutil.copytree(build.CSRC, tmp_path / "guardx_amd" / "csrc")
    shutil.copytree(os.path.join(ROOT, "include"), tmp_path / "include")
    os.remove(tmp_path / "guardx_amd" / "csrc" / MINE[0])
    os.remove(tmp_path / "include" / MINE[1])
    monkeypatch.setattr(build, "CSRC", str(tmp_path / "guardx_amd" / "csrc"))
    assert {lib.key: lib.source_hash() for lib in build.actor_libraries()} == before
    with pytest.raises(OSError):
        LIB.source_hash()


def test_the_binding_matches_the_header():
    side_abi.assert_binding_matches_the_header(KEY, PREFIX, n, None, PROTOS, 7)
    assert n._side.symbols == n.SYMBOLS and len(_declared()) == PROTOS
    assert not re.search(r"\bdouble\b", side_abi.header(KEY))      # float64 data travels behind void*
    assert set(n.SYMBOLS) == {"gxq_fit", "gxq_gradient", "gxq_softplus_probe", "gxq_work_bytes", "gxq_param_count",
                              "gxq_default_workgroups", "gxq_build_id", "gxq_last_error"}
    assert (n.GXQ_HEAD_IDENTITY, n.GXQ_HEAD_SOFTPLUS, n.GXQ_HEAD_DOT) == (0, 1, 2)


@pytest.fixture(scope="module")
def defined():
    """{key: {symbol: type}} of what each built library defines (nm -D)"""
    build.build()
    out = {}
    for lib in build.safety_libraries():
        nm = subprocess.run(["nm", "-D", "--defined-only", lib.lib], capture_output=True, text=True, check=True).stdout
        out[lib.key] = {ln.split()[-1]: ln.split()[-2] for ln in nm.splitlines()}
    return out


def test_build_builds_fifteen_libraries(defined):
    assert len(defined) == 15 and all(os.path.exists(lib.lib) and not lib.needs_build() for lib in build.safety_libraries())


def test_the_export_list_is_the_header_and_nobody_elses(defined):
    mine = {s for s, t in defined[KEY].items() if t == "T" and s.startswith(("gx", "guardx_"))}
    assert mine == _declared() == set(n.SYMBOLS)
    for key, syms in defined.items():
        assert key == KEY or not mine & set(syms), key


def test_the_build_id_round_trip(defined):
    lib = n.load()
    assert lib.gxq_build_id().decode() == LIB.source_hash() == LIB.built_id()


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
SOFT, DOT, IDENT = n.GXQ_HEAD_SOFTPLUS, n.GXQ_HEAD_DOT, n.GXQ_HEAD_IDENTITY


def _gradient(lib, B=64, D=45, A=1, h=64, head=SOFT, theta=PTR, x=PTR, y=PTR, w=None, act=None, off=None, wg=0, work=PTR, g=PTR, loss=PTR,
              wsum=PTR):
    return lib.gxq_gradient(B, D, A, h, head, theta, x, y, w, act, off, wg, work, g, loss, wsum, None)


def _fit(lib, B=64, D=45, A=1, h=64, head=SOFT, theta=PTR, m=PTR, v=PTR, step0=0, x=PTR, y=PTR, w=None, stride=0, act=None, off=None, iters=3,
         hyper=True, wg=0, work=PTR, loss=PTR, wsum=PTR):
    arr = (C.c_double * 10)(1e-3, 0.9, 0.999, 1e-8, 0.9, 0.999, 0.81, 0.998, 0.729, 0.997)
    return lib.gxq_fit(B, D, A, h, head, theta, m, v, step0, x, y, w, stride, act, off, iters, C.cast(arr, C.c_void_p) if hyper else None, wg,
                       work, loss, wsum, None)


def test_sizes(defined):
    lib = n.load()
    for D, A in ((45, 1), (43, 2), (1, 16), (128, 8)):
        assert lib.gxq_param_count(D, A, 64) == c64.param_count(D, A, 64) == cfit.param_count(D, A)
    assert lib.gxq_param_count(43, 2, 8) == c64.param_count(43, 2, 8)
    assert lib.gxq_param_count(0, 1, 64) == lib.gxq_param_count(43, 0, 64) == lib.gxq_param_count(43, 2, 0) == -1
    rows = (0, -1, 1, 64, 65, 256 * 64, 256 * 64 + 1, 400000, 2 ** 31 - 1)
    assert [lib.gxq_default_workgroups(B) for B in rows] == [0, 0, 1, 1, 2, 256, 256, 256, 256]
    P = c64.param_count(45, 1)
    # one partial vector of P float32 and two float64 per workgroup
    assert lib.gxq_work_bytes(65, 45, 1, SOFT, 0) == (4 * 2 * P + 7) // 8 * 8 + 16 * 2
    assert lib.gxq_work_bytes(65, 45, 1, IDENT, 5) == (4 * 5 * P + 7) // 8 * 8 + 16 * 5
    assert lib.gxq_work_bytes(400000, 43, 2, DOT, 0) == 4 * 256 * c64.param_count(43, 2) + 16 * 256


def test_arg_errors_fire_before_a_launch(defined):
    lib = n.load()
    for kw in [dict([(k, None)]) for k in ("theta", "x", "y", "work", "g", "loss", "wsum")] + \
            [dict(B=0), dict(B=-1), dict(D=0), dict(A=0), dict(wg=-1), dict(wg=4097), dict(head=3), dict(head=-1), dict(head=DOT, A=2, act=None)]:
        assert _gradient(lib, **kw) == n.GXQ_ERR_ARG, kw
        assert b"gxq_gradient" in lib.gxq_last_error()
    for kw in [dict([(k, None)]) for k in ("theta", "m", "v", "x", "y", "work", "loss", "wsum")] + \
            [dict(hyper=False), dict(B=0), dict(D=0), dict(A=-2), dict(wg=-1), dict(wg=4097), dict(iters=-1), dict(step0=-1), dict(head=7),
             dict(head=DOT, A=2), dict(w=PTR, stride=1), dict(w=PTR, stride=-64), dict(w=PTR, stride=128)]:
        assert _fit(lib, **kw) == n.GXQ_ERR_ARG, kw
        assert b"gxq_fit" in lib.gxq_last_error()
    with pytest.raises(n.GxqError, match="guardx cfit status 1: gxq_gradient: null pointer") as e:
        n.check(_gradient(lib, x=None))
    assert e.value.status == n.GXQ_ERR_ARG
    assert lib.gxq_softplus_probe(-1, PTR, PTR, PTR, None) == lib.gxq_softplus_probe(4, None, PTR, PTR, None) == n.GXQ_ERR_ARG
    assert lib.gxq_softplus_probe(4, PTR, None, PTR, None) == lib.gxq_softplus_probe(4, PTR, PTR, None, None) == n.GXQ_ERR_ARG
    assert lib.gxq_softplus_probe(0, PTR, PTR, PTR, None) == n.GXQ_OK
    for args in ((0, 45, 1, SOFT, 0), (64, 0, 1, SOFT, 0), (64, 45, 0, SOFT, 0), (64, 45, 1, SOFT, -1), (64, 45, 1, SOFT, 4097), (64, 45, 1, 3, 0)):
        assert lib.gxq_work_bytes(*args) == -1, args
    # zero iterations launch nothing, with or without weights
    assert _fit(lib, iters=0) == _fit(lib, iters=0, w=PTR, stride=64) == _fit(lib, iters=0, head=DOT, A=2, act=PTR) == n.GXQ_OK


def test_unsupported_shapes_fire_before_a_launch(defined):
    lib = n.load()
    for kw, word in ((dict(h=128), "hidden width 64"), (dict(h=32), "hidden width 64"), (dict(D=129), "input width"),
                     (dict(A=2), "one output"), (dict(head=IDENT, A=2), "one output"), (dict(head=DOT, A=3, act=PTR), "even action width"),
                     (dict(head=DOT, A=18, act=PTR), "even action width"), (dict(head=DOT, A=1, act=PTR), "even action width")):
        assert _gradient(lib, **kw) == n.GXQ_ERR_UNSUPPORTED, kw
        assert word in lib.gxq_last_error().decode()
        assert _fit(lib, **kw) == n.GXQ_ERR_UNSUPPORTED, kw
        assert word in lib.gxq_last_error().decode()
    assert lib.gxq_work_bytes(64, 129, 1, SOFT, 0) == lib.gxq_work_bytes(64, 43, 3, DOT, 0) == lib.gxq_work_bytes(64, 43, 2, SOFT, 0) == -1
    assert lib.gxq_work_bytes(64, 128, 16, DOT, 0) > 0 and lib.gxq_work_bytes(1, 1, 1, IDENT, 4096) > 0


# ---------------------------------------------------------------------------------------------------------------------
# guardx_amd.cfit refuses before it loads or launches anything
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_library(monkeypatch):
    """nothing below may get as far as the library"""
    def refuse():
        raise AssertionError("the library was loaded")
    monkeypatch.setattr(n, "load", refuse)
    monkeypatch.setattr(cfit._n, "load", refuse)


def _seq(D=45, h=64, h2=None, out=1, act=torch.nn.Tanh, tail=None, bias=True, layers=2):
    nn = torch.nn
    h2 = h2 or h
    mods = [nn.Linear(D, h, bias=bias), act()]
    if layers >= 2:
        mods += [nn.Linear(h, h2, bias=bias), act()]
    if layers >= 3:
        mods += [nn.Linear(h2, h2, bias=bias), act()]
    mods.append(nn.Linear(h2 if layers >= 2 else h, out, bias=bias))
    if tail is not None:
        mods.append(tail)
    return nn.Sequential(*mods)


class _Mod(torch.nn.Module):
    def __init__(self, extra=False, **nets):
        super().__init__()
        for k, v in nets.items():
            setattr(self, k, v)
        if extra:
            self.extra = torch.nn.Parameter(torch.zeros(3))


def test_the_head_is_read_off_the_module(no_library):
    sp = torch.nn.Softplus
    for mod, head, Din, A in ((_Mod(c_net=_seq(45, tail=sp())), "softplus", 45, 1), (_Mod(v_net=_seq(44, tail=sp())), "softplus", 44, 1),
                              (_Mod(g_net=_seq(43, out=2)), "dot", 43, 2), (_Mod(g_net=_seq(43, out=16, tail=torch.nn.Identity())), "dot", 43, 16),
                              (_Mod(v_net=_seq(64, tail=torch.nn.Identity())), "identity", 64, 1)):
        QF = cfit.CostCriticFit(mod, lr=1e-3)
        assert (QF.head, QF.Din, QF.A, QF.P) == (head, Din, A, c64.param_count(Din, A))
        assert cfit.CostCriticFit(mod, lr=1e-3, head=head).head == head
        other = [k for k in cfit.HEADS if k != head][0]
        with pytest.raises(NotImplementedError, match=f"head='{other}' was asked for, the module's head is '{head}'"):
            cfit.CostCriticFit(mod, lr=1e-3, head=other)
    with pytest.raises(ValueError, match="head must be one of"):
        cfit.CostCriticFit(_Mod(v_net=_seq(64)), lr=1e-3, head="relu")
    for head in c64.HEADS:                                       # and the modules tests/cfit64.py declares
        assert cfit.CostCriticFit(c64.make_module(head, 43, 2), lr=1e-3).head == head
    assert cfit.CostCriticFit(c64.make_module("softplus", 44, attr="v_net"), lr=1e-3).head == "softplus"


def test_modules_it_does_not_support_in_the_packers_words(no_library):
    from guardx_amd import Engine
    sp = torch.nn.Softplus
    cases = [
        (_Mod(c_net=_seq(45)), Engine.pack_q_critic, "rollout_usl"),                                  # no Softplus
        (_Mod(c_net=_seq(45, tail=sp(beta=2))), Engine.pack_q_critic, "rollout_usl"),
        (_Mod(c_net=_seq(45, tail=sp(), act=torch.nn.ReLU)), Engine.pack_q_critic, "rollout_usl"),
        (_Mod(c_net=_seq(45, tail=sp(), layers=1)), Engine.pack_q_critic, "rollout_usl"),
        (_Mod(c_net=_seq(45, tail=sp(), out=2)), Engine.pack_q_critic, "rollout_usl"),
        (_Mod(g_net=_seq(43, out=3)), Engine.pack_g_net, "rollout_safelayer"),
        (_Mod(g_net=_seq(43, out=18)), Engine.pack_g_net, "rollout_safelayer"),
        (_Mod(g_net=_seq(43, out=2, tail=sp())), Engine.pack_g_net, "rollout_safelayer"),
        (_Mod(g_net=_seq(43, out=2, h2=32)), Engine.pack_g_net, "rollout_safelayer"),
        (_Mod(v_net=_seq(44, layers=3)), Engine.pack_critic, "the cost critic pass"),
        (_Mod(v_net=_seq(44, out=2)), Engine.pack_critic, "the cost critic pass"),
    ]
    for mod, pack, theirs in cases:
        with pytest.raises(NotImplementedError) as want:
            pack(mod)
        with pytest.raises(NotImplementedError) as mine:
            cfit.CostCriticFit(mod, lr=1e-3)
        assert str(mine.value) == str(want.value).replace(theirs, "CostCriticFit") and "CostCriticFit" in str(mine.value)
    with pytest.raises(NotImplementedError, match=re.escape("CostCriticFit supports nn.Softplus(beta=1, threshold=20)")):
        cfit.CostCriticFit(_Mod(v_net=_seq(44, tail=sp(threshold=10))), lr=1e-3)
    for mod, words in ((torch.nn.Linear(3, 2), ".c_net (usl, lpg), .g_net (safelayer) or .v_net"),
                       (_Mod(c_net=_seq(45, h=128, tail=sp())), "hidden width 64, not 128"),
                       (_Mod(g_net=_seq(43, out=2, bias=False)), "Linear layers with a bias"),
                       (_Mod(v_net=_seq(129)), "input width <= 128, not 129"),
                       (_Mod(extra=True, v_net=_seq(44)), "parameters() are its network's weights and biases")):
        with pytest.raises(NotImplementedError, match=re.escape(words)):
            cfit.CostCriticFit(mod, lr=1e-3)


def test_optimizers_it_does_not_support(no_library):
    mod = c64.make_module("softplus", 45)
    for kw in (dict(weight_decay=1e-4), dict(amsgrad=True)):
        with pytest.raises(NotImplementedError, match="CostCriticFit supports Adam without weight_decay and amsgrad"):
            cfit.CostCriticFit(mod, lr=1e-3, **kw)
    for kw in (dict(lr=-1.0), dict(lr=1e-3, eps=-1e-8), dict(lr=1e-3, betas=(1.0, 0.999)), dict(lr=1e-3, betas=(0.9, -0.1))):
        with pytest.raises(ValueError, match="CostCriticFit: lr and eps must not be negative"):
            cfit.CostCriticFit(mod, **kw)
    for wg in (-1, 4097, 1.5):
        with pytest.raises(ValueError, match="CostCriticFit: workgroups must be 0"):
            cfit.CostCriticFit(mod, lr=1e-3, workgroups=wg)


@pytest.mark.parametrize("x,words", [
    (np.zeros((8, 45), np.float32), "CostCriticFit: x must be a float32 tensor"),
    (torch.zeros(8, 44), "CostCriticFit: x must be (B, 45)"),
    (torch.zeros(8, 50)[:, :45], "CostCriticFit: x must be contiguous"),
    (torch.zeros(8, 45), "CostCriticFit: x lives on cpu; it must be on a cuda device"),
    (torch.zeros(8, 45, dtype=torch.float64), "CostCriticFit: x must be a float32 tensor"),
])
def test_batches_it_does_not_accept(x, words, no_library):
    QF = cfit.CostCriticFit(c64.make_module("softplus", 45), lr=1e-3)
    for call in (QF.fit, QF.gradient):
        with pytest.raises(ValueError, match=re.escape(words)):
            call(x, torch.zeros(8))


def test_the_rows_entries_and_the_fit_arguments(no_library):
    dev = torch.device("cuda:0")
    for name, v, shape, words in (("act", torch.zeros(8, 3), (8, 2), "must be (8, 2)"), ("target", torch.zeros(9), (8,), "must be (8,)"),
                                  ("weight", torch.zeros(3, 9), (3, 8), "must be (3, 8)"),
                                  ("offset", torch.zeros(8, dtype=torch.float64), (8,), "must be a float32 tensor"),
                                  ("weight", torch.zeros(16)[::2], (8,), "must be contiguous"),
                                  ("target", torch.zeros(8), (8,), "lives on cpu; it must be on cuda:0, where x is")):
        with pytest.raises(ValueError, match=re.escape(f"CostCriticFit: {name} {words}")):
            cfit._checked(name, v, shape, dev)
    QF = cfit.CostCriticFit(c64.make_module("softplus", 45), lr=1e-3)
    for iters in (-1, 1.5):
        with pytest.raises(ValueError, match="CostCriticFit.fit: iters must be a non-negative integer"):
            QF.fit(torch.zeros(8, 45), torch.zeros(8), iters=iters)


def test_the_package_exports_it():
    import guardx_amd
    assert guardx_amd.cfit is cfit and guardx_amd.CostCriticFit is cfit.CostCriticFit
    assert cfit.HEADS == ("identity", "softplus", "dot") and callable(cfit.downsample_weights)
    assert "guardx_amd.cfit" in guardx_amd.vfit.__doc__          # where vfit sends SCPO's down-sampled loss
