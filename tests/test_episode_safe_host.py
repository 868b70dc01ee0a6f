"""The host side of the one-episode form of the three safe-action rollouts (Engine.rollout_safelayer / rollout_usl /
rollout_lpg(..., episode=True)): the argument checks of the guardx_<library>_policy_step_episode and guardx_<library>_tail_probe entries and of
guardx_episode_finish_cols (nothing launches), the device code of the changed libraries, the host-tensor path of the extended
episode_rollout_batch against a numpy restatement of the learners' one-episode buffers
(safe_rl_libX/safelayer_one_episode/safelayer.py:30-140, usl_one_episode/usl.py:22-144; LPG's is USL's under another
name), and the sizing of tests/test_gpu_episode_safe.py's inputs on the CPU checker's engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_episode_host import OneEpisodeBufferNP, first_done_np, _synthetic, _torch_out, _close, T_, N_, A_

LIBS = {"safelayer": ("gxl", "g_hidden", 18), "usl": ("gxu", "c_hidden", 21), "lpg": ("gxp", "c_hidden", 21)}


# ---------------------------------------------------------------------------------------------------------------------
# argument checks
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def built():
    from guardx_amd import build
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU


def _native(key):
    import importlib
    n = importlib.import_module("guardx_amd._%s_native" % key)
    return n, n.load(), getattr(n, "Gx%sStepArgs" % LIBS[key][0][2])


@pytest.mark.parametrize("key", sorted(LIBS))
def test_the_episode_entries_check_their_arguments(built, key):
    """guardx_<library>_policy_step_episode refuses what gx?_policy_step refuses and a bad bookkeeping struct; guardx_<library>_tail_probe its own
    arguments.  Every call fails (or has nothing to do) before any HIP call: the pointers are never dereferenced."""
    from guardx_amd._sidelib import FirstDoneState
    n, lib, Args = _native(key)
    prefix, h3, _ = LIBS[key]
    P = prefix.upper()
    OK, ARG, UNS = (getattr(n, f"{P}_{s}") for s in ("OK", "ERR_ARG", "ERR_UNSUPPORTED"))
    step, probe = (getattr(lib, "guardx_%s_%s" % (key, s)) for s in ("policy_step_episode", "tail_probe"))
    old, err = getattr(lib, prefix + "_policy_step"), getattr(lib, prefix + "_last_error")
    fake = 4096

    def args(**over):
        a = Args()
        a.struct_size = C.sizeof(Args)
        a.N, a.D, a.A, a.hidden, a.T, a.t = 4, 43, 2, 64, 3, 1
        setattr(a, h3, 64)
        for f, _ in Args._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a

    def book(**over):
        b = FirstDoneState()
        b.struct_size, b.t_base = C.sizeof(b), 0
        b.d_first_done = b.d_ep_len = b.d_ep_ret = b.d_ep_cost = fake
        for k, v in over.items():
            setattr(b, k, v)
        return b
    assert C.sizeof(FirstDoneState) == 40
    assert step(None, C.byref(book()), None) == ARG
    assert step(C.byref(args(struct_size=8)), C.byref(book()), None) == ARG and b"struct_size" in err()
    own = dict(safelayer=[dict(d_prev_c=None), dict(d_g=None)], usl=[dict(niter=-1), dict(d_iters=None)],
               lpg=[dict(d_q_init=None), dict(d_lam=None)])[key]
    for bad in [dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(d_params=None), dict(d_work=None), dict(d_cost_in=None),
                dict(d_obs_rd=None), dict(d_act_safe=None), dict(t=3, d_val_last=None), dict(t=0, d_obs0=None)] + own:
        assert step(C.byref(args(**bad)), C.byref(book()), None) == ARG, bad
        assert old(C.byref(args(**bad)), None) == ARG, bad
    for bad in (dict(hidden=96), {h3: 0}, dict(A=3), dict(A=18), {"D": 5000, "hidden": 256, h3: 256}):
        assert step(C.byref(args(**bad)), C.byref(book()), None) == UNS, bad
    # the bookkeeping argument: checked even where N == 0 leaves nothing to launch
    assert step(C.byref(args(N=0)), None, None) == ARG and b"bookkeeping" in err()
    for bad in (dict(struct_size=8), dict(t_base=-1), dict(d_first_done=None), dict(d_ep_len=None), dict(d_ep_ret=None),
                dict(d_ep_cost=None)):
        assert step(C.byref(args(N=0)), C.byref(book(**bad)), None) == ARG, bad
        assert step(C.byref(args()), C.byref(book(**bad)), None) == ARG, bad
    assert step(C.byref(args(N=0)), C.byref(book(t_base=7)), None) == OK
    assert step(C.byref(args(t=0, d_cost_in=None, d_obs_rd=None, N=0)), C.byref(book()), None) == OK

    def tail(n_=4, D=43, A=2, h=64, hh=64, ptrs=None):
        return probe(n_, D, A, h, hh, *([fake] * 6 if ptrs is None else ptrs), None)
    assert tail(n_=-1) == ARG
    for i in range(6):
        p = [fake] * 6
        p[i] = None
        assert tail(ptrs=p) == ARG, i
    assert tail(h=96) == UNS and tail(hh=32) == UNS and tail(A=3) == UNS and tail(D=5000, h=256, hh=256) == UNS
    assert tail(n_=0) == OK


def test_finish_cols_checks_its_arguments(built):
    from guardx_amd import _episode_native as n
    lib = n.load()
    fake = 4096

    def cols(*specs):
        arr = (n.GxeFinishCol * max(1, len(specs)))()
        for c, (s, d, w) in zip(arr, specs):
            c.d_src, c.d_dst, c.width = s, d, w
        return C.cast(arr, C.c_void_p)

    def finish(N=4, T=3, D=5, A=2, ptrs=None, n_cols=0, cl=None, q=(None, None, None), count=fake):
        p = [fake] * 20 if ptrs is None else ptrs
        return lib.guardx_episode_finish_cols(N, T, D, A, 0.99, 0.95, *p, n_cols, cl, *q, count, None)
    assert n.FINISH_MAX_COLS == 4 and C.sizeof(n.GxeFinishCol) == 24
    # what gxe_finish refuses
    assert finish(N=-1) == n.GXE_ERR_ARG and finish(T=0) == n.GXE_ERR_ARG and finish(D=0) == n.GXE_ERR_ARG
    assert finish(N=1 << 20, T=1 << 12) == n.GXE_ERR_UNSUPPORTED
    for i in (0, 1, 7, 11, 12, 17):
        p = [fake] * 20
        p[i] = None
        assert finish(ptrs=p) == n.GXE_ERR_ARG, i
    assert finish(count=None) == n.GXE_ERR_ARG
    p = [fake] * 20
    p[8] = None
    assert finish(ptrs=p) == n.GXE_ERR_ARG and b"cost channel" in lib.gxe_last_error()
    # its own
    assert finish(n_cols=-1) == n.GXE_ERR_ARG and finish(n_cols=5, cl=cols()) == n.GXE_ERR_ARG
    assert finish(n_cols=1, cl=None) == n.GXE_ERR_ARG and b"column list" in lib.gxe_last_error()
    for spec in ((None, fake, 2), (fake, None, 2), (fake, fake, 0)):
        assert finish(n_cols=2, cl=cols((fake, fake, 1), spec)) == n.GXE_ERR_ARG, spec
    for q in ((fake, None, None), (fake, fake, None), (None, fake, fake)):
        assert finish(q=q) == n.GXE_ERR_ARG and b"target" in lib.gxe_last_error()


@pytest.mark.parametrize("key,count", [("safelayer", 18), ("usl", 21), ("lpg", 21), ("episode", 20)])
def test_no_scratch_in_the_device_code(tmp_path, key, count):
    """the libraries whose kernels take the episode mode as a uniform argument, and the episode library with the
    extended gather launch: the kernel counts of before (the mode is no template parameter), no scratch memory, and
    within the 168 registers that 12 waves per workgroup leave a lane"""
    import subprocess
    from guardx_amd import build
    step_h = open(os.path.join(build.CSRC, "gx_step.h")).read()
    assert "GX_D void episode_book(" in step_h and "GX_D void stage_rows(" in step_h   # what this check is about
    asm = tmp_path / ("gx_%s.s" % key)
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_%s.hip" % key)])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print(key, "kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == count and max(scratch) == 0 and max(vgpr) <= 168


def test_the_bookkeeping_struct_is_one_declaration_and_the_first_abi_stands(built):
    """gx_first_done_state stands in the three public headers under one guard, letter for letter, and matches the
    binding; the new entries are exported and declared under the library's full name, outside the gx?_ symbol sets"""
    import subprocess
    import side_abi
    from guardx_amd import build, _sidelib, _episode_native
    texts = []
    for key in sorted(LIBS):
        text = open(os.path.join(os.path.dirname(build.CSRC), "..", "include", "guardx_%s.h" % key)).read()
        m = re.search(r"#ifndef GX_FIRST_DONE_STATE_DEFINED\n(.*?)#endif", text, flags=re.S)
        texts.append(m.group(1))
        n, _, Args = _native(key)
        assert sorted(n.EPISODE_SYMBOLS) == ["guardx_%s_policy_step_episode" % key, "guardx_%s_tail_probe" % key]
        assert not set(n.EPISODE_SYMBOLS) & set(n.SYMBOLS)
        for name in n.EPISODE_SYMBOLS:
            assert re.search(r"\b%s_status %s\(" % (LIBS[key][0], name), side_abi.header(key)), name
        out = subprocess.run(["nm", "-D", "--defined-only", n.LIB_PATH], capture_output=True, text=True, check=True).stdout
        assert {ln.split()[-1] for ln in out.splitlines() if re.search(r"\sT\s+guardx_", ln)} == set(n.EPISODE_SYMBOLS)
    assert texts[0] == texts[1] == texts[2]
    fields = re.findall(r"(uint32_t|int32_t\*|int32_t|float\*)\s+(\w+);", re.sub(r"/\*.*?\*/", "", texts[0], flags=re.S))
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "int32_t*": C.c_void_p, "float*": C.c_void_p}
    assert [(nm, ctype[t]) for t, nm in fields] == [(f[0], f[1]) for f in _sidelib.FirstDoneState._fields_]
    assert list(_episode_native.COLS_SYMBOLS) == ["guardx_episode_finish_cols"]
    assert re.search(r"\bgxe_status guardx_episode_finish_cols\(", side_abi.header("episode"))
    assert not any("first_done" in h for lib in build.LIBRARIES.values() for h in lib.headers)


# ---------------------------------------------------------------------------------------------------------------------
# the one-episode buffers of the three learners in numpy
# ---------------------------------------------------------------------------------------------------------------------
class SafeEpisodeBufferNP(OneEpisodeBufferNP):
    """SafeLayerBufferX (kind 'safelayer': act_safe, cost, prev_cost stored and returned) and USLBufferX / LPGBufferX
    (kind 'q': act_safe, cost, qc stored; act_safe, cost, targetc returned) of the one-episode directories, on top of the
    TRPO one-episode restatement they extend"""

    def __init__(self, kind, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95):
        super().__init__(env_num, max_ep_len, obs_dim, act_dim, gamma, lam)
        f = np.float32
        self.kind = kind
        self.act_safe_buf = np.zeros((env_num, max_ep_len, act_dim), f)
        self.cost_buf, self.own_buf = np.zeros((env_num, max_ep_len), f), np.zeros((env_num, max_ep_len), f)
        self.targetc_buf = np.zeros((env_num, max_ep_len), f)

    def store(self, obs, act, act_safe, rew, val, logp, mu, logstd, cost, own):
        p = self.ptr
        super().store(obs, act, rew, val, logp, mu, logstd)
        self.act_safe_buf[:, p], self.cost_buf[:, p], self.own_buf[:, p] = act_safe, cost, own

    def finish_path(self, last_val, first_done_idx):
        super().finish_path(last_val, first_done_idx)
        if self.kind == 'q':                                      # usl.py:105-107
            for e in range(self.N):
                sl = slice(0, int(first_done_idx[e]))
                qcs = np.append(self.own_buf[e, sl], 0).astype(np.float32)
                costs = np.append(self.cost_buf[e, sl], 0).astype(np.float32)
                self.targetc_buf[e, sl] = costs[:-1] + np.float32(self.gamma) * qcs[1:]

    def get(self):
        valid = np.where(self.valid_buf.reshape(self.N * self.T) == 1)
        data = super().get()                                      # (clears valid_buf)
        flat = lambda x: x.reshape(self.N * self.T, *x.shape[2:])[valid]   # noqa: E731
        data.update(act_safe=flat(self.act_safe_buf), cost=flat(self.cost_buf))
        data.update(prev_cost=flat(self.own_buf)) if self.kind == 'safelayer' else data.update(targetc=flat(self.targetc_buf))
        return data


def safe_episode_batch_np(g, learner, gamma=0.99, lam=0.95):
    """the learner's epoch (safelayer_one_episode/safelayer.py:499-578, usl_one_episode/usl.py:463-543) over a recorded
    episode=True result `g` (numpy): store every step, one finish_path with first_done_idx and the bootstrap of the envs
    that never finished and whose last observation is finite, get"""
    T, N = g['rew'].shape
    A = g['act'].shape[-1]
    buf = SafeEpisodeBufferNP('safelayer' if learner == "safelayer" else 'q', N, T, g['obs'].shape[-1], A, gamma, lam)
    logstd = np.broadcast_to(g['logstd'].reshape(1, A), (N, A))
    own = g['prev_cost'] if learner == "safelayer" else g['qc']
    for t in range(T):
        buf.store(g['obs'][t], g['act'][t], g['act_safe'][t], g['rew'][t], g['val'][t], g['logp'][t], g['mu'][t], logstd,
                  g['cost'][t], own[t])
    fd = first_done_np(g['done'])
    assert (fd == g['first_done']).all()
    boot = (fd == 0) & np.isfinite(g['obs_last']).all(1)
    buf.finish_path(np.where(boot, g['val_last'], np.float32(0)), np.where(fd > 0, fd, T))
    return buf.get()


def _synthetic_safe(seed, learner):
    """test_episode_host's synthetic episode (envs done at step 1, inside, at the last step and never; L == T on envs 0, 3,
    5, 7) with the learner's columns"""
    g = _synthetic(seed, False)
    rng = np.random.default_rng(seed + 100)
    g['act_safe'] = rng.uniform(-1, 1, size=(T_, N_, A_)).astype(np.float32)
    if learner == "safelayer":
        g['prev_cost'] = rng.random((T_, N_)).astype(np.float32)
    else:
        g['qc'] = (rng.random((T_, N_)) * 3).astype(np.float32)
    return g


@pytest.mark.parametrize("learner", ["safelayer", "usl", "lpg"])
def test_episode_rollout_batch_on_host_tensors_against_the_buffer_restatement(learner):
    from guardx_amd.rollout_buffer import episode_rollout_batch
    g = _synthetic_safe(5, learner)
    want = safe_episode_batch_np(g, learner)
    got = episode_rollout_batch(_torch_out(g))
    L = np.where(g['first_done'] > 0, g['first_done'], T_)
    assert got.pop('n_valid') == int(L.sum()) == len(want['ret'])
    extra = ('act_safe', 'cost', 'prev_cost') if learner == "safelayer" else ('act_safe', 'cost', 'targetc')
    assert set(got) == set(want) == {'obs', 'act', 'ret', 'adv', 'logp', 'mu', 'logstd'} | set(extra)
    for k in ('obs', 'act', 'logp', 'mu', 'logstd') + extra:      # copies, and targetc's one multiply and one add: the bits
        np.testing.assert_array_equal(got[k].numpy().view(np.uint32), want[k].view(np.uint32), err_msg=k)
    _close(got, want, ('ret', 'adv'))
    if learner != "safelayer":
        off = np.concatenate([[0], np.cumsum(L)])
        tc = got['targetc'].numpy()
        for e in range(N_):
            np.testing.assert_array_equal(tc[off[e + 1] - 1], g['cost'][L[e] - 1, e])       # t = L - 1: qc counts as 0
            np.testing.assert_array_equal(tc[off[e]:off[e + 1] - 1],
                                          g['cost'][:L[e] - 1, e] + np.float32(0.99) * g['qc'][1:L[e], e])
        assert (L == T_).sum() >= 3 and (L == 1).any()
    # rollout_episode's own result is served as before
    plain = episode_rollout_batch(_torch_out(_synthetic(5, False)))
    assert set(plain) == {'obs', 'act', 'ret', 'adv', 'logp', 'mu', 'logstd', 'n_valid'}
    for k in ('ret', 'adv', 'obs'):
        np.testing.assert_array_equal(plain[k].numpy().view(np.uint32), got[k].numpy().view(np.uint32))
    with pytest.raises(KeyError, match="cost"):
        episode_rollout_batch({k: v for k, v in _torch_out(g).items() if k != 'cost'})
    with pytest.raises(ValueError, match="shape"):
        episode_rollout_batch(dict(_torch_out(g), act_safe=_torch_out(g)['act_safe'][:-1]))


# ---------------------------------------------------------------------------------------------------------------------
# sizing the GPU tests' inputs on the CPU checker's engine
# ---------------------------------------------------------------------------------------------------------------------
def _closed_loop(O, learner, ac, third, T, kw, seed):
    """the learner's one-episode loop on the checker's engine `O` (reset, state planted; O.obs0 its observation) with the
    policy and the correction in float64 and the action handed over in float32, no reset_done: -> (rows before an env's
    first done, those of them the correction acted on, first_done)"""
    from oracle import policy64
    import safelayer64
    import usl64
    import lpg64
    pol = policy64.ActorCritic(ac)
    N = O.N
    env = np.arange(N, dtype=np.int64)
    o, prev_c, fd = O.obs0, np.zeros(N, np.float32), np.zeros(N, np.int64)
    Q = None if learner == "safelayer" else usl64.QCritic(third)
    rows = acted = 0
    for t in range(T):
        o = np.where(np.isfinite(o), o, 0).astype(np.float32)
        w = pol.step(o, seed, env, np.full(N, t, np.int64))
        act = w['act'].astype(np.float32)
        if learner == "safelayer":
            g, dg = safelayer64.g_values(third, o)
            c = safelayer64.correction64(g, dg, w['act'], w['act_b'], prev_c, kw['delta'])
            a_safe, did = c['a_safe'], c['corrected']
        elif learner == "usl":
            it = Q.iterate(o, act, kw['delta'], 20, 0.05, 1.0 / N)
            a_safe, did = it['a_safe'], it['iters'] > 0
        else:
            r = lpg64.probe64(Q, o, act, np.zeros(N), kw['delta'], kw['grad_scale'])
            a_safe, did = r['a_safe'], r['lam'] > 0
        live = fd == 0
        rows += int(live.sum())
        acted += int((did & live).sum())
        o, _, d, info = O.step(np.asarray(a_safe, np.float32))
        fd = np.where(live & (d > 0), t + 1, fd)
        prev_c = np.asarray(info['cost'], np.float32)
    return rows, acted, fd


@pytest.mark.parametrize("shape", range(5))
@pytest.mark.parametrize("learner", ["safelayer", "usl", "lpg"])
def test_the_chosen_inputs_are_corrected(oracle, learner, shape):
    """the engines, planted states, networks and keywords of tests/test_gpu_episode_safe.py's twin test on the CPU
    checker's engine with the float64 restatements: the correction acts on at least a fifth of the rows before an env's
    first done, twice what the GPU test asks for (its fp32 trajectory differs)"""
    import test_gpu_episode_safe as tg
    from helpers import random_state
    from test_gpu_episode import STATE_SEED
    from test_gpu_statewise import _cfg, SEED
    robot, h, h3, N = tg.SHAPES[shape]
    O = oracle.OracleEngine(_cfg(robot, N, num_steps=tg.NUM_STEPS), n_candidates=max(40000, 100 * N))
    O.obs0 = O.reset()
    s = random_state(N, 8, np.random.default_rng(STATE_SEED), done_frac=0, robot=robot)
    s['steps'][:] = 0
    O.set_state(s)
    ac, third = tg.nets(learner, O.obs0.shape[1], O.na, h, h3)
    rows, acted, fd = _closed_loop(O, learner, ac, third, tg.T, tg.correct_kw(learner, robot), SEED)
    print(f"{learner} {robot} N={N}: corrected {acted} of {rows} rows before the first done; first_done {sorted(set(fd.tolist()))}")
    assert acted >= 2 * tg.SHARE * rows and rows >= 1
