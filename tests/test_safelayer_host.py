"""The host side of Engine.rollout_safelayer (the safety layer on the device path): packing g_net, the fourth library's
device code and argument checks (its build identity and ABI: tests/test_build_identity.py), the float32 transcription of the correction against the float64 one, the batch helper against a
numpy restatement of SafeLayerBufferX, and the sizing of the GPU tests' inputs on the CPU checker's engine."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle import policy64
from oracle.trpo_buffer_np import TRPOBufferNP
from helpers import task_config
import safelayer64



def _seq(D, h, A, tail=(), act=None, h2=None):
    import torch.nn as nn
    act = act or nn.Tanh
    h2 = h2 or h
    return nn.Sequential(nn.Linear(D, h), act(), nn.Linear(h, h2), act(), nn.Linear(h2, A), *tail)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_g_net():
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    from guardx_amd.safelayer import G_NET_ATTR, g_floats
    for D, A, h in ((43, 2, 64), (64, 8, 256)):
        net = _seq(D, h, A, (nn.Identity(),))                   # mlp([D, h, h, A], tanh): the reference shape
        flat = Engine.pack_g_net(net, act_dim=A)
        lin = [m for m in net if isinstance(m, nn.Linear)]
        want = torch.cat([t.detach().reshape(-1) for m in lin for t in (m.weight, m.bias)])
        assert torch.equal(flat, want) and flat.numel() == g_floats(D, A, h) and getattr(flat, G_NET_ATTR) == A

        class CCritic:                                          # safelayer_core.py C_Critic: the net sits in .g_net
            g_net = net
        assert torch.equal(Engine.pack_g_net(CCritic()), want)
        assert getattr(flat.clone(), G_NET_ATTR, None) is None
    with pytest.raises(NotImplementedError, match="outputs"):
        Engine.pack_g_net(_seq(43, 64, 8), act_dim=2)           # a wrong output width
    for why, bad in {"odd width": _seq(43, 64, 3), "width 18": _seq(43, 64, 18), "ReLU": _seq(43, 64, 2, act=nn.ReLU),
                     "Tanh output": _seq(43, 64, 2, (nn.Tanh(),)), "Softplus output": _seq(43, 64, 2, (nn.Softplus(),)),
                     "hidden 96": _seq(43, 96, 2), "unequal hidden": _seq(43, 64, 2, h2=128),
                     "one hidden layer": nn.Sequential(nn.Linear(43, 64), nn.Tanh(), nn.Linear(64, 2))}.items():
        with pytest.raises(NotImplementedError):
            Engine.pack_g_net(bad)
            pytest.fail(why)


# ---------------------------------------------------------------------------------------------------------------------
# the correction: float32 transcription against float64
# ---------------------------------------------------------------------------------------------------------------------
def test_correction32_against_correction64():
    """random (g, a, prev_c) over several scales and widths: every element of the float32 transcription within the
    float64 restatement's bound with exact inputs (dg = da = 0: the roundings of the fixed operation order alone); on an
    edge row either branch"""
    rng = np.random.default_rng(1)
    f = np.float32
    for A in (2, 8, 16):
        for delta in (0.0, 0.1):
            n = 50000
            g = (rng.normal(size=(n, A)) * rng.choice([1e-3, 0.1, 1.0, 20.0], size=(n, 1))).astype(f)
            a = (rng.normal(size=(n, A)) * 1.2).astype(f)
            pc = (rng.random(n) * (rng.random(n) < 0.5)).astype(f)
            got, pred = safelayer64.correction32(g, a, pc, delta)
            z = np.zeros_like(g, np.float64)
            c = safelayer64.correction64(g, z, a, z, pc, delta)
            want = dict(corr=c)
            worst, med, edge = safelayer64.compare_act_safe(dict(act_safe=got), want, f"A={A} delta={delta}")
            print(f"correction32 vs 64: A={A} delta={delta} worst err / bound {worst:.3f} median bound {med:.2e} edge rows {edge:.5f}")
            assert edge < 1e-3 and np.isfinite(c['a_safe_b']).all()
            share = float(c['corrected'].mean())
            assert 0.2 < share < 0.9
            # off the edge the two agree on the branch
            np.testing.assert_array_equal((pred > f(delta))[~c['edge']], c['corrected'][~c['edge']])
    # hand-worked: g = (3, 4), a = (0.5, 0.25), prev_c = 0.5: pred = 3, mult = 3 / 25, a_safe = a - 0.12 g
    got, pred = safelayer64.correction32(np.array([[3, 4]], f), np.array([[0.5, 0.25]], f), np.array([0.5], f))
    assert pred[0] == f(3.0)
    np.testing.assert_allclose(got[0], [0.5 - 0.36, 0.25 - 0.48], rtol=0, atol=1e-7)
    got, _ = safelayer64.correction32(np.array([[3, 4]], f), np.array([[-0.5, 1.7]], f), np.array([-4.0], f), 1.5)
    np.testing.assert_array_equal(got[0], np.array([-0.5, 1.7], f))          # pred = 1.3 <= delta: unclamped


# ---------------------------------------------------------------------------------------------------------------------
# device code and argument checks (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sl_lib():
    from guardx_amd import build, _safelayer_native
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _safelayer_native.load()    # refuses a library whose build id is not the tree's


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles every kernel of the library (16 step kernels, the probe kernel, the transpose)
    without scratch memory and within the 168 registers that 12 waves per workgroup (3 on a SIMD, 512 / 3 rounded down) leave a lane"""
    import subprocess
    from guardx_amd import build
    asm = tmp_path / "gx_safelayer.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_safelayer.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print("safelayer kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == 18 and max(scratch) == 0 and max(vgpr) <= 168


def test_sizes_and_bad_arguments_are_errors_not_crashes(sl_lib):
    from guardx_amd import _safelayer_native as n
    from guardx_amd.safelayer import policy_floats, g_floats
    lib = sl_lib
    for D, A in ((43, 2), (64, 8), (70, 10)):
        for h in (64, 128, 192, 256):
            assert lib.gxl_params_floats(D, A, h) == policy_floats(D, A, h)
            assert lib.gxl_g_floats(D, A, h) == g_floats(D, A, h)
            for hg in (64, 256):
                Dp = (D + 3) // 4 * 4
                assert lib.gxl_work_floats(D, A, h, hg) == 2 * (Dp * h + h * h) + Dp * hg + hg * hg
    assert lib.gxl_params_floats(43, 2, 96) == -1 and lib.gxl_params_floats(0, 2, 64) == -1
    assert lib.gxl_params_floats(43, 3, 64) == -1 and lib.gxl_work_floats(43, 2, 64, 32) == -1
    assert lib.gxl_g_floats(43, 18, 64) == -1
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxl_prepare(43, 2, 64, 64, None, fake, fake, None) == n.GXL_ERR_ARG
    assert lib.gxl_prepare(43, 2, 64, 96, fake, fake, fake, None) == n.GXL_ERR_UNSUPPORTED
    assert lib.gxl_prepare(5000, 2, 256, 256, fake, fake, fake, None) == n.GXL_ERR_UNSUPPORTED
    assert lib.gxl_correction_probe(4, 2, None, fake, fake, 0.0, fake, None) == n.GXL_ERR_ARG
    assert lib.gxl_correction_probe(-1, 2, fake, fake, fake, 0.0, fake, None) == n.GXL_ERR_ARG
    assert lib.gxl_correction_probe(4, 17, fake, fake, fake, 0.0, fake, None) == n.GXL_ERR_UNSUPPORTED
    assert lib.gxl_correction_probe(0, 2, fake, fake, fake, 0.0, fake, None) == n.GXL_OK

    def args(**over):
        a = n.GxlStepArgs()
        a.struct_size = C.sizeof(n.GxlStepArgs)
        a.N, a.D, a.A, a.hidden, a.g_hidden, a.T, a.t = 4, 43, 2, 64, 64, 3, 1
        for f, _ in n.GxlStepArgs._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.gxl_policy_step(None, None) == n.GXL_ERR_ARG
    assert lib.gxl_policy_step(C.byref(args(struct_size=8)), None) == n.GXL_ERR_ARG
    assert b"struct_size" in lib.gxl_last_error()
    for bad in (dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(d_params=None), dict(d_g_params=None),
                dict(d_prev_c=None), dict(d_cost_in=None), dict(d_act_safe=None), dict(d_g=None),
                dict(t=3, d_val_last=None), dict(t=0, d_obs0=None)):
        assert lib.gxl_policy_step(C.byref(args(**bad)), None) == n.GXL_ERR_ARG, bad
    for bad in (dict(hidden=96), dict(g_hidden=0), dict(A=3), dict(A=18), dict(D=5000, hidden=256, g_hidden=256)):
        assert lib.gxl_policy_step(C.byref(args(**bad)), None) == n.GXL_ERR_UNSUPPORTED, bad
    assert lib.gxl_policy_step(C.byref(args(N=0)), None) == n.GXL_OK          # N == 0: nothing to do
    assert lib.gxl_policy_step(C.byref(args(t=0, d_cost_in=None, d_obs_rd=None, N=0)), None) == n.GXL_OK


# ---------------------------------------------------------------------------------------------------------------------
# SafeLayerBufferX in numpy (safe_rl_libX/safelayer/safelayer.py:32-154): the TRPO restatement plus act_safe, cost and
# prev_cost, which it stores and returns untouched
# ---------------------------------------------------------------------------------------------------------------------
class SafeLayerBufferNP(TRPOBufferNP):
    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95):
        super().__init__(env_num, max_ep_len, obs_dim, act_dim, gamma, lam)
        f = np.float32
        self.act_safe_buf = np.zeros((env_num, max_ep_len, act_dim), f)
        self.cost_buf, self.prev_cost_buf = np.zeros((env_num, max_ep_len), f), np.zeros((env_num, max_ep_len), f)

    def store(self, obs, act, act_safe, rew, val, logp, mu, logstd, cost, prev_cost):   # safelayer.py:51-70
        p = self.ptr[0]
        super().store(obs, act, rew, val, logp, mu, logstd)
        self.act_safe_buf[:, p, :] = act_safe
        self.cost_buf[:, p] = cost
        self.prev_cost_buf[:, p] = prev_cost

    def get(self):                                                                       # safelayer.py:126-154
        data = super().get()
        N, T = self.env_num, self.max_ep_len
        data['act_safe'] = self.act_safe_buf.reshape(N * T, -1)
        data['cost'] = self.cost_buf.reshape(N * T)
        data['prev_cost'] = self.prev_cost_buf.reshape(N * T)
        return data


def safelayer_batch_np(g, gamma=0.99, lam=0.95):
    """the learner's collection loop (safelayer.py:514-583) over a recorded rollout_safelayer result `g` (numpy): store
    every step, finish_path with v = 0 for the envs done at that step, the closing finish_path of the time-out"""
    T, N = g['rew'].shape
    A = g['act'].shape[-1]
    buf = SafeLayerBufferNP(N, T, g['obs'].shape[-1], A, gamma, lam)
    logstd = np.broadcast_to(g['logstd'].reshape(1, A), (N, A))
    for t in range(T):
        buf.store(g['obs'][t], g['act'][t], g['act_safe'][t], g['rew'][t], g['val'][t], g['logp'][t], g['mu'][t], logstd,
                  g['cost'][t], g['prev_cost'][t])
        if t + 1 == T:
            buf.finish_path(np.zeros(N, np.float32), np.ones(N))
        elif g['done'][t].any():
            buf.finish_path(np.zeros(N, np.float32), g['done'][t])
    return buf.get()


def _synthetic(T, N, D, A, seed, no_done=False):
    rng = np.random.default_rng(seed)
    f = np.float32
    g = dict(obs=rng.normal(size=(T, N, D)).astype(f), act=rng.normal(size=(T, N, A)).astype(f),
             act_safe=rng.uniform(-1, 1, size=(T, N, A)).astype(f), mu=rng.normal(size=(T, N, A)).astype(f),
             logp=rng.normal(size=(T, N)).astype(f), rew=rng.normal(size=(T, N)).astype(f),
             val=rng.normal(size=(T, N)).astype(f), cost=rng.random((T, N)).astype(f),
             prev_cost=rng.random((T, N)).astype(f), logstd=np.linspace(-0.5, 0.1, A).astype(f),
             done=(rng.random((T, N)) < (0.0 if no_done else 0.2)).astype(f))
    if not no_done:
        g['done'][:, 0] = 0                                   # one env closed by the time-out alone
        g['done'][0, 1] = 1                                   # a one-step episode
        g['done'][T - 1, 2] = 1                               # done on the last step
    return g


@pytest.mark.parametrize("no_done", [False, True])
def test_safelayer_rollout_batch_against_the_buffer_restatement(no_done):
    """safelayer_rollout_batch on host tensors against SafeLayerBufferX.store / finish_path / get restated in numpy, on a
    synthetic rollout with dones (finish_path's per-env branch) and without (its batch branch)"""
    import torch
    from guardx_amd.rollout_buffer import safelayer_rollout_batch
    T, N, D, A = 30, 9, 5, 4
    g = _synthetic(T, N, D, A, 5, no_done)
    want = safelayer_batch_np(g)
    got = safelayer_rollout_batch({k: torch.from_numpy(v) for k, v in g.items()})
    assert set(got) == set(want) == {'obs', 'act', 'act_safe', 'ret', 'adv', 'logp', 'mu', 'logstd', 'cost', 'prev_cost'}
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=tol, atol=tol, err_msg=k)
    np.testing.assert_array_equal(got['act_safe'].numpy().reshape(N, T, A)[3, 7], g['act_safe'][7, 3])
    np.testing.assert_array_equal(got['prev_cost'].numpy().reshape(N, T)[4, 11], g['prev_cost'][11, 4])
    # per env, every episode segment is its own discounted sum
    ret = want['ret'].reshape(N, T)
    for e in range(N):
        start = 0
        for end in [t for t in range(T) if g['done'][t, e] > 0 or t == T - 1]:
            r = g['rew'][start:end + 1, e].astype(np.float64)
            exp = [sum(r[j] * 0.99 ** (j - i) for j in range(i, len(r))) for i in range(len(r))]
            np.testing.assert_allclose(ret[e, start:end + 1], exp, rtol=1e-5, atol=1e-5)
            start = end + 1
    with pytest.raises(KeyError, match="prev_cost"):
        safelayer_rollout_batch({k: torch.from_numpy(v) for k, v in g.items() if k != 'prev_cost'})


# ---------------------------------------------------------------------------------------------------------------------
# sizing the GPU tests' inputs on the CPU checker's engine
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [0, 1])
def test_chosen_inputs_exercise_both_branches_and_few_edges(oracle, case):
    """the engine, networks and seeds of tests/test_gpu_safelayer.py's correction tests, run as a closed loop on the
    checker's engine with the float64 restatement: corrected and uncorrected rows are each at least a tenth of all rows
    (with room to spare for the fp32 trajectory, which differs), rows within pred's own bound of delta stay far below
    the 1 % cap, and prev_cost is live"""
    import test_gpu_safelayer as tg
    from test_policy64 import ROBOTS
    robot, h, hg = tg.CORR_CASES[case]
    cfg = task_config(tg.CORR_N, seed=tg.CORR_CFG_SEED, goal_size=0.9, **dict(ROBOTS[robot], **tg.COSTLY))
    O = oracle.OracleEngine(cfg, n_candidates=max(40000, 100 * tg.CORR_N))
    O.obs0 = O.reset()
    ac, gm = tg.corr_nets(O.D, O.na, h, hg)
    for delta in (0.0, 0.05):
        rec = safelayer64.closed_loop(O, ac, gm, tg.CORR_T + tg.CORR_T2, tg.SEED, delta=delta)
        share, edge = float(rec['corrected'].mean()), float(rec['edge'].mean())
        print(f"safelayer sizing {robot} A={O.na} delta={delta}: corrected {share:.3f}, edge rows {edge:.5f}, "
              f"prev_cost > 0 on {float((rec['prev_cost'] > 0).mean()):.3f}, done {int(rec['done'].sum())}")
        assert 0.15 <= share <= 0.85
        assert edge <= tg.EDGE_CAP / 4
        assert (rec['prev_cost'] > 0).mean() > 0.05 and rec['done'][:-1].sum() > 0
        O.obs0 = O.reset()
