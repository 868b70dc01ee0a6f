"""The host side of Engine.rollout_usl (USL's gradient-descent safety loop on the device path): packing c_net, the fifth
library's device code and argument checks (its build identity and ABI: tests/test_build_identity.py), the float64 analytic gradient against torch autograd, the float32 update against the
float64 one, the batch helper against a numpy restatement of USLBufferX, and the sizing of the GPU tests' probe inputs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle.trpo_buffer_np import TRPOBufferNP
import usl64



def _seq(D, h, out=1, tail=None, act=None, h2=None):
    import torch.nn as nn
    act = act or nn.Tanh
    h2 = h2 or h
    tail = (nn.Softplus(),) if tail is None else tail
    return nn.Sequential(nn.Linear(D, h), act(), nn.Linear(h, h2), act(), nn.Linear(h2, out), *tail)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_q_critic():
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    from guardx_amd.usl import Q_CRITIC_ATTR, q_floats
    for D, A, h in ((43, 2, 64), (64, 8, 256)):
        net = _seq(D + A, h)                                    # mlp([D + A, h, h, 1], tanh, Softplus): the reference shape
        flat = Engine.pack_q_critic(net)
        lin = [m for m in net if isinstance(m, nn.Linear)]
        want = torch.cat([t.detach().reshape(-1) for m in lin for t in (m.weight, m.bias)])
        assert torch.equal(flat, want) and flat.numel() == q_floats(D, A, h) and getattr(flat, Q_CRITIC_ATTR) == D + A

        class CCritic:                                          # usl_core.py C_Critic: the net sits in .c_net
            c_net = net
        assert torch.equal(Engine.pack_q_critic(CCritic()), want)
        assert getattr(flat.clone(), Q_CRITIC_ATTR, None) is None
    for why, bad in {"no Softplus": _seq(45, 64, tail=()), "Identity output": _seq(45, 64, tail=(nn.Identity(),)),
                     "beta 2": _seq(45, 64, tail=(nn.Softplus(beta=2),)), "threshold 10": _seq(45, 64, tail=(nn.Softplus(threshold=10),)),
                     "ReLU": _seq(45, 64, act=nn.ReLU), "two outputs": _seq(45, 64, out=2), "hidden 96": _seq(45, 96),
                     "unequal hidden": _seq(45, 64, h2=128),
                     "one hidden layer": nn.Sequential(nn.Linear(45, 64), nn.Tanh(), nn.Linear(64, 1), nn.Softplus())}.items():
        with pytest.raises(NotImplementedError):
            Engine.pack_q_critic(bad)
            pytest.fail(why)


# ---------------------------------------------------------------------------------------------------------------------
# device code and argument checks (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def usl_lib():
    from guardx_amd import build, _usl_native
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _usl_native.load()          # refuses a library whose build id is not the tree's


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles every kernel of the library without scratch memory and within the 168
    registers that 12 waves per workgroup leave a lane"""
    import subprocess
    from guardx_amd import build
    asm = tmp_path / "gx_usl.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_usl.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print("usl kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == 21 and max(scratch) == 0 and max(vgpr) <= 168


def test_sizes_and_bad_arguments_are_errors_not_crashes(usl_lib):
    from guardx_amd import _usl_native as n
    from guardx_amd.usl import policy_floats, q_floats
    lib = usl_lib
    for D, A in ((43, 2), (64, 8), (70, 10)):
        Dp = (D + 3) // 4 * 4
        for h in (64, 128, 192, 256):
            assert lib.gxu_params_floats(D, A, h) == policy_floats(D, A, h)
            assert lib.gxu_q_floats(D, A, h) == q_floats(D, A, h)
            assert lib.gxu_probe_work_floats(D, A, h) == Dp * h + h * h
            for hc in (64, 256):
                assert lib.gxu_work_floats(D, A, h, hc) == 2 * (Dp * h + h * h) + Dp * hc + hc * hc
    assert lib.gxu_params_floats(43, 2, 96) == -1 and lib.gxu_q_floats(0, 2, 64) == -1
    assert lib.gxu_q_floats(43, 3, 64) == -1 and lib.gxu_work_floats(43, 2, 64, 32) == -1
    assert lib.gxu_probe_work_floats(43, 18, 64) == -1
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxu_prepare(43, 2, 64, 64, None, fake, fake, None) == n.GXU_ERR_ARG
    assert lib.gxu_prepare(43, 2, 64, 96, fake, fake, fake, None) == n.GXU_ERR_UNSUPPORTED
    assert lib.gxu_prepare(9000, 2, 256, 256, fake, fake, fake, None) == n.GXU_ERR_UNSUPPORTED

    def probe(n_=4, D=43, A=2, hc=64, cp=fake, niter=1):
        return lib.gxu_correction_probe(n_, D, A, hc, cp, fake, fake, fake, 0.0, niter, 0.05, 1.0, fake, fake, fake, fake,
                                        fake, None)
    assert probe(cp=None) == n.GXU_ERR_ARG and probe(n_=-1) == n.GXU_ERR_ARG and probe(niter=-1) == n.GXU_ERR_ARG
    assert probe(hc=96) == n.GXU_ERR_UNSUPPORTED and probe(A=3) == n.GXU_ERR_UNSUPPORTED and probe(A=18) == n.GXU_ERR_UNSUPPORTED
    assert probe(n_=0) == n.GXU_OK

    def args(**over):
        a = n.GxuStepArgs()
        a.struct_size = C.sizeof(n.GxuStepArgs)
        a.N, a.D, a.A, a.hidden, a.c_hidden, a.T, a.t, a.niter = 4, 43, 2, 64, 64, 3, 1, 20
        for f, _ in n.GxuStepArgs._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.gxu_policy_step(None, None) == n.GXU_ERR_ARG
    assert lib.gxu_policy_step(C.byref(args(struct_size=8)), None) == n.GXU_ERR_ARG
    assert b"struct_size" in lib.gxu_last_error()
    for bad in (dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(niter=-1), dict(d_params=None), dict(d_c_params=None),
                dict(d_cost_in=None), dict(d_act_safe=None), dict(d_qc=None), dict(d_iters=None),
                dict(t=3, d_val_last=None), dict(t=0, d_obs0=None)):
        assert lib.gxu_policy_step(C.byref(args(**bad)), None) == n.GXU_ERR_ARG, bad
    for bad in (dict(hidden=96), dict(c_hidden=0), dict(A=3), dict(A=18), dict(D=9000, hidden=256, c_hidden=256)):
        assert lib.gxu_policy_step(C.byref(args(**bad)), None) == n.GXU_ERR_UNSUPPORTED, bad
    assert lib.gxu_policy_step(C.byref(args(N=0)), None) == n.GXU_OK          # N == 0: nothing to do


# ---------------------------------------------------------------------------------------------------------------------
# the float64 restatement against torch autograd, and the float32 update against it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["point64", "ant256", "saturated192", "threshold20", "zero-gradient"])
def test_analytic_gradient_equals_torch_autograd_in_float64(name):
    import test_gpu_usl as tg
    qm, obs, act, _ = tg.probe_inputs(name)
    obs, act = obs[:400], act[:400]
    r = usl64.QCritic(qm).grad(obs, act, 0.25)
    q, s = usl64.torch_autograd_s(qm, obs, act, 0.25)
    np.testing.assert_allclose(r['q'], q, rtol=1e-12, atol=1e-300)
    scale = np.abs(s).max() + 1e-300
    assert np.abs(r['s'] - s).max() <= 1e-11 * scale + 1e-25, np.abs(r['s'] - s).max()
    if name != "zero-gradient":
        assert scale > 1e-6
    else:
        assert (s == 0).all() and (r['s'] == 0).all()


def test_update32_against_the_float64_update():
    """update32 on exact float32 s within the float64 step's own bound (ds = 0: the roundings of the update alone), and
    its fixed points: s = 0 leaves a where it is (0 / 1e-8), the largest component moves by eta up to the 1e-8"""
    rng = np.random.default_rng(3)
    f = np.float32
    for A in (2, 8, 16):
        n = 20000
        s = (rng.normal(size=(n, A)) * rng.choice([1e-12, 1e-6, 1.0, 50.0], size=(n, 1))).astype(f)
        a = (rng.normal(size=(n, A)) * 0.7).astype(f)
        got = usl64.update32(a, s, 0.05)
        s64, a64 = s.astype(np.float64), a.astype(np.float64)
        den = np.abs(s64).max(-1, keepdims=True) + float(f(1e-8))
        want = a64 - float(f(0.05)) * s64 / den
        bound = 1.01 * usl64.U * (3 * float(f(0.05)) * np.abs(s64 / den) + np.abs(want) + np.abs(a64))
        assert (np.abs(got - want) <= bound).all()
    z = usl64.update32(np.array([[0.3, -0.2]], f), np.zeros((1, 2), f), 0.05)
    np.testing.assert_array_equal(z, np.array([[0.3, -0.2]], f))
    m = usl64.update32(np.array([[0.5, 0.5]], f), np.array([[2.0, -1.0]], f), 0.05)
    np.testing.assert_allclose(m, [[0.45, 0.525]], rtol=0, atol=1e-7)


# ---------------------------------------------------------------------------------------------------------------------
# USLBufferX in numpy (safe_rl_libX/usl/usl.py:26-159): the TRPO restatement plus act_safe, cost, qc and targetc
# ---------------------------------------------------------------------------------------------------------------------
class USLBufferNP(TRPOBufferNP):
    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95):
        super().__init__(env_num, max_ep_len, obs_dim, act_dim, gamma, lam)
        f = np.float32
        self.act_safe_buf = np.zeros((env_num, max_ep_len, act_dim), f)
        self.cost_buf, self.qc_buf = np.zeros((env_num, max_ep_len), f), np.zeros((env_num, max_ep_len), f)
        self.targetc_buf = np.zeros((env_num, max_ep_len), f)

    def store(self, obs, act, act_safe, rew, val, logp, mu, logstd, cost, qc):          # usl.py:50-69
        p = self.ptr[0]
        super().store(obs, act, rew, val, logp, mu, logstd)
        self.act_safe_buf[:, p, :] = act_safe
        self.cost_buf[:, p] = cost
        self.qc_buf[:, p] = qc

    def finish_path(self, last_val, done):                                               # usl.py:71-129
        f = np.float32
        if np.all(self.path_start_idx == 0) and np.all(self.ptr == self.max_ep_len):
            z = np.zeros((self.env_num, 1), f)
            qcs, costs = np.hstack((self.qc_buf, z)), np.hstack((self.cost_buf, z))
            self.targetc_buf = costs[:, :-1] + f(self.gamma) * qcs[:, 1:]
        else:
            for e in np.where(np.asarray(done) == 1)[0]:
                sl = slice(self.path_start_idx[e], self.ptr[e])
                qcs, costs = np.append(self.qc_buf[e, sl], 0).astype(f), np.append(self.cost_buf[e, sl], 0).astype(f)
                self.targetc_buf[e, sl] = costs[:-1] + f(self.gamma) * qcs[1:]
        super().finish_path(last_val, done)

    def get(self):                                                                       # usl.py:131-159
        data = super().get()
        N, T = self.env_num, self.max_ep_len
        data['act_safe'] = self.act_safe_buf.reshape(N * T, -1)
        data['cost'] = self.cost_buf.reshape(N * T)
        data['targetc'] = self.targetc_buf.reshape(N * T)
        return data


def usl_batch_np(g, gamma=0.99, lam=0.95):
    """the learner's collection loop (usl.py:478-553) over a recorded rollout_usl result `g` (numpy): store every step,
    finish_path with v = 0 for the envs done at that step, the closing finish_path of the time-out"""
    T, N = g['rew'].shape
    A = g['act'].shape[-1]
    buf = USLBufferNP(N, T, g['obs'].shape[-1], A, gamma, lam)
    logstd = np.broadcast_to(g['logstd'].reshape(1, A), (N, A))
    for t in range(T):
        buf.store(g['obs'][t], g['act'][t], g['act_safe'][t], g['rew'][t], g['val'][t], g['logp'][t], g['mu'][t], logstd,
                  g['cost'][t], g['qc'][t])
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
             qc=rng.random((T, N)).astype(f), logstd=np.linspace(-0.5, 0.1, A).astype(f),
             done=(rng.random((T, N)) < (0.0 if no_done else 0.2)).astype(f))
    if not no_done:
        g['done'][:, 0] = 0                                   # one env closed by the time-out alone
        g['done'][0, 1] = 1                                   # a one-step episode
        g['done'][T - 1, 2] = 1                               # done on the last step
    return g


@pytest.mark.parametrize("no_done", [False, True])
def test_usl_rollout_batch_against_the_buffer_restatement(no_done):
    """usl_rollout_batch on host tensors against USLBufferX.store / finish_path / get restated in numpy, on a synthetic
    rollout with paths that end mid-epoch (finish_path's per-env branch) and without (its batch branch)"""
    import torch
    from guardx_amd.rollout_buffer import usl_rollout_batch
    T, N, D, A = 30, 9, 5, 4
    g = _synthetic(T, N, D, A, 5, no_done)
    want = usl_batch_np(g)
    got = usl_rollout_batch({k: torch.from_numpy(v) for k, v in g.items()})
    assert set(got) == set(want) == {'obs', 'act', 'act_safe', 'ret', 'adv', 'logp', 'mu', 'logstd', 'cost', 'targetc'}
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=tol, atol=tol, err_msg=k)
    tc = got['targetc'].numpy().reshape(N, T)
    for e in range(N):
        for t in range(T):
            end = t == T - 1 or g['done'][t, e] > 0
            exp = g['cost'][t, e] + (0.0 if end else np.float32(0.99) * g['qc'][t + 1, e])
            assert abs(tc[e, t] - exp) <= 1e-6
    with pytest.raises(KeyError, match="qc"):
        usl_rollout_batch({k: torch.from_numpy(v) for k, v in g.items() if k != 'qc'})


# ---------------------------------------------------------------------------------------------------------------------
# sizing the GPU tests' probe inputs with the float64 checker alone
# ---------------------------------------------------------------------------------------------------------------------
def test_probe_inputs_are_sized():
    """On exactly the inputs of tests/test_gpu_usl.py (probe_inputs), with the float64 restatement alone: every stop
    reason occurs in at least 5 % of the rows of some case, at least half of all rows apply one update or more, and the
    edge rows of the single pass are at most 2 % in every case.  Observed with niter = 20 (share of stop 0 / 1 / 2, rows
    that moved, edge rows of the first pass):
        ant256         0.052 0.415 0.533   0.278   0.0007        below-87       0.921 0.079 0.000   0.921   0
        point64        0.278 0.099 0.623   0.429   0.0010        saturated192   0.174 0.180 0.646   0.435   0.0007
        threshold20    0.455 0.545 0.000   0.918   0             walker128      0.055 0.482 0.463   0.284   0
        zero-gradient  0.914 0.086 0.000   0.914   0
    About 12 500 of the 21 000 rows move at least once (0.60)."""
    import test_gpu_usl as tg
    best, moved_all, rows = np.zeros(3), 0, 0
    for name in sorted(tg.PROBE_CASES):
        qm, obs, act, delta = tg.probe_inputs(name)
        Q = usl64.QCritic(qm)
        one = Q.one_pass(obs, act, delta, tg.ETA, 1.0)
        edge = float(one['edge'].mean())
        it = Q.iterate(obs, act, delta, 20, tg.ETA, 1.0)
        shares = np.array([(it['stop'] == k).mean() for k in range(3)])
        moved = float((it['iters'] > 0).mean())
        print(f"usl sizing {name}: stop 0/1/2 {shares[0]:.3f} {shares[1]:.3f} {shares[2]:.3f}  moved {moved:.3f}  "
              f"edge {edge:.4f}  median q0 {np.median(one['q']):.3f}")
        assert edge <= tg.EDGE_CAP, (name, edge)
        assert np.isfinite(one['ds']).all() and np.isfinite(one['da_next']).all()
        best = np.maximum(best, shares)
        moved_all += int((it['iters'] > 0).sum())
        rows += len(obs)
    assert (best >= 0.05).all(), best
    assert moved_all >= 0.5 * rows, (moved_all, rows)


def test_multi_pass_inputs_are_sized():
    """On the rows of tests/test_gpu_usl.py's multi-pass tests (33 of each case from MULTI_ROW0[case], both gradient scales), with the
    float64 restatement alone: some row runs all 20 passes, at least two stop reasons occur, some row moves twice or
    more, the running sum moves such a row somewhere else than the memoryless step does (by far more than fp32
    resolves), no row is an edge row in any pass (the GPU tests cap them at 2 % of 33 rows or fewer: none), the first row runs all
    20 passes and a row that never moves is among the first 15."""
    import test_gpu_usl as tg
    for name in tg.MULTI_CASES:
        qm, obs, act, delta = tg.probe_inputs(name)
        n = max(tg.MULTI_ROWS)
        r0 = tg.MULTI_ROW0[name]
        obs, act = obs[r0:r0 + n], act[r0:r0 + n]
        Q = usl64.QCritic(qm)
        for gs in tg.MULTI_SCALES:
            it = Q.iterate(obs, act, delta, tg.MULTI_PASSES, tg.ETA, gs)
            a, acc, dacc, live, edges, gap = act.astype(np.float64), None, None, np.ones(n, bool), np.zeros(n, bool), 0.0
            for p in range(tg.MULTI_PASSES):
                r = Q.one_pass(obs, a, delta, tg.ETA, gs, acc=acc, dacc=dacc)
                edges |= live & r['edge']
                live &= r['stop'] < 0
                if p == 1 and live.any():
                    gap = np.abs(Q.one_pass(obs, a, delta, tg.ETA, gs)['a_next'] - r['a_next'])[live].max()
                a, acc, dacc = r['a_next'], r['acc'], r['dacc']
            np.testing.assert_array_equal(a, it['a_safe'])
            print(f"usl multi-pass sizing {name} gs={gs:g}: iters {np.bincount(it['iters'], minlength=21).tolist()}  "
                  f"stop {np.bincount(it['stop'], minlength=3).tolist()}  edge rows {int(edges.sum())}  "
                  f"second step: running sum against memoryless {gap:.2e}")
            assert it['iters'].max() == tg.MULTI_PASSES and len(set(it['stop'].tolist())) >= 2
            assert (it['iters'] >= 2).any() and gap > 1e-5
            assert not edges.any()
            # the first row runs every pass, so the tests on 1, 15, 16 and 17 rows carry a running sum as well, and a row
            # that never moves sits among the first 15
            assert it['iters'][0] == tg.MULTI_PASSES and (it['iters'][:min(tg.MULTI_ROWS[1:])] == 0).any()


@pytest.mark.parametrize("case", [0, 1, 2])
def test_rollout_inputs_are_sized(oracle, case):
    """the engine, networks and delta of tests/test_gpu_usl.py's rollout test on the CPU checker's engine, first step, with
    the float64 restatement alone: at least 45 % of the rows apply an update (the GPU test asks for 30 % over its whole
    trajectory) and almost no sampled action leaves the box"""
    import test_gpu_usl as tg
    from oracle import policy64
    from test_gpu_statewise import _cfg, COSTLY, SEED
    robot, h, hc, delta = tg.ROLLOUT_CASES[case]
    N = tg.ROLLOUT_N
    O = oracle.OracleEngine(_cfg(robot, N, seed=tg.ROLLOUT_CFG_SEED, **COSTLY), n_candidates=max(40000, 100 * N))
    obs = O.reset()
    ac, qm = tg.rollout_nets(obs.shape[1], O.na, h, hc)
    w = policy64.ActorCritic(ac).step(obs, SEED, np.arange(N), np.zeros(N, np.int64))
    act = w['act'].astype(np.float32)
    it = usl64.QCritic(qm).iterate(obs, act, delta, 20, 0.05, 1.0 / N)
    moved = float((it['iters'] > 0).mean())
    print(f"usl rollout sizing {robot} A={O.na} delta={delta}: moved {moved:.3f}, max a > 1 on {float((act.max(1) > 1).mean()):.3f}")
    assert moved >= 0.45 and (act.max(1) > 1).mean() < 0.1
