"""The host side of Engine.rollout_statewise (SCPO on the device path): packing the Softplus-headed cost critic, the
third library's device code and argument checks (its build identity and ABI: tests/test_build_identity.py), the M recurrence against SCPO's loop as written and as intended, and the numpy
restatement of SCPOBufferX the device batch helper is checked against (tests/test_gpu_statewise.py)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle.trpo_buffer_np import TRPOBufferNP, discount_cumsum



def _seq(D, h, tail=()):
    import torch.nn as nn
    return nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, 1), *tail)


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_critic_softplus():
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    from guardx_amd.statewise import critic_output
    net = _seq(44, 128, (nn.Softplus(),))
    flat = Engine.pack_critic(net, output='softplus')
    lin = [m for m in net if isinstance(m, nn.Linear)]
    want = torch.cat([t.detach().reshape(-1) for m in lin for t in (m.weight, m.bias)])
    assert torch.equal(flat, want) and critic_output(flat) == 'softplus'

    class VC:                      # scpo_core.py MLPMaxCostCritic: the net sits in .v_net
        v_net = net
    assert torch.equal(Engine.pack_critic(VC(), output='softplus'), want)
    # today's behaviour pinned: the default call refuses a Softplus net, and accepts / declares a linear one
    with pytest.raises(NotImplementedError, match="linear output only"):
        Engine.pack_critic(net)
    assert critic_output(Engine.pack_critic(_seq(44, 64))) == 'identity'
    assert critic_output(flat.clone()) is None
    for why, bad in {"no output activation": _seq(44, 64), "Tanh output": _seq(44, 64, (nn.Tanh(),)),
                     "ReLU output": _seq(44, 64, (nn.ReLU(),)), "Sigmoid output": _seq(44, 64, (nn.Sigmoid(),)),
                     "beta 2": _seq(44, 64, (nn.Softplus(beta=2),)), "threshold 10": _seq(44, 64, (nn.Softplus(threshold=10),)),
                     "two Softplus": _seq(44, 64, (nn.Softplus(), nn.Softplus())),
                     "width 96": _seq(44, 96, (nn.Softplus(),))}.items():
        with pytest.raises(NotImplementedError):
            Engine.pack_critic(bad, output='softplus')
            pytest.fail(why)
    with pytest.raises(ValueError):
        Engine.pack_critic(net, output='relu')


def test_scpo_actor_critic_packs_on_the_augmented_width():
    from guardx_amd import Engine
    from guardx_amd.statewise import policy_floats
    from test_policy64 import make_ac
    for D, A, h in ((43, 2, 64), (64, 8, 256)):
        assert Engine.pack_actor_critic(make_ac(D + 1, A, h)).numel() == policy_floats(D + 1, A, h) \
            == Engine._policy_floats(D + 1, A, h)


# ---------------------------------------------------------------------------------------------------------------------
# device code and argument checks (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sw_lib():
    from guardx_amd import build, _statewise_native
    build.build()
    return _statewise_native.load()


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles every kernel of the library (16 step kernels, the probe kernel, the transpose)
    without scratch memory and within the 256 registers that 6 waves per workgroup (at most 2 on a SIMD) leave a lane"""
    import subprocess
    from guardx_amd import build
    asm = tmp_path / "gx_statewise.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_statewise.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print("statewise kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == 18 and max(scratch) == 0 and max(vgpr) <= 256


def test_sizes_and_bad_arguments_are_errors_not_crashes(sw_lib):
    from guardx_amd import _statewise_native as n
    from guardx_amd.statewise import policy_floats
    lib = sw_lib
    for Da, A in ((44, 2), (65, 8), (71, 10)):
        for h in (64, 128, 192, 256):
            assert lib.gxs_params_floats(Da, A, h) == policy_floats(Da, A, h)
            for hc in (64, 256):
                Dp = (Da + 3) // 4 * 4
                assert lib.gxs_work_floats(Da, A, h, hc) == 2 * (Dp * h + h * h) + Dp * hc + hc * hc
    assert lib.gxs_params_floats(44, 2, 96) == -1 and lib.gxs_params_floats(1, 2, 64) == -1
    assert lib.gxs_params_floats(44, 3, 64) == -1 and lib.gxs_work_floats(44, 2, 64, 32) == -1
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxs_prepare(44, 2, 64, 64, None, fake, fake, None) == n.GXS_ERR_ARG
    assert lib.gxs_prepare(44, 2, 64, 96, fake, fake, fake, None) == n.GXS_ERR_UNSUPPORTED
    assert lib.gxs_prepare(5000, 2, 256, 256, fake, fake, fake, None) == n.GXS_ERR_UNSUPPORTED
    assert lib.gxs_softplus_probe(4, None, fake, None) == n.GXS_ERR_ARG
    assert lib.gxs_softplus_probe(-1, fake, fake, None) == n.GXS_ERR_ARG
    assert lib.gxs_softplus_probe(0, fake, fake, None) == n.GXS_OK

    def args(**over):
        a = n.GxsStepArgs()
        a.struct_size = C.sizeof(n.GxsStepArgs)
        a.N, a.D_aug, a.A, a.hidden, a.vc_hidden, a.T, a.t = 4, 44, 2, 64, 64, 3, 1
        for f, _ in n.GxsStepArgs._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.gxs_policy_step(None, None) == n.GXS_ERR_ARG
    assert lib.gxs_policy_step(C.byref(args(struct_size=8)), None) == n.GXS_ERR_ARG
    assert b"struct_size" in lib.gxs_last_error()
    for bad in (dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(d_params=None), dict(d_M=None), dict(d_cost_in=None),
                dict(d_act=None), dict(t=3, d_vc_last=None), dict(t=0, d_obs0=None)):
        assert lib.gxs_policy_step(C.byref(args(**bad)), None) == n.GXS_ERR_ARG, bad
    for bad in (dict(hidden=96), dict(vc_hidden=0), dict(A=3), dict(A=18), dict(D_aug=5000, hidden=256, vc_hidden=256)):
        assert lib.gxs_policy_step(C.byref(args(**bad)), None) == n.GXS_ERR_UNSUPPORTED, bad
    assert lib.gxs_policy_step(C.byref(args(N=0)), None) == n.GXS_OK          # N == 0: nothing to do
    assert lib.gxs_policy_step(C.byref(args(t=0, d_cost_in=None, d_obs_rd=None, N=0)), None) == n.GXS_OK


# ---------------------------------------------------------------------------------------------------------------------
# the M recurrence against SCPO's loop
# ---------------------------------------------------------------------------------------------------------------------
def _scpo_loop(cost, done, aliased):
    """safe_rl_libX/scpo/scpo.py:644-654 and 713-715, line for line, over recorded costs and dones.  aliased=True: as
    written (`cost_increase` and `M_next` ARE info['cost']); False: with copies (what the names say).  Returns what
    buf.store receives as cost_increase, and M_next, per step."""
    import torch
    T, N = cost.shape
    M = torch.zeros(N, dtype=torch.float32)
    first_step = np.ones(N)
    stored, m_next = [], []
    for t in range(T):
        info = {'cost': torch.from_numpy(cost[t].copy())}
        d = done[t]
        cost_increase = info['cost'] if aliased else info['cost'].clone()
        M_next = info['cost'] if aliased else info['cost'].clone()
        for i in range(N):
            if first_step[i]:
                first_step[i] = False
            else:
                cost_increase[i] = max(info['cost'][i] - M[i], 0)
                M_next[i] = M[i] + cost_increase[i]
        stored.append(cost_increase.clone().numpy())
        m_next.append(M_next.clone().numpy().reshape(N))
        M = M_next
        if d.any():                                   # scpo.py:713-715
            idx = np.where(d == 1)
            M = M.clone()                             # (M_next aliases info['cost'], recorded above)
            M[idx] = torch.zeros(len(idx[0]))
            first_step[idx] = np.ones(len(idx[0]))
    return np.array(stored), np.array(m_next)


def test_m_recurrence_against_scpo_as_intended_and_as_written():
    from test_gpu_statewise import m_recurrence
    rng = np.random.default_rng(3)
    T, N = 40, 37
    cost = (rng.random((T, N)) * (rng.random((T, N)) < 0.6)).astype(np.float32)
    done = (rng.random((T, N)) < 0.15).astype(np.float32)
    done[0, :5] = 1          # done on the first step
    done[3:6, 7] = 1         # consecutive dones
    done[:, 11] = 0          # never done
    cost[:, 12] = 0          # never a cost
    inc, Mn, M_in, M, first = m_recurrence(cost, done, np.zeros(N, np.float32), np.ones(N, bool))
    want_inc, want_M = _scpo_loop(cost, done, aliased=False)
    np.testing.assert_array_equal(inc, want_inc)            # the increment SCPO defines
    np.testing.assert_array_equal(Mn, want_M)
    as_written, as_written_M = _scpo_loop(cost, done, aliased=True)
    np.testing.assert_array_equal(Mn, as_written)           # what the reference stores as "cost_increase": M_next
    np.testing.assert_array_equal(Mn, as_written_M)
    assert (inc != Mn).any()
    # the issue's three lines
    i3, m3, _, _, _ = m_recurrence(np.array([[0.3, 0.4, 0.0], [0.5, 0.2, 0.0]], np.float32), np.zeros((2, 3), np.float32),
                                   np.zeros(3, np.float32), np.ones(3, bool))
    np.testing.assert_array_equal(m3[1], np.array([0.5, 0.4, 0.0], np.float32))
    np.testing.assert_array_equal(i3[1], np.array([0.5, 0.2, 0.0], np.float32) - np.array([0.3, 0.2, 0.0], np.float32))
    # M as the networks see it: 0 after a done, the running maximum within an episode
    np.testing.assert_array_equal(M_in[1:][done > 0], 0)
    np.testing.assert_array_equal(M_in[1:, 11], np.maximum.accumulate(cost[:, 11]))
    # continuation: two calls equal one
    a = m_recurrence(cost[:17], done[:17], np.zeros(N, np.float32), np.ones(N, bool))
    b = m_recurrence(cost[17:], done[17:], a[3], a[4])
    np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), inc)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), Mn)


# ---------------------------------------------------------------------------------------------------------------------
# SCPOBufferX in numpy (safe_rl_libX/scpo/scpo.py:30-175): the TRPO restatement plus the cost channel with cgamma / clam
# ---------------------------------------------------------------------------------------------------------------------
class SCPOBufferNP(TRPOBufferNP):
    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95, cgamma=1., clam=0.95):
        super().__init__(env_num, max_ep_len, obs_dim, act_dim, gamma, lam)
        f = np.float32
        self.cost_buf, self.cost_ret_buf = np.zeros((env_num, max_ep_len), f), np.zeros((env_num, max_ep_len), f)
        self.cost_val_buf, self.adc_buf = np.zeros((env_num, max_ep_len), f), np.zeros((env_num, max_ep_len), f)
        self.cgamma, self.clam = cgamma, clam                              # scpo.py:52

    def store(self, obs, act, rew, val, logp, cost, cost_val, mu, logstd):   # scpo.py:58-76
        p = self.ptr[0]
        super().store(obs, act, rew, val, logp, mu, logstd)
        self.cost_buf[:, p] = cost
        self.cost_val_buf[:, p] = cost_val

    def finish_path(self, last_val, last_cost_val, done):                    # scpo.py:78-146
        last_cost_val = np.asarray(last_cost_val, np.float32).reshape(-1)
        if np.all(self.path_start_idx == 0) and np.all(self.ptr == self.max_ep_len):
            lc = last_cost_val[:, None]
            costs = np.hstack((self.cost_buf, lc))
            cvals = np.hstack((self.cost_val_buf, lc))
            deltas = costs[:, :-1] + np.float32(self.cgamma) * cvals[:, 1:] - cvals[:, :-1]
            self.adc_buf = np.asarray([discount_cumsum(r, self.cgamma * self.clam) for r in deltas]).astype(np.float32)
            self.cost_ret_buf = np.asarray([discount_cumsum(r, self.cgamma) for r in costs])[:, :-1].astype(np.float32)
        else:
            for e in np.where(np.asarray(done) == 1)[0]:
                sl = slice(self.path_start_idx[e], self.ptr[e])
                costs = np.append(self.cost_buf[e, sl], last_cost_val[e])
                cvals = np.append(self.cost_val_buf[e, sl], last_cost_val[e])
                deltas = costs[:-1] + self.cgamma * cvals[1:] - cvals[:-1]
                self.adc_buf[e, sl] = discount_cumsum(deltas, self.cgamma * self.clam).astype(np.float32)
                self.cost_ret_buf[e, sl] = discount_cumsum(costs, self.cgamma)[:-1].astype(np.float32)
        super().finish_path(last_val, done)                                   # (advances path_start_idx)

    def get(self):                                                            # scpo.py:148-175
        data = super().get()
        adc = np.array(self.adc_buf, dtype=np.float32)
        self.adc_buf = adc - (adc.sum(1, keepdims=True) / adc.shape[1])       # centred, not scaled
        N, T = self.env_num, self.max_ep_len
        data['cost_ret'] = self.cost_ret_buf.reshape(N * T)
        data['adc'] = self.adc_buf.reshape(N * T)
        return data


def scpo_batch_np(g, cost_signal, gamma=0.99, lam=0.95, cgamma=1.0, clam=0.95):
    """SCPO's collection loop (scpo.py:640-720) over a recorded rollout_statewise result `g` (numpy): store every step,
    finish_path with v = vc = 0 for the envs done at that step, the closing finish_path of the time-out."""
    T, N = g['rew'].shape
    A = g['act'].shape[-1]
    buf = SCPOBufferNP(N, T, g['obs'].shape[-1], A, gamma, lam, cgamma, clam)
    stored = g['cost_inc'] if cost_signal == 'increment' else g['M']
    logstd = np.broadcast_to(g['logstd'].reshape(1, A), (N, A))
    for t in range(T):
        buf.store(g['obs'][t], g['act'][t], g['rew'][t], g['val'][t], g['logp'][t], stored[t], g['vc'][t], g['mu'][t], logstd)
        if t + 1 == T:
            buf.finish_path(np.zeros(N, np.float32), np.zeros(N, np.float32), np.ones(N))
        elif g['done'][t].any():
            buf.finish_path(np.zeros(N, np.float32), np.zeros(N, np.float32), g['done'][t])
    return buf.get()


def test_scpo_buffer_restatement_paths():
    """the restatement itself: per env, every episode segment is its own discounted sum (cost channel undiscounted,
    lambda 0.95), whichever of finish_path's two branches closed it"""
    rng = np.random.default_rng(5)
    T, N, Da, A = 30, 9, 5, 2
    g = dict(obs=rng.normal(size=(T, N, Da)).astype(np.float32), act=rng.normal(size=(T, N, A)).astype(np.float32),
             mu=rng.normal(size=(T, N, A)).astype(np.float32), logp=rng.normal(size=(T, N)).astype(np.float32),
             rew=rng.normal(size=(T, N)).astype(np.float32), val=rng.normal(size=(T, N)).astype(np.float32),
             vc=rng.random((T, N)).astype(np.float32), cost_inc=rng.random((T, N)).astype(np.float32),
             M=rng.random((T, N)).astype(np.float32), logstd=np.array([-0.5, 0.1], np.float32),
             done=(rng.random((T, N)) < 0.2).astype(np.float32))
    g['done'][:, 0] = 0                                   # one env closed by the time-out alone
    for signal, key in (('increment', 'cost_inc'), ('reference', 'M')):
        b = scpo_batch_np(g, signal)
        cost_ret, adc = b['cost_ret'].reshape(N, T), b['adc'].reshape(N, T)
        for e in range(N):
            ends = [t for t in range(T) if g['done'][t, e] > 0 or t == T - 1]
            start, raw = 0, np.zeros(T)
            for end in ends:
                c, v = g[key][start:end + 1, e].astype(np.float64), np.append(g['vc'][start:end + 1, e], 0.0).astype(np.float64)
                np.testing.assert_allclose(cost_ret[e, start:end + 1], np.cumsum(c[::-1])[::-1], rtol=1e-5, atol=1e-5)
                delta = c + v[1:] - v[:-1]
                raw[start:end + 1] = [sum(delta[j] * 0.95 ** (j - i) for j in range(i, len(delta))) for i in range(len(delta))]
                start = end + 1
            np.testing.assert_allclose(adc[e], raw - raw.mean(), rtol=1e-4, atol=1e-4)
        assert b['obs'].shape == (N * T, Da) and b['logstd'].shape == (N * T, A)
        np.testing.assert_array_equal(b['obs'].reshape(N, T, Da)[3, 7], g['obs'][7, 3])
