"""The host side of Engine.rollout_episode (the `*_one_episode` learners on the device path): the seventh library's
argument checks and device code (its build identity and ABI: tests/test_build_identity.py), and the batch helper's host-tensor path against a numpy
restatement of the one-episode buffer (safe_rl_libX/trpo_one_episode/trpo.py:24-132, cpo_one_episode/cpo.py:22-156)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from oracle.trpo_buffer_np import discount_cumsum


# ---------------------------------------------------------------------------------------------------------------------
# device code and argument checks (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ep_lib():
    from guardx_amd import build, _episode_native
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _episode_native.load()      # refuses a library whose build id is not the tree's


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles every kernel of the library (16 step kernels, the transpose, the two kernels
    of gxe_finish and its N == 0 kernel) without scratch memory and within the 168 registers that 12 waves per workgroup
    (3 on a SIMD, 512 / 3 rounded down) leave a lane"""
    import subprocess
    from guardx_amd import build
    asm = tmp_path / "gx_episode.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_episode.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    vgpr = [int(v) for v in re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text)]
    print("episode kernels:", len(scratch), "max vgpr", max(vgpr))
    assert len(scratch) == 20 and max(scratch) == 0 and max(vgpr) <= 168


def test_sizes_and_bad_arguments_are_errors_not_crashes(ep_lib):
    from guardx_amd import _episode_native as n
    from guardx_amd.episode import policy_floats
    from guardx_amd.critic import critic_floats
    lib = ep_lib
    for D, A in ((43, 2), (64, 8), (70, 10)):
        for h in (64, 128, 192, 256):
            assert lib.gxe_params_floats(D, A, h) == policy_floats(D, A, h)
            assert lib.gxe_vc_floats(D, h) == critic_floats(D, h)
            for hc in (64, 256):
                Dp = (D + 3) // 4 * 4
                assert lib.gxe_work_floats(D, A, h, hc) == 2 * (Dp * h + h * h) + Dp * hc + hc * hc
    assert lib.gxe_params_floats(43, 2, 96) == -1 and lib.gxe_params_floats(0, 2, 64) == -1
    assert lib.gxe_params_floats(43, 3, 64) == -1 and lib.gxe_work_floats(43, 2, 64, 32) == -1
    assert lib.gxe_vc_floats(43, 96) == -1 and lib.gxe_vc_floats(0, 64) == -1
    assert lib.gxe_finish_work_floats(-1, 4) == -1 and lib.gxe_finish_work_floats(4, 0) == -1
    assert lib.gxe_finish_work_floats(300, 5) == 4 * 300 * 5 + 4 * 300 + 300 + 2
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxe_prepare(43, 2, 64, 64, None, fake, fake, None) == n.GXE_ERR_ARG
    assert lib.gxe_prepare(43, 2, 64, 96, fake, fake, fake, None) == n.GXE_ERR_UNSUPPORTED
    assert lib.gxe_prepare(5000, 2, 256, 256, fake, fake, fake, None) == n.GXE_ERR_UNSUPPORTED

    def probe(n_=4, D=43, A=2, h=64, hc=64, has_vc=1, ptrs=None):
        p = [fake] * 7 if ptrs is None else ptrs
        return lib.gxe_tail_probe(n_, D, A, h, hc, has_vc, *p, None)
    assert probe(n_=-1) == n.GXE_ERR_ARG
    assert probe(ptrs=[fake, fake, fake, None, fake, fake, fake]) == n.GXE_ERR_ARG
    assert probe(ptrs=[fake] * 6 + [None]) == n.GXE_ERR_ARG                    # has_vc needs d_vc_last
    assert probe(h=96) == n.GXE_ERR_UNSUPPORTED and probe(A=3) == n.GXE_ERR_UNSUPPORTED
    assert probe(n_=0) == n.GXE_OK and probe(n_=0, has_vc=0, ptrs=[fake] * 6 + [None]) == n.GXE_OK

    def finish(N=4, T=3, D=5, A=2, ptrs=None):
        p = [fake] * 21 if ptrs is None else ptrs
        return lib.gxe_finish(N, T, D, A, 0.99, 0.95, *p, None)
    assert finish(N=-1) == n.GXE_ERR_ARG and finish(T=0) == n.GXE_ERR_ARG and finish(D=0) == n.GXE_ERR_ARG
    assert finish(N=1 << 20, T=1 << 12) == n.GXE_ERR_UNSUPPORTED
    for i in (0, 1, 7, 11, 12, 17, 20):
        p = [fake] * 21
        p[i] = None
        assert finish(ptrs=p) == n.GXE_ERR_ARG, i
    p = [fake] * 21
    p[8] = None                                                                # d_cost alone missing of the cost channel
    assert finish(ptrs=p) == n.GXE_ERR_ARG and b"cost channel" in lib.gxe_last_error()

    def args(**over):
        a = n.GxeStepArgs()
        a.struct_size = C.sizeof(n.GxeStepArgs)
        a.N, a.D, a.A, a.hidden, a.vc_hidden, a.has_vc, a.T, a.t = 4, 43, 2, 64, 64, 1, 3, 1
        for f, _ in n.GxeStepArgs._fields_:
            if f.startswith("d_"):
                setattr(a, f, fake)
        for k, v in over.items():
            setattr(a, k, v)
        return a
    assert lib.gxe_policy_step(None, None) == n.GXE_ERR_ARG
    assert lib.gxe_policy_step(C.byref(args(struct_size=8)), None) == n.GXE_ERR_ARG
    assert b"struct_size" in lib.gxe_last_error()
    assert lib.gxe_policy_step(C.byref(args(t_base=-1)), None) == n.GXE_ERR_ARG
    assert b"t_base >= 0" in lib.gxe_last_error()
    for bad in (dict(N=-1), dict(t=-1), dict(t=4), dict(T=0), dict(d_params=None), dict(d_vc_params=None),
                dict(d_work=None), dict(d_first_done=None), dict(d_ep_ret=None), dict(d_ep_cost=None), dict(d_ep_len=None),
                dict(d_cost_in=None), dict(d_obs_rd=None), dict(d_vc=None), dict(d_act=None), dict(t=3, d_val_last=None),
                dict(t=3, d_vc_last=None), dict(t=0, d_obs0=None)):
        assert lib.gxe_policy_step(C.byref(args(**bad)), None) == n.GXE_ERR_ARG, bad
    for bad in (dict(hidden=96), dict(vc_hidden=0), dict(hidden=320), dict(A=3), dict(A=18),
                dict(D=5000, hidden=256, vc_hidden=256)):
        assert lib.gxe_policy_step(C.byref(args(**bad)), None) == n.GXE_ERR_UNSUPPORTED, bad
    assert lib.gxe_policy_step(C.byref(args(N=0)), None) == n.GXE_OK          # N == 0: nothing to do
    assert lib.gxe_policy_step(C.byref(args(N=0, has_vc=0, d_vc=None, d_vc_last=None)), None) == n.GXE_OK
    assert lib.gxe_policy_step(C.byref(args(t=0, d_cost_in=None, d_obs_rd=None, N=0)), None) == n.GXE_OK


# ---------------------------------------------------------------------------------------------------------------------
# the one-episode buffer in numpy (trpo_one_episode/trpo.py:24-132; the cost channel of cpo_one_episode/cpo.py:22-156)
# ---------------------------------------------------------------------------------------------------------------------
class OneEpisodeBufferNP:
    """store / finish_path(first_done_idx) / get as the reference runs them, buffers kept from one epoch to the next the way
    it keeps them: valid_buf is cleared by get(), adv_buf / adc_buf (and the returns) are not"""

    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95, cost=False):
        f = np.float32
        N, T = env_num, max_ep_len
        self.obs_buf, self.act_buf = np.zeros((N, T, obs_dim), f), np.zeros((N, T, act_dim), f)
        self.mu_buf, self.logstd_buf = np.zeros((N, T, act_dim), f), np.zeros((N, T, act_dim), f)
        self.rew_buf, self.val_buf, self.logp_buf = np.zeros((N, T), f), np.zeros((N, T), f), np.zeros((N, T), f)
        self.adv_buf, self.ret_buf, self.valid_buf = np.zeros((N, T), f), np.zeros((N, T), f), np.zeros((N, T), f)
        self.cost = cost
        if cost:
            self.cost_buf, self.cost_val_buf = np.zeros((N, T), f), np.zeros((N, T), f)
            self.adc_buf, self.cost_ret_buf = np.zeros((N, T), f), np.zeros((N, T), f)
        self.gamma, self.lam, self.ptr, self.N, self.T = gamma, lam, 0, N, T

    def store(self, obs, act, rew, val, logp, mu, logstd, cost=None, cost_val=None):
        p = self.ptr
        assert p < self.T
        self.obs_buf[:, p], self.act_buf[:, p], self.mu_buf[:, p], self.logstd_buf[:, p] = obs, act, mu, logstd
        self.rew_buf[:, p], self.val_buf[:, p], self.logp_buf[:, p] = rew, val, logp
        if self.cost:
            self.cost_buf[:, p], self.cost_val_buf[:, p] = cost, cost_val
        self.ptr += 1

    def _path(self, rew, val, last, sl):
        rews, vals = np.append(rew[sl], last), np.append(val[sl], last)
        deltas = rews[:-1] + self.gamma * vals[1:] - vals[:-1]
        return (discount_cumsum(deltas, self.gamma * self.lam).astype(np.float32),
                discount_cumsum(rews, self.gamma)[:-1].astype(np.float32))

    def finish_path(self, last_val, first_done_idx, last_cost_val=None):
        for e in range(self.N):
            sl = slice(0, int(first_done_idx[e]))
            self.adv_buf[e, sl], self.ret_buf[e, sl] = self._path(self.rew_buf[e], self.val_buf[e], np.float32(last_val[e]), sl)
            if self.cost:
                self.adc_buf[e, sl], self.cost_ret_buf[e, sl] = self._path(self.cost_buf[e], self.cost_val_buf[e],
                                                                           np.float32(last_cost_val[e]), sl)
            self.valid_buf[e, sl] = 1

    def get(self):
        assert self.ptr == self.T
        self.ptr = 0
        N, T = self.N, self.T

        def stats(x):                                           # mpi_statistics_scalar, one process
            x = np.array(x, dtype=np.float32)
            mean = np.sum(x) / len(x)
            return mean, np.sqrt(np.sum((x - mean) ** 2) / len(x))
        self.adv_buf = np.asarray([(r - stats(r)[0]) / stats(r)[1] for r in self.adv_buf], np.float32)
        valid = np.where(self.valid_buf.reshape(N * T) == 1)
        flat = lambda x: x.reshape(N * T, *x.shape[2:])[valid]   # noqa: E731
        data = dict(obs=flat(self.obs_buf), act=flat(self.act_buf), ret=flat(self.ret_buf), adv=flat(self.adv_buf),
                    logp=flat(self.logp_buf), mu=flat(self.mu_buf), logstd=flat(self.logstd_buf))
        if self.cost:
            self.adc_buf = np.asarray([r - stats(r)[0] for r in self.adc_buf], np.float32)    # centred only
            data.update(cost_ret=flat(self.cost_ret_buf), adc=flat(self.adc_buf))
        self.valid_buf = np.zeros((N, T), np.float32)
        return data


def first_done_np(done):
    """(T, N) done -> the 1-based index of the first step with done per env, 0 where there is none"""
    any_done = (done > 0).any(0)
    return np.where(any_done, (done > 0).argmax(0) + 1, 0).astype(np.int32)


def one_episode_batch_np(g, buf=None, gamma=0.99, lam=0.95):
    """the learner's epoch (trpo.py:450-545, cpo.py:619-708) over a recorded rollout_episode result `g` (numpy): store every
    step, one finish_path with first_done_idx and a bootstrap for the envs that never finished and whose last
    observation is finite, get"""
    T, N = g['rew'].shape
    A = g['act'].shape[-1]
    cost = 'vc' in g
    buf = buf or OneEpisodeBufferNP(N, T, g['obs'].shape[-1], A, gamma, lam, cost)
    logstd = np.broadcast_to(g['logstd'].reshape(1, A), (N, A))
    for t in range(T):
        buf.store(g['obs'][t], g['act'][t], g['rew'][t], g['val'][t], g['logp'][t], g['mu'][t], logstd,
                  *((g['cost'][t], g['vc'][t]) if cost else ()))
    fd = first_done_np(g['done'])
    boot = (fd == 0) & np.isfinite(g['obs_last']).all(1)
    z = np.float32(0)
    buf.finish_path(np.where(boot, g['val_last'], z), np.where(fd > 0, fd, T),
                    np.where(boot, g['vc_last'], z) if cost else None)
    return buf.get(), buf


T_, N_, D_, A_ = 12, 8, 5, 4


def _synthetic(seed, cost, first=(0, 1, 5, T_, 3, 0, 8, 0)):
    """a rollout_episode result as numpy: env 1 is done at every step, env 3 at the last step only, envs 0 / 5 / 7 never
    (the bootstrap), env 5 with a non-finite obs_last (so the tail gave it val_last = vc_last = 0); envs 2 / 4 / 6 finish
    inside and their done returns to 0 afterwards"""
    rng = np.random.default_rng(seed)
    f = np.float32
    T, N, D, A = T_, N_, D_, A_
    r = lambda *s: rng.normal(size=s).astype(f)   # noqa: E731
    g = dict(obs=r(T, N, D), act=r(T, N, A), mu=r(T, N, A), logp=r(T, N), rew=r(T, N), val=r(T, N),
             cost=rng.random((T, N)).astype(f), logstd=np.linspace(-0.5, 0.1, A).astype(f), obs_last=r(N, D), val_last=r(N),
             done=np.zeros((T, N), f))
    for e, k in enumerate(first):
        if k:
            g['done'][k - 1, e] = 1
    if first[1] == 1:
        g['done'][:, 1] = 1
    g['done'][7, 2] = 1                                          # a second done of env 2: not its first
    g['obs_last'][5, 2] = np.inf
    g['obs_last'][5, 3] = np.nan
    g['val_last'][5] = 0
    g['first_done'] = first_done_np(g['done'])
    assert list(g['first_done']) == list(first)
    if cost:
        g['vc'], g['vc_last'] = r(T, N), r(N)
        g['vc_last'][5] = 0
    return g


def _torch_out(g):
    import torch
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items()}
    out['t0'] = 0
    return out


def _close(got, want, keys):
    for k in keys:
        # the tolerances of tests/test_rollout_buffer.py for the same recursion: returns 1e-6, normalised / centred
        # advantages 2e-5 (the fp32 order of mean and deviation)
        tol = 2e-5 if k in ('adv', 'adc') else 1e-6
        np.testing.assert_allclose(got[k].numpy(), want[k], rtol=tol, atol=tol, err_msg=k)


@pytest.mark.parametrize("cost", [False, True])
def test_episode_rollout_batch_against_the_buffer_restatement(cost):
    import torch
    from guardx_amd.rollout_buffer import episode_rollout_batch
    g = _synthetic(5, cost)
    want, _ = one_episode_batch_np(g)
    got = episode_rollout_batch(_torch_out(g))
    L = np.where(g['first_done'] > 0, g['first_done'], T_)
    assert got.pop('n_valid') == int(L.sum()) == len(want['ret']) == 12 + 1 + 5 + 12 + 3 + 12 + 8 + 12
    assert set(got) == set(want) == {'obs', 'act', 'ret', 'adv', 'logp', 'mu', 'logstd'} | ({'cost_ret', 'adc'} if cost else set())
    # the row order: env-major, each env's prefix [0, L)
    rows = [(e, t) for e in range(N_) for t in range(L[e])]
    for k in ('obs', 'act', 'logp', 'mu'):
        np.testing.assert_array_equal(got[k].numpy(), want[k], err_msg=k)
        np.testing.assert_array_equal(got[k].numpy(), np.stack([g[k][t, e] for e, t in rows]), err_msg=k)
    np.testing.assert_array_equal(got['logstd'].numpy(), want['logstd'])
    _close(got, want, ('ret', 'adv') + (('cost_ret', 'adc') if cost else ()))
    # env 5 (non-finite obs_last) and the finished envs close with 0, envs 0 and 7 with val_last: hand-worked last rows
    off = np.concatenate([[0], np.cumsum(L)])
    for e in range(N_):
        last = got['ret'].numpy()[off[e + 1] - 1]
        boot = g['val_last'][e] if g['first_done'][e] == 0 else 0.0
        np.testing.assert_allclose(last, g['rew'][L[e] - 1, e] + 0.99 * boot, rtol=1e-6, atol=1e-6)
    # t0 != 0: not a whole episode
    out = _torch_out(g)
    out['t0'] = 6
    with pytest.raises(ValueError, match="t0"):
        episode_rollout_batch(out)
    with pytest.raises(KeyError, match="first_done"):
        episode_rollout_batch({k: v for k, v in _torch_out(g).items() if k != 'first_done'})
    assert isinstance(got['adv'], torch.Tensor)


def test_the_reference_keeps_stale_advantages_past_first_done():
    """The reference never re-zeroes adv_buf / adc_buf: in its second epoch the entries past first_done hold the first
    epoch's normalised values and enter mean and deviation.  The device definition takes them as 0 (the first epoch).
    So the two agree in the second epoch on every env whose path fills the row (L == T) and differ, in adv and adc
    alone, on every env that finished before T."""
    from guardx_amd.rollout_buffer import episode_rollout_batch
    g1 = _synthetic(5, True)
    g2 = _synthetic(6, True, first=(4, 0, 5, T_, 0, 2, 0, 9))
    _, buf = one_episode_batch_np(g1)
    stale, _ = one_episode_batch_np(g2, buf)                      # the reference's second epoch
    fresh, _ = one_episode_batch_np(g2)                           # a first epoch on the same data
    got = episode_rollout_batch(_torch_out(g2))
    got.pop('n_valid')
    _close(got, fresh, ('ret', 'adv', 'cost_ret', 'adc'))
    _close(got, stale, ('ret', 'cost_ret'))
    L = np.where(g2['first_done'] > 0, g2['first_done'], T_)
    off = np.concatenate([[0], np.cumsum(L)])
    for e in range(N_):
        sl = slice(off[e], off[e + 1])
        for k in ('adv', 'adc'):
            same = np.allclose(got[k].numpy()[sl], stale[k][sl], rtol=2e-5, atol=2e-5)
            assert same == (L[e] == T_), (e, k)
