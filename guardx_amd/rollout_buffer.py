"""Device-resident rollout buffer with GAE-lambda: the `TRPOBufferX` of
safe_rl_libX/trpo/trpo.py:24-146 with the same attribute names and methods
(`store`, `finish_path`, `get`), but `finish_path` and the advantage normalisation
run as HIP kernels on the env's stream -- no `.cpu()`, no per-env Python/scipy loop
when some environments finish mid-epoch (trpo.py:101-119), no host round trip in `get`
(trpo.py:131-135).  SURVEY.md row f1.
"""
import ctypes as C

import torch

from . import _native


class DeviceRolloutBuffer:
    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95, device=None):
        obs_dim = int(obs_dim[0]) if hasattr(obs_dim, '__len__') else int(obs_dim)
        act_dim = int(act_dim[0]) if hasattr(act_dim, '__len__') else int(act_dim)
        self.device = torch.device(device if device is not None else 'cuda')
        z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=self.device)   # noqa: E731
        N, T = int(env_num), int(max_ep_len)
        self.obs_buf, self.act_buf = z(N, T, obs_dim), z(N, T, act_dim)
        self.adv_buf, self.rew_buf, self.ret_buf = z(N, T), z(N, T), z(N, T)
        self.val_buf, self.logp_buf = z(N, T), z(N, T)
        self.mu_buf, self.logstd_buf = z(N, T, act_dim), z(N, T, act_dim)
        self.gamma, self.lam = float(gamma), float(lam)
        self.ptr = 0                                                     # same for every env (trpo.py:54)
        self.path_start_idx = torch.zeros(N, dtype=torch.int32, device=self.device)
        self.max_ep_len, self.env_num = T, N
        self.obs_dim, self.act_dim = obs_dim, act_dim
        self._lib = _native.load()

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    @staticmethod
    def _f32(t, shape):
        t = t.detach()
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        assert tuple(t.shape) == shape, (tuple(t.shape), shape)
        return t

    def store(self, obs, act, rew, val, logp, mu, logstd):
        """trpo.py:49-64: one step of every env into column `ptr`."""
        assert self.ptr < self.max_ep_len
        N, D, A = self.env_num, self.obs_dim, self.act_dim
        obs, act = self._f32(obs, (N, D)), self._f32(act, (N, A))
        mu, logstd = self._f32(mu, (N, A)), self._f32(logstd, (N, A))
        rew, val, logp = (self._f32(x.reshape(N), (N,)) for x in (rew, val, logp))
        _native.check(self._lib.gx_buffer_store(
            N, self.max_ep_len, self.ptr, D, A, obs.data_ptr(), act.data_ptr(), rew.data_ptr(),
            val.data_ptr(), logp.data_ptr(), mu.data_ptr(), logstd.data_ptr(),
            self.obs_buf.data_ptr(), self.act_buf.data_ptr(), self.rew_buf.data_ptr(),
            self.val_buf.data_ptr(), self.logp_buf.data_ptr(), self.mu_buf.data_ptr(),
            self.logstd_buf.data_ptr(), self._stream()))
        self.ptr += 1

    def finish_path(self, last_val=None, done=None):
        """trpo.py:66-119.  `done` (env_num,) selects the envs whose current path ends (== 1);
        None / all-ones closes every path.  `last_val` (env_num,) bootstraps the tail."""
        N = self.env_num
        if last_val is None:
            last_val = torch.zeros(N, device=self.device)
        last_val = self._f32(torch.as_tensor(last_val, device=self.device).reshape(N), (N,))
        dptr = None
        if done is not None:
            done = self._f32(torch.as_tensor(done, device=self.device).reshape(N), (N,))
            dptr = done.data_ptr()
        _native.check(self._lib.gx_gae_finish_path(
            N, self.max_ep_len, self.ptr, self.rew_buf.data_ptr(), self.val_buf.data_ptr(),
            last_val.data_ptr(), dptr, self.path_start_idx.data_ptr(), self.gamma, self.lam,
            self.adv_buf.data_ptr(), self.ret_buf.data_ptr(), 1, self._stream()))

    def get(self):
        """trpo.py:121-146: per-env normalised advantages, flattened views of every field."""
        assert self.ptr == self.max_ep_len
        self.ptr = 0
        self.path_start_idx.zero_()
        N, T = self.env_num, self.max_ep_len
        _native.check(self._lib.gx_adv_normalize(N, T, self.adv_buf.data_ptr(), 1, self._stream()))
        return dict(obs=self.obs_buf.view(N * T, -1), act=self.act_buf.view(N * T, -1),
                    ret=self.ret_buf.view(N * T), adv=self.adv_buf.view(N * T),
                    logp=self.logp_buf.view(N * T), mu=self.mu_buf.view(N * T, -1),
                    logstd=self.logstd_buf.view(N * T, -1))


class DeviceCostRolloutBuffer(DeviceRolloutBuffer):
    """`CPOBufferX` (safe_rl_libX/cpo/cpo.py:22-175): the TRPO buffer plus a cost channel
    (`cost_buf`, `cost_val_buf` -> `adc_buf`, `cost_ret_buf`); the cost advantage is centred but
    not scaled in `get()` (cpo.py:158-162)."""

    def __init__(self, env_num, max_ep_len, obs_dim, act_dim, gamma=0.99, lam=0.95, device=None):
        super().__init__(env_num, max_ep_len, obs_dim, act_dim, gamma, lam, device)
        z = lambda: torch.zeros(self.env_num, self.max_ep_len, dtype=torch.float32, device=self.device)  # noqa: E731
        self.cost_buf, self.cost_ret_buf, self.cost_val_buf, self.adc_buf = z(), z(), z(), z()

    def store(self, obs, act, rew, val, logp, cost, cost_val, mu, logstd):   # cpo.py:51-69
        p = self.ptr
        super().store(obs, act, rew, val, logp, mu, logstd)
        self.cost_buf[:, p] = cost.reshape(self.env_num)
        self.cost_val_buf[:, p] = cost_val.reshape(self.env_num)

    def finish_path(self, last_val=None, last_cost_val=None, done=None):     # cpo.py:71-140
        N = self.env_num
        zeros = lambda: torch.zeros(N, device=self.device)   # noqa: E731
        last_val = self._f32(torch.as_tensor(zeros() if last_val is None else last_val, device=self.device).reshape(N), (N,))
        last_cv = self._f32(torch.as_tensor(zeros() if last_cost_val is None else last_cost_val,
                                            device=self.device).reshape(N), (N,))
        dptr = None
        if done is not None:
            done = self._f32(torch.as_tensor(done, device=self.device).reshape(N), (N,))
            dptr = done.data_ptr()
        for rew, val, lv, adv, ret, advance in (
                (self.cost_buf, self.cost_val_buf, last_cv, self.adc_buf, self.cost_ret_buf, 0),
                (self.rew_buf, self.val_buf, last_val, self.adv_buf, self.ret_buf, 1)):
            _native.check(self._lib.gx_gae_finish_path(
                N, self.max_ep_len, self.ptr, rew.data_ptr(), val.data_ptr(), lv.data_ptr(), dptr,
                self.path_start_idx.data_ptr(), self.gamma, self.lam, adv.data_ptr(), ret.data_ptr(),
                advance, self._stream()))

    def get(self):                                                           # cpo.py:142-175
        data = super().get()
        N, T = self.env_num, self.max_ep_len
        _native.check(self._lib.gx_adv_normalize(N, T, self.adc_buf.data_ptr(), 0, self._stream()))
        data['cost_ret'] = self.cost_ret_buf.view(N * T)
        data['adc'] = self.adc_buf.view(N * T)
        return data


def gae_rollout(rew, val, done, last_val=None, gamma=0.99, lam=0.95):
    """GAE-lambda advantages and rewards-to-go for a whole fused rollout (time-major (T, N) tensors from
    Engine.rollout / rollout_policy): equivalent to TRPOBufferX.store + finish_path at every done step +
    the closing finish_path (trpo.py:466-547), in one kernel launch.  Returns (adv, ret), both (T, N)."""
    T, N = rew.shape
    dev = rew.device
    f = lambda x: x.to(torch.float32).contiguous()   # noqa: E731
    rew, val, done = f(rew), f(val), f(done)
    last_val = torch.zeros(N, device=dev) if last_val is None else f(last_val.reshape(N))
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    lib = _native.load()
    _native.check(lib.gx_gae_rollout(N, T, rew.data_ptr(), val.data_ptr(), done.data_ptr(), last_val.data_ptr(),
                                     float(gamma), float(lam), adv.data_ptr(), ret.data_ptr(),
                                     C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index))))
    return adv, ret


def _gae_host(rew, val, done, gamma, lam):
    """gae_rollout + the per-env normalisation for HOST tensors, in plain torch: the same recursion the kernels run
    (paths closed with 0 at every step with done == 1 and at step T - 1).  A path closes where done == 1 and nowhere
    else, which is what the kernels read (gx_gae.hip) and what the buffers of the three learners this serves do
    (np.where(done == 1): safelayer.py:109, usl.py:112, lpg.py:112).  Returns (adv normalised, env-major (N, T); ret (T, N))."""
    T, N = rew.shape
    adv, ret = torch.empty_like(rew), torch.empty_like(rew)
    a_next, r_next, v_next = torch.zeros(N), torch.zeros(N), torch.zeros(N)
    for t in range(T - 1, -1, -1):
        live = 1.0 - (done[t] == 1).to(torch.float32) if t + 1 < T else torch.zeros(N)
        delta = rew[t] + gamma * live * v_next - val[t]
        a_next = delta + gamma * lam * live * a_next
        r_next = rew[t] + gamma * live * r_next
        adv[t], ret[t], v_next = a_next, r_next, val[t]
    adv = adv.transpose(0, 1).contiguous()
    mean = adv.sum(1, keepdim=True) / T
    std = (((adv - mean) ** 2).sum(1, keepdim=True) / T).sqrt()
    return (adv - mean) / std, ret


def _env_major(x):
    return x.transpose(0, 1).contiguous()   # (T, N, ...) -> (N, T, ...)


def _require(out, keys, who, source):
    for k in keys:
        if k not in out:
            raise KeyError(f"{who} needs out['{k}'] ({source})")


def _channel(rew, val, done, last_val, gamma, lam, scale=1):
    """One GAE channel of a rollout, (T, N) tensors -> (advantage: env-major (N, T), per env normalised, or centred only
    with scale=0; returns-to-go: (T, N)).  Device tensors go through the GAE and normalisation kernels; host tensors (a
    result moved to the CPU) through the same recursion in torch, which serves the reward channel without bootstrap."""
    if not rew.is_cuda:
        if last_val is not None or not scale:
            raise NotImplementedError("host tensors: only the normalised reward channel without bootstrap")
        f = lambda x: x.to(torch.float32)   # noqa: E731
        return _gae_host(f(rew), f(val), f(done), float(gamma), float(lam))
    T, N = rew.shape
    adv, ret = gae_rollout(rew, val, done, last_val, gamma, lam)
    adv = _env_major(adv)
    _native.check(_native.load().gx_adv_normalize(N, T, adv.data_ptr(), scale,
                                                  C.c_void_p(torch._C._cuda_getCurrentRawStream(adv.device.index))))
    return adv, ret


def _batch(out, adv, ret, **more):
    """What every *_rollout_batch returns, env-major and flattened: obs act ret adv logp mu logstd from a rollout's `out`
    and its reward channel, then the path's own time-major tensors `more`."""
    T, N = out['rew'].shape
    A = out['act'].shape[-1]
    flat = lambda x: _env_major(x).view(N * T, *x.shape[2:])   # noqa: E731
    return dict(obs=flat(out['obs']), act=flat(out['act']), ret=flat(ret), adv=adv.view(N * T),
                logp=flat(out['logp']), mu=flat(out['mu']),
                logstd=out['logstd'].reshape(1, A).expand(N * T, A).contiguous(),
                **{k: flat(v) for k, v in more.items()})


def cost_rollout_batch(out, gamma=0.99, lam=0.95):
    """A rollout_policy(..., cost_critic=pack_critic(ac.vc)) result as the batch DeviceCostRolloutBuffer.get() returns
    after CPO's collection loop (cpo.py:596-660): store() every step, finish_path() with v = vc = 0 for the envs done at
    that step, a closing finish_path() over every env without bootstrap.  Env-major, flattened:
    obs act ret adv cost_ret adc logp mu logstd; adv normalised per env, adc centred per env only (cpo.py:142-175)."""
    _require(out, ('vc', 'rew', 'val', 'cost', 'done', 'obs'), "cost_rollout_batch", "rollout_policy(..., cost_critic=...)")
    adv, ret = _channel(out['rew'], out['val'], out['done'], None, gamma, lam)
    adc, cost_ret = _channel(out['cost'], out['vc'], out['done'], None, gamma, lam, scale=0)
    return dict(_batch(out, adv, ret, cost_ret=cost_ret), adc=adc.view(-1))


def statewise_rollout_batch(out, gamma=0.99, lam=0.95, cgamma=1.0, clam=0.95, cost_signal='increment', bootstrap=False):
    """An Engine.rollout_statewise result as the batch SCPOBufferX.get() returns after SCPO's collection loop
    (safe_rl_libX/scpo/scpo.py:30-175, 640-720): store() every step, finish_path() with v = vc = 0 for the envs done at
    that step, a closing finish_path() at the time-out.  The cost channel runs with SCPO's own cgamma / clam
    (scpo.py:36: no discount of the cost).  Env-major, flattened: obs act ret adv cost_ret adc logp mu logstd; adv
    normalised per env, adc centred per env only (scpo.py:148-160).
    cost_signal: 'increment' = out['cost_inc'], the max(cost - M, 0) SCPO defines; 'reference' = out['M']: what
    scpo.py:647-654 stores as written (its `cost_increase` and `M_next` are the same tensor, which ends up holding M_next).
    bootstrap: False closes every path at step T - 1 with 0, as SCPO's time-out does (scpo.py:683-686); True bootstraps
    the envs not done at step T - 1 with val_last / vc_last (a call shorter than the episode)."""
    if cost_signal not in ('increment', 'reference'):
        raise ValueError(f"cost_signal must be 'increment' or 'reference', got {cost_signal!r}")
    _require(out, ('vc', 'rew', 'val', 'cost_inc', 'M', 'done', 'obs', 'val_last', 'vc_last'),
             "statewise_rollout_batch", "Engine.rollout_statewise")
    costs = out['cost_inc'] if cost_signal == 'increment' else out['M']
    lv, lvc = None, None
    if bootstrap:
        alive = 1.0 - out['done'][-1]
        lv, lvc = out['val_last'] * alive, out['vc_last'] * alive
    adv, ret = _channel(out['rew'], out['val'], out['done'], lv, gamma, lam)
    adc, cost_ret = _channel(costs, out['vc'], out['done'], lvc, cgamma, clam, scale=0)
    return dict(_batch(out, adv, ret, cost_ret=cost_ret), adc=adc.view(-1))


def safelayer_rollout_batch(out, gamma=0.99, lam=0.95):
    """An Engine.rollout_safelayer result as the batch SafeLayerBufferX.get() returns after the safelayer learner's
    collection loop (safe_rl_libX/safelayer/safelayer.py:32-154, 514-583): store() every step, finish_path() with v = 0
    for the envs done at that step, a closing finish_path() over every env at the time-out, without bootstrap.
    Env-major, flattened: obs act act_safe ret adv logp mu logstd cost prev_cost; adv normalised per env
    (safelayer.py:137-141).  Device tensors go through the GAE and normalisation kernels; a dict of host tensors (a
    result moved to the CPU) is served by the same recursion in torch."""
    _require(out, ('obs', 'act', 'act_safe', 'rew', 'val', 'logp', 'mu', 'logstd', 'cost', 'prev_cost', 'done'),
             "safelayer_rollout_batch", "Engine.rollout_safelayer")
    adv, ret = _channel(out['rew'], out['val'], out['done'], None, gamma, lam)
    return _batch(out, adv, ret, act_safe=out['act_safe'], cost=out['cost'], prev_cost=out['prev_cost'])


def _q_target_batch(out, gamma, lam, who, source):
    """USLBufferX.get() and LPGBufferX.get(): the two classes keep the same fields, close paths the same way and build
    the same targetc (usl.py:26-159 and lpg.py:26-159 differ in their names only).  Both close a path where done == 1
    (usl.py:112, lpg.py:112), so that is where qc[t + 1] is taken as 0, on host tensors as in the kernels."""
    _require(out, ('obs', 'act', 'act_safe', 'rew', 'val', 'logp', 'mu', 'logstd', 'cost', 'qc', 'done'), who, source)
    adv, ret = _channel(out['rew'], out['val'], out['done'], None, gamma, lam)
    f = lambda x: x.to(torch.float32)   # noqa: E731
    qc, done = f(out['qc']), f(out['done'])
    q_next = torch.zeros_like(qc)
    q_next[:-1] = qc[1:] * (1.0 - (done[:-1] == 1).to(torch.float32))
    targetc = f(out['cost']) + float(gamma) * q_next
    return _batch(out, adv, ret, act_safe=out['act_safe'], cost=out['cost'], targetc=targetc)


def usl_rollout_batch(out, gamma=0.99, lam=0.95):
    """An Engine.rollout_usl result as the batch USLBufferX.get() returns after the USL learner's collection loop
    (safe_rl_libX/usl/usl.py:50-159, 478-553): store() every step, finish_path() with v = 0 for the envs done at that
    step, a closing finish_path() over every env at the time-out, without bootstrap.  Env-major, flattened:
    obs act act_safe ret adv logp mu logstd cost targetc; adv normalised per env (usl.py:142-146);
    targetc[t] = cost[t] + gamma qc[t + 1] with qc taken as 0 past the end of a path (usl.py:105-107, 125-127): at every
    done step and at step T - 1.  Device tensors go through the GAE and normalisation kernels; a dict of host tensors (a
    result moved to the CPU) is served by the same recursion in torch."""
    return _q_target_batch(out, gamma, lam, "usl_rollout_batch", "Engine.rollout_usl")


def lpg_rollout_batch(out, gamma=0.99, lam=0.95):
    """An Engine.rollout_lpg result as the batch LPGBufferX.get() returns after the LPG learner's collection loop
    (safe_rl_libX/lpg/lpg.py:50-159, 486-564): the same buffer as USL's under another name, so the same batch as
    usl_rollout_batch: obs act act_safe ret adv logp mu logstd cost targetc, env-major and flattened, adv normalised per
    env, targetc[t] = cost[t] + gamma qc[t + 1] with qc of the UNCORRECTED action and 0 past the end of a path.  (`lam`
    here is GAE's lambda; out['lam'], the projection's multiplier, is not part of the batch.)"""
    return _q_target_batch(out, gamma, lam, "lpg_rollout_batch", "Engine.rollout_lpg")


def _episode_lengths(first_done, T):
    """L = first_done ? min(first_done, T) : T, int64 (N,)"""
    fd = first_done.to(torch.int64)
    return torch.where(fd > 0, fd.clamp(max=T), torch.full_like(fd, T))


def _episode_channel_host(rew, val, last, L, finished, gamma, lam, scale):
    """One channel of gxe_finish in torch, operation for operation (include/guardx_episode.h): (T, N) host tensors ->
    (advantage (T, N) normalised over all T entries of an env, or centred only; returns-to-go (T, N)), 0 on [L, T)."""
    T, N = rew.shape
    f32, f64 = torch.float32, torch.float64
    g32 = torch.tensor(gamma, dtype=f32)
    dg = float(g32)
    dgl = dg * float(torch.tensor(lam, dtype=f32))
    boot = torch.where(finished, torch.zeros(N, dtype=f32), last.to(f32))
    adv, ret = torch.zeros(T, N, dtype=f32), torch.zeros(T, N, dtype=f32)
    a, r, v_next, s = torch.zeros(N, dtype=f64), boot.to(f64), boot.clone(), torch.zeros(N, dtype=f32)
    for t in range(T - 1, -1, -1):
        m = L > t                                   # the envs whose path holds step t
        delta = (rew[t] + g32 * v_next) - val[t]
        a = torch.where(m, delta.to(f64) + dgl * a, a)
        r = torch.where(m, rew[t].to(f64) + dg * r, r)
        adv[t] = torch.where(m, a.to(f32), adv[t])
        ret[t] = torch.where(m, r.to(f32), ret[t])
        s = torch.where(m, s + adv[t], s)
        v_next = torch.where(m, val[t], v_next)
    Tf = torch.tensor(float(T), dtype=f32)
    mean = s / Tf
    if not scale:
        return torch.where(L > torch.arange(T).view(T, 1), adv - mean, adv), ret
    q = torch.zeros(N, dtype=f32)
    for t in range(T):
        d = adv[t] - mean
        q = q + d * d
    # the square root through float64: torch's float32 sqrt on the CPU is not correctly rounded on every build, the
    # device's is, and the float64 root of a float32 value rounds to the correctly rounded float32 root
    sd = (q / Tf).to(f64).sqrt().to(f32)
    return (adv - mean) / sd, ret


def episode_rollout_batch(out, gamma=0.99, lam=0.95):
    """An Engine.rollout_episode result covering a whole episode (out['t0'] == 0, else ValueError) as the batch the
    one-episode buffer's get() returns after its finish_path (trpo_one_episode/trpo.py:67-132, cpo_one_episode/
    cpo.py:72-156), first epoch.  Per env, with L = first_done or T: GAE-lambda and rewards-to-go over [0, L), closed with
    val_last for the envs that never finished and with 0 for the others; adv normalised over ALL T entries of the env's
    row, the zeros on [L, T) included (mpi_tools.py:81-86; no guard on a zero deviation); with out['vc'] the same on
    cost / vc / vc_last, centred only.  Then the valid rows only, env-major, in the order x.view(N T, .)[valid] gives:
    obs act ret adv logp mu logstd (+ cost_ret adc), each a view of the first n_valid rows of an (N T)-row tensor whose
    other rows are left unwritten, and n_valid.  Device tensors: two launches (gxe_finish) and ONE .item(), the only
    synchronisation.  Host tensors (a result moved to the CPU) go through the same recursion in torch, operation for
    operation, so the two agree bit for bit.
    The episode=True results of rollout_safelayer / rollout_usl / rollout_lpg (the one-episode buffers of
    safelayer_one_episode/safelayer.py:30-140, usl_one_episode/usl.py:22-144; LPG's is USL's) are served too, keyed on
    what `out` holds: with out['act_safe'] also act_safe; with out['prev_cost'] also cost and prev_cost; with out['qc']
    also cost and targetc, targetc[t] = cost[t] + gamma32 * qc[t + 1] (one fp32 multiply, one fp32 add), the product
    taken as +0 at t + 1 == L (usl.py:105-107).  Same two launches (guardx_episode_finish_cols), same one .item().
    (The reference never re-zeroes adv_buf / adc_buf between epochs: from its second epoch on the entries past
    first_done hold the previous epoch's normalised values and leak into mean and deviation.  Here they are 0, which is
    what its first epoch sees.)"""
    keys = ('obs', 'act', 'mu', 'logp', 'rew', 'val', 'val_last', 'logstd', 'first_done', 't0')
    _require(out, keys, "episode_rollout_batch", "Engine.rollout_episode")
    if int(out['t0']) != 0:
        raise ValueError(f"episode_rollout_batch needs the call that starts the episode (out['t0'] == 0), got t0 = {out['t0']}")
    has_cost = 'vc' in out
    if has_cost:
        _require(out, ('cost', 'vc_last'), "episode_rollout_batch", "Engine.rollout_episode(..., cost_critic=...)")
    T, N = out['rew'].shape
    D, A = out['obs'].shape[-1], out['act'].shape[-1]
    # the safe-action learners' extra columns: (key, width)
    cols = [('act_safe', A)] if 'act_safe' in out else []
    has_q = 'qc' in out
    if 'prev_cost' in out or has_q:
        _require(out, ('cost',), "episode_rollout_batch", "Engine.rollout_safelayer / rollout_usl / rollout_lpg(..., episode=True)")
        cols.append(('cost', 1))
    if 'prev_cost' in out:
        cols.append(('prev_cost', 1))
    # gxe_finish is handed raw pointers: every tensor must have the shape the sizes above promise
    shapes = dict(obs=(T, N, D), act=(T, N, A), mu=(T, N, A), logp=(T, N), val=(T, N), val_last=(N,), first_done=(N,),
                  logstd=(A,))
    if has_cost:
        shapes.update(cost=(T, N), vc=(T, N), vc_last=(N,))
    shapes.update({k: (T, N, A) if k == 'act_safe' else (T, N) for k, _ in cols})
    if has_q:
        shapes.update(qc=(T, N))
    for k, want in shapes.items():
        if tuple(out[k].shape) != want:
            raise ValueError(f"episode_rollout_batch: out['{k}'] has shape {tuple(out[k].shape)}; expected {want} "
                             f"(from out['rew'] {(T, N)}, out['obs'] and out['act'])")
    f = lambda x: x.to(torch.float32).contiguous()   # noqa: E731
    if not out['rew'].is_cuda:
        L = _episode_lengths(out['first_done'], T)
        finished = out['first_done'] > 0
        valid = (torch.arange(T).view(1, T) < L.view(N, 1)).reshape(N * T)
        pick = lambda x: _env_major(f(x)).reshape(N * T, *x.shape[2:])[valid]   # noqa: E731
        adv, ret = _episode_channel_host(f(out['rew']), f(out['val']), out['val_last'], L, finished, gamma, lam, 1)
        n_valid = int(L.sum())
        batch = dict(obs=pick(out['obs']), act=pick(out['act']), ret=pick(ret), adv=pick(adv), logp=pick(out['logp']),
                     mu=pick(out['mu']))
        if has_cost:
            adc, cost_ret = _episode_channel_host(f(out['cost']), f(out['vc']), out['vc_last'], L, finished, gamma, lam, 0)
            batch.update(cost_ret=pick(cost_ret), adc=pick(adc))
        batch.update({k: pick(out[k]) for k, _ in cols})
        if has_q:
            qc = f(out['qc'])
            q_next = torch.zeros_like(qc)
            q_next[:-1] = torch.tensor(gamma, dtype=torch.float32) * qc[1:]
            q_next = torch.where(torch.arange(1, T + 1).view(T, 1) < L.view(1, N), q_next, torch.zeros_like(qc))
            batch['targetc'] = pick(f(out['cost']) + q_next)
    else:
        from . import _episode_native
        lib = _episode_native.load()
        dev = out['rew'].device
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
        src = {k: f(out[k]) for k in ('obs', 'act', 'mu', 'logp', 'rew', 'val', 'val_last')}
        cost = {k: f(out[k]) for k in ('cost', 'vc', 'vc_last')} if has_cost else {}
        extra = {k: f(out[k]) for k, _ in cols}
        qsrc = {k: f(out[k]) for k in ('qc', 'cost')} if has_q else {}
        fd = out['first_done'].to(device=dev, dtype=torch.int32).contiguous()
        batch = dict(obs=new(N * T, D), act=new(N * T, A), ret=new(N * T), adv=new(N * T), logp=new(N * T), mu=new(N * T, A))
        if has_cost:
            batch.update(cost_ret=new(N * T), adc=new(N * T))
        batch.update({k: new(N * T, w) if k == 'act_safe' else new(N * T) for k, w in cols})
        if has_q:
            batch['targetc'] = new(N * T)
        carr = (_episode_native.GxeFinishCol * max(1, len(cols)))()
        for c, (k, w) in zip(carr, cols):
            c.d_src, c.d_dst, c.width = extra[k].data_ptr(), batch[k].data_ptr(), w
        qp = lambda t: t.data_ptr() if has_q else None   # noqa: E731
        count = torch.empty(1, dtype=torch.int32, device=dev)
        work = new(int(lib.gxe_finish_work_floats(N, T)))
        cp = lambda k: cost[k].data_ptr() if has_cost else None   # noqa: E731
        bp = lambda k: batch[k].data_ptr() if has_cost else None   # noqa: E731
        with torch.cuda.device(dev):
            _episode_native.check(lib.guardx_episode_finish_cols(
                N, T, D, A, float(gamma), float(lam), fd.data_ptr(), src['obs'].data_ptr(), src['act'].data_ptr(),
                src['mu'].data_ptr(), src['logp'].data_ptr(), src['rew'].data_ptr(), src['val'].data_ptr(),
                src['val_last'].data_ptr(), cp('cost'), cp('vc'), cp('vc_last'), work.data_ptr(), batch['obs'].data_ptr(),
                batch['act'].data_ptr(), batch['mu'].data_ptr(), batch['logp'].data_ptr(), batch['ret'].data_ptr(),
                batch['adv'].data_ptr(), bp('cost_ret'), bp('adc'), len(cols), C.cast(carr, C.c_void_p) if cols else None,
                qp(qsrc.get('qc')), qp(qsrc.get('cost')), qp(batch.get('targetc')), count.data_ptr(),
                C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index))))
        n_valid = int(count.item())
        batch = {k: v[:n_valid] for k, v in batch.items()}
    batch['logstd'] = out['logstd'].reshape(1, A).expand(n_valid, A).contiguous()
    batch['n_valid'] = n_valid
    return batch
