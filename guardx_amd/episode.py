"""The one-episode rollout on the device: `Engine.rollout_episode`, the collection loop of the `*_one_episode` learners
(safe_rl_libX/trpo_one_episode/trpo.py:450-545, cpo_one_episode/cpo.py:619-708) whose ac.step is the actor and v (a2c,
alphappo, apo, espo, papo, ppo, trpo, trpoipo, vmpo) or the actor, v and vc (cpo, pcpo, pdo, trpofac, trpolag).

These learners never call reset_done(): a finished env keeps being stepped, and the learner keeps per env the first step
at which `done` was 1 (first_done), sums reward and cost up to and including that step, bootstraps only the envs that
never finished and hands the update the rows before first_done.  Before ac.step it zeroes the NaN / Inf entries of the
observation.  Per control step: one `gxe_policy_step` launch (libguardx_episode.so, include/guardx_episode.h: the
bookkeeping of the step just made, the sanitised row, ac.step) and one `gx_step_slab` launch with flags = 0 -- a plain
env.step, nothing speculated, nothing committed.  Everything runs on torch's current stream; nothing synchronises.

Without a cost critic the value network's block of `params` stands in for the third network (the kernel's third group
of waves stays idle): gxe_prepare and the kernel dispatch are those of the other step libraries.
"""
import ctypes as C

import torch

from . import _closed_loop as _cl, _episode_native, _native
from ._closed_loop import policy_floats  # noqa: F401 (part of this module's surface)
from .critic import HIDDEN, critic_floats, critic_hidden


class State(_cl.State):
    """the slab and the noise counter of _closed_loop.State, and per env first_done / ep_len (int32), ep_ret / ep_cost
    (float32), with the number of steps the episode has made (t_base)"""

    def __init__(self, env):
        N = env.env_num
        self.ints = torch.zeros(2, N, dtype=torch.int32, device=env.device)      # [0] = first_done, [1] = ep_len
        self.sums = torch.zeros(2, N, dtype=torch.float32, device=env.device)    # [0] = ep_ret, [1] = ep_cost
        self.t_base = 0
        super().__init__(env)

    def reset(self):
        self.ints.zero_()
        self.sums.zero_()
        self.t_base = 0


def _cost_critic(who, cost_critic, D, device):
    """-> (the packed cost critic on the device, its hidden width); (None, None) without one"""
    if cost_critic is None:
        return None, None
    if getattr(cost_critic, 'gx_output', None) == 'softplus':
        raise ValueError(f"{who} evaluates the cost critic with a linear output; cost_critic was packed with "
                         "output='softplus' (SCPO's MLPMaxCostCritic: use rollout_statewise)")
    vcp = cost_critic.to(device=device, dtype=torch.float32).contiguous()
    vc_hidden = critic_hidden(D, vcp.numel())
    if vc_hidden is None:
        raise ValueError(f"cost_critic has {vcp.numel()} floats; expected one of "
                         f"{[critic_floats(D, h) for h in HIDDEN]} (hidden {HIDDEN})")
    return vcp, vc_hidden


def tail_probe(params, rows, act_dim, cost_critic=None):
    """The tail of a call alone on `rows` (n, D), a float32 device tensor (gxe_tail_probe): -> obs_last (the rows as
    they are), val_last and, with cost_critic, vc_last: the critics on the rows, 0 for a row with a non-finite entry."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2):
        raise ValueError("tail_probe: rows must be a float32 (n, D) device tensor")
    rows = rows.contiguous()
    n, D = rows.shape
    A = int(act_dim)
    if n >= 2 ** 31:
        raise ValueError("tail_probe: more than 2^31 - 1 rows")
    params = params.to(device=rows.device, dtype=torch.float32).contiguous()
    hidden = _cl.hidden_of(params.numel(), lambda h: policy_floats(D, A, h))
    if hidden is None:
        raise ValueError(f"params has {params.numel()} floats; expected one of "
                         f"{[policy_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN})")
    vcp, vc_hidden = _cost_critic("tail_probe", cost_critic, D, rows.device)
    has_vc = vcp is not None
    third = vcp if has_vc else params[_cl.net_floats(D, A, hidden):]
    lib = _episode_native.load()
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=rows.device)   # noqa: E731
    out = dict(obs_last=new(n, D), val_last=new(n))
    if has_vc:
        out['vc_last'] = new(n)
    h3 = vc_hidden if has_vc else hidden
    work = new(int(lib.gxe_work_floats(D, A, hidden, h3)))
    stream = C.c_void_p(torch._C._cuda_getCurrentRawStream(rows.device.index))
    with torch.cuda.device(rows.device):
        _episode_native.check(lib.gxe_prepare(D, A, hidden, h3, params.data_ptr(), third.data_ptr(), work.data_ptr(), stream))
        _episode_native.check(lib.gxe_tail_probe(
            n, D, A, hidden, h3, int(has_vc), params.data_ptr(), third.data_ptr(), work.data_ptr(), rows.data_ptr(),
            out['obs_last'].data_ptr(), out['val_last'].data_ptr(), out['vc_last'].data_ptr() if has_vc else None, stream))
    return out


def rollout(env, params, T, obs0=None, noise_seed=(0, 0), cost_critic=None):
    obs0, N, D, A, T = _cl.begin(env, "rollout_episode", obs0, T)
    vcp, vc_hidden = _cost_critic("rollout_episode", cost_critic, D, env.device)
    has_vc = vcp is not None
    # (device_inputs moves its `third` argument like the others: params itself where there is no cost critic)
    params, third, obs0, hidden = _cl.device_inputs(env, params, vcp if has_vc else params, obs0, D, A)
    if not has_vc:
        third, vc_hidden = params[_cl.net_floats(D, A, hidden):], hidden     # the value network's block stands in
    lib = _episode_native.load()
    st = env._episode
    if st is None:
        st = env._episode = State(env)
    new = env._new
    out = dict(obs=new(T, N, D), act=new(T, N, A), mu=new(T, N, A), logp=new(T, N), val=new(T, N), rew=new(T, N),
               cost=new(T, N), done=new(T, N), obs_last=new(N, D), val_last=new(N), logstd=new(A))
    if has_vc:
        out['vc'], out['vc_last'] = new(T, N), new(N)
    work = new(int(lib.gxe_work_floats(D, A, hidden, vc_hidden)))
    a = _episode_native.GxeStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0)
    slab = st.slab
    a.d_obs_rd = slab[0][0].data_ptr()     # the env's plain observation: a flags = 0 step writes no obs_rd piece
    a.D, a.hidden, a.vc_hidden, a.has_vc = D, hidden, vc_hidden, int(has_vc)
    a.t_base = st.t_base
    a.d_vc_params = third.data_ptr()
    a.d_first_done, a.d_ep_len = st.ints[0].data_ptr(), st.ints[1].data_ptr()
    a.d_ep_ret, a.d_ep_cost = st.sums[0].data_ptr(), st.sums[1].data_ptr()

    check = _episode_native.check
    stream = env._raw_stream(env._dev_index)
    h, ref, spec_ref = env._h, C.byref(a), env._spec_ref
    step_fn, slab_fn = lib.gxe_policy_step, env._gx_step_slab
    act = out['act']
    act_ptr, act_stride, slab_ptr = act.data_ptr(), 4 * N * A, slab[6]
    env._rd_obs = None
    with torch.cuda.device(env.device):
        check(lib.gxe_prepare(D, A, hidden, vc_hidden, a.d_params, a.d_vc_params, a.d_work, stream))
        for t in range(T):
            a.t = t
            rc = step_fn(ref, stream)
            if rc:
                check(rc)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 0, spec_ref, stream)   # env.step(act[t]), nothing else
            if rc:
                _native.check(rc)
        a.t = T
        check(step_fn(ref, stream))
    out['t0'] = st.t_base
    st.steps += T
    st.t_base += T
    out['first_done'], out['ep_len'] = st.ints.clone().unbind(0)
    out['ep_ret'], out['ep_cost'] = st.sums.clone().unbind(0)
    # as a step() leaves them
    env._obs, env._reward, env._done = out['obs_last'], out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out
