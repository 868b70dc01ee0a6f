"""The state-wise (SCPO) rollout on the device: `Engine.rollout_statewise` (safe_rl_libX/scpo/scpo.py:640-720 with the
actor-critic of scpo_core.py:158-200 evaluated there).

SCPO's networks read o_aug = cat(obs, M): M is the env's running maximum of the cost since its episode began, and what
the learner stores is the cost increment max(cost - M, 0).  M depends on the cost of the step just made, so it sits
inside the closed loop.  Per control step: one `gxs_policy_step` launch (libguardx_statewise.so,
include/guardx_statewise.h: the M update of the step just made, then ac.step on o_aug) and one `gx_step_slab` launch
(env.step with the speculated reset_done, committed on the host) -- the two launches per control step the step-wise
rollout_policy already has.  Everything runs on torch's current stream; nothing synchronises.
"""
import ctypes as C

import torch

from . import _native, _statewise_native
from .critic import HIDDEN, critic_floats, critic_hidden

# how pack_critic marks what the packed critic's output layer is followed by (sizes are equal either way)
OUTPUT_ATTR = "gx_output"


def critic_output(t):
    """'identity' / 'softplus' as Engine.pack_critic declared it, None for a tensor that carries no declaration"""
    return getattr(t, OUTPUT_ATTR, None)


def policy_floats(D_aug, A, h):
    return 2 * (h * D_aug + h + h * h + h) + (A + 1) * h + (A + 1) + A


def softplus_probe(x):
    """Softplus(x) as the kernel evaluates it, for x a float32 device tensor (gxs_softplus_probe)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError("softplus_probe: x must be a float32 device tensor")
    x = x.contiguous()
    if x.numel() >= 2 ** 31:
        raise ValueError("softplus_probe: more than 2^31 - 1 values")
    y = torch.empty_like(x)
    lib = _statewise_native.load()
    with torch.cuda.device(x.device):
        _statewise_native.check(lib.gxs_softplus_probe(x.numel(), x.data_ptr(), y.data_ptr(),
                                                       C.c_void_p(torch._C._cuda_getCurrentRawStream(x.device.index))))
    return y


class State:
    """what the path keeps per engine: M / first (one (2, N) tensor), the one-set output slab of its env.step launches,
    and its own count of policy steps (the noise counter: 0 at construction, + T per call, not reset by reset())"""

    def __init__(self, env):
        N = env.env_num
        self.init = torch.zeros(2, N, dtype=torch.float32, device=env.device)
        self.init[1].fill_(1.0)
        self.mf = self.init.clone()          # [0] = M, [1] = first (1.f / 0.f)
        self.slab = env._out_slab(1)
        self.steps = 0

    def reset(self):
        self.mf.copy_(self.init)


def rollout(env, params, T, cost_critic, obs0=None, noise_seed=(0, 0)):
    if obs0 is None:
        obs0 = env._obs
    if obs0 is None:
        raise RuntimeError("rollout_statewise() before reset()")
    N, D, A, T = env.env_num, env.obs_flat_size, env.action_space.shape[0], int(T)
    if T < 1:
        raise ValueError("rollout_statewise: T must be >= 1")
    Da = D + 1
    if cost_critic is None:
        raise ValueError("rollout_statewise needs cost_critic=Engine.pack_critic(ac.vc, output='softplus')")
    declared = critic_output(cost_critic)
    if declared != 'softplus':
        raise ValueError("rollout_statewise evaluates the cost critic with a Softplus output (scpo_core.py "
                         f"MLPMaxCostCritic); cost_critic was packed with output={declared!r}: pack it with "
                         "Engine.pack_critic(ac.vc, output='softplus', device=...) (the declaration travels with the "
                         "tensor pack_critic returns, not with copies of it)")
    params = params.to(device=env.device, dtype=torch.float32).contiguous()
    vcp = cost_critic.to(device=env.device, dtype=torch.float32).contiguous()
    obs0 = obs0.to(device=env.device, dtype=torch.float32).contiguous()
    if tuple(obs0.shape) != (N, D):
        raise ValueError(f"obs0 has shape {tuple(obs0.shape)}; expected {(N, D)}")
    hidden = next((h for h in HIDDEN if policy_floats(Da, A, h) == params.numel()), None)
    if hidden is None:
        raise ValueError(f"params has {params.numel()} floats; expected one of "
                         f"{[policy_floats(Da, A, h) for h in HIDDEN]} (hidden {HIDDEN}) for the {Da} = obs_dim + 1 "
                         "inputs of the state-wise networks")
    vc_hidden = critic_hidden(Da, vcp.numel())
    if vc_hidden is None:
        raise ValueError(f"cost_critic has {vcp.numel()} floats; expected one of "
                         f"{[critic_floats(Da, h) for h in HIDDEN]} (hidden {HIDDEN}) for {Da} = obs_dim + 1 inputs")
    lib = _statewise_native.load()
    st = env._statewise
    if st is None:
        st = env._statewise = State(env)
    new = env._new
    out = dict(obs=new(T, N, Da), act=new(T, N, A), mu=new(T, N, A), logp=new(T, N), val=new(T, N), vc=new(T, N),
               rew=new(T, N), cost=new(T, N), cost_inc=new(T, N), M=new(T, N), done=new(T, N),
               obs_last=new(N, Da), val_last=new(N), vc_last=new(N), logstd=new(A))
    work = new(int(lib.gxs_work_floats(Da, A, hidden, vc_hidden)))
    slab = st.slab
    s_obs, s_rd, s_rew, s_cost, s_done = slab[0][0], slab[1][0], slab[2][0], slab[3][0], slab[4][0]
    a = _statewise_native.GxsStepArgs()
    a.struct_size = C.sizeof(_statewise_native.GxsStepArgs)
    a.N, a.D_aug, a.A, a.hidden, a.vc_hidden = N, Da, A, hidden, vc_hidden
    a.env_offset = int(env._cfg.env_offset)
    a.T, a.t = T, 0
    a.seed[0], a.seed[1] = int(noise_seed[0]) & 0xFFFFFFFF, int(noise_seed[1]) & 0xFFFFFFFF
    a.step0 = st.steps & 0xFFFFFFFF
    a.d_params, a.d_vc_params, a.d_work = params.data_ptr(), vcp.data_ptr(), work.data_ptr()
    a.d_obs0, a.d_obs_rd = obs0.data_ptr(), s_rd.data_ptr()
    a.d_rew_in, a.d_cost_in, a.d_done_in = s_rew.data_ptr(), s_cost.data_ptr(), s_done.data_ptr()
    a.d_M, a.d_first = st.mf[0].data_ptr(), st.mf[1].data_ptr()
    for k, f in (('obs', 'd_obs'), ('act', 'd_act'), ('mu', 'd_mu'), ('logp', 'd_logp'), ('val', 'd_val'),
                 ('vc', 'd_vc'), ('rew', 'd_rew'), ('cost', 'd_cost'), ('done', 'd_done'), ('cost_inc', 'd_cost_inc'),
                 ('M', 'd_M_after'), ('obs_last', 'd_obs_last'), ('val_last', 'd_val_last'),
                 ('vc_last', 'd_vc_last'), ('logstd', 'd_logstd')):
        setattr(a, f, out[k].data_ptr())
    stream = env._raw_stream(env._dev_index)
    h, ref, spec, spec_ref = env._h, C.byref(a), env._spec, env._spec_ref
    step_fn, slab_fn, commit_fn, rd_fn = lib.gxs_policy_step, env._gx_step_slab, env._gx_commit, env._lib.gx_reset_done
    act_ptr, act_stride, slab_ptr = out['act'].data_ptr(), 4 * N * A, slab[6]
    obs_ptr, rd_ptr = s_obs.data_ptr(), s_rd.data_ptr()
    env._rd_obs = None
    with torch.cuda.device(env.device):
        _statewise_native.check(lib.gxs_prepare(Da, A, hidden, vc_hidden, a.d_params, a.d_vc_params, a.d_work, stream))
        for t in range(T):
            a.t = t
            rc = step_fn(ref, stream)
            if rc:
                _statewise_native.check(rc)
            # env.step(act[t]) and, in the same launch, what reset_done() returns for it (flags bit 1)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 2, spec_ref, stream)
            if rc:
                _native.check(rc)
            # thread-per-env kernels (env_num > 16384) do not speculate: reset_done as a launch of its own
            rc = commit_fn(h) if spec.value else rd_fn(h, obs_ptr, rd_ptr, stream)
            if rc:
                _native.check(rc)
        a.t = T
        _statewise_native.check(step_fn(ref, stream))
    st.steps += T
    # as rollout_policy leaves them; _obs = the env's own (N, D) rows after the last reset_done (the slab's are rewritten
    # by the next call)
    env._obs, env._reward, env._done = s_rd.clone(), out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out
