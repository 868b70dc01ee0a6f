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

from . import _closed_loop as _cl, _statewise_native
from ._closed_loop import policy_floats  # noqa: F401 (part of this module's surface)
from .critic import HIDDEN, critic_floats, critic_hidden

# how pack_critic marks what the packed critic's output layer is followed by (sizes are equal either way)
OUTPUT_ATTR = "gx_output"


def critic_output(t):
    """'identity' / 'softplus' as Engine.pack_critic declared it, None for a tensor that carries no declaration"""
    return getattr(t, OUTPUT_ATTR, None)


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


class State(_cl.State):
    """the slab and the noise counter of _closed_loop.State, and M / first (one (2, N) tensor)"""

    def __init__(self, env):
        N = env.env_num
        self.init = torch.zeros(2, N, dtype=torch.float32, device=env.device)
        self.init[1].fill_(1.0)
        self.mf = self.init.clone()          # [0] = M, [1] = first (1.f / 0.f)
        super().__init__(env)

    def reset(self):
        self.mf.copy_(self.init)


def rollout(env, params, T, cost_critic, obs0=None, noise_seed=(0, 0)):
    obs0, N, D, A, T = _cl.begin(env, "rollout_statewise", obs0, T)
    Da = D + 1
    if cost_critic is None:
        raise ValueError("rollout_statewise needs cost_critic=Engine.pack_critic(ac.vc, output='softplus')")
    declared = critic_output(cost_critic)
    if declared != 'softplus':
        raise ValueError("rollout_statewise evaluates the cost critic with a Softplus output (scpo_core.py "
                         f"MLPMaxCostCritic); cost_critic was packed with output={declared!r}: pack it with "
                         "Engine.pack_critic(ac.vc, output='softplus', device=...) (the declaration travels with the "
                         "tensor pack_critic returns, not with copies of it)")
    params, vcp, obs0, hidden = _cl.device_inputs(
        env, params, cost_critic, obs0, Da, A, f" for the {Da} = obs_dim + 1 inputs of the state-wise networks")
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
    a = _statewise_native.GxsStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0, rename=dict(M='d_M_after'))
    a.D_aug, a.hidden, a.vc_hidden = Da, hidden, vc_hidden
    a.d_vc_params = vcp.data_ptr()
    a.d_M, a.d_first = st.mf[0].data_ptr(), st.mf[1].data_ptr()

    def prepare(stream):
        return lib.gxs_prepare(Da, A, hidden, vc_hidden, a.d_params, a.d_vc_params, a.d_work, stream)

    _cl.run(env, st, a, out, T, prepare, lib.gxs_policy_step, _statewise_native.check, out['act'])
    # _obs = the env's own (N, D) rows after the last reset_done (the slab's are rewritten by the next call)
    env._obs = st.slab[1][0].clone()
    return out
