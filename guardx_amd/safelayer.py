"""The safety-layer rollout on the device: `Engine.rollout_safelayer` (safe_rl_libX/safelayer/safelayer.py:514-581 with
the actor-critic and the C_Critic of safelayer_core.py:147-190 evaluated there; Dalal et al. 2018).

The learner edits the action between ac.step and env.step: a_safe = a - relu((g.a + prev_c - delta) / (g.g + 1e-8)) g,
clamped to [-1, 1], where pred = g.a + prev_c exceeds delta; g = g_net(obs) and prev_c is the cost of the env's previous
step (0 after a done or a reset()).  prev_c depends on the cost of the step just made, so it sits inside the closed
loop.  Per control step: one `gxl_policy_step` launch (libguardx_safelayer.so, include/guardx_safelayer.h: the prev_c
update of the step just made, ac.step, g_net, the correction) and one `gx_step_slab` launch on act_safe[t] (env.step with
the speculated reset_done, committed on the host) -- the two launches per control step the step-wise rollout_policy
already has.  Everything runs on torch's current stream; nothing synchronises.
"""
import ctypes as C

import torch

from . import _native, _safelayer_native
from .critic import HIDDEN

# how pack_g_net marks what it returns (a g_net and another A-output network of the same size look alike)
G_NET_ATTR = "gx_g_net"


def policy_floats(D, A, h):
    return 2 * (h * D + h + h * h + h) + (A + 1) * h + (A + 1) + A


def g_floats(D, A, h):
    return h * D + h + h * h + h + A * h + A


def pack_g_net(ccritic, device=None):
    """Flatten the safety layer's g_net (`ac.ccritic` of safelayer_core.py:147-156: anything with .g_net, or the
    nn.Sequential Linear/Tanh/Linear/Tanh/Linear[/Identity] itself) into W1 b1 W2 b2 W3 b3, float32.  Anything the kernel
    would evaluate differently raises NotImplementedError."""
    nn = torch.nn
    net = getattr(ccritic, 'g_net', ccritic)
    mods = [m for m in net if not isinstance(m, nn.Identity)]
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    if len(lin) != 3:
        raise NotImplementedError("rollout_safelayer supports a g_net with two hidden layers (--l 2)")
    if [type(m) for m in mods] != [nn.Linear, nn.Tanh] * 2 + [nn.Linear]:
        raise NotImplementedError("rollout_safelayer supports a g_net with Tanh hidden activations and a linear output "
                                  "only (activation=nn.Tanh, output_activation=nn.Identity)")
    if lin[0].out_features != lin[1].out_features or lin[1].in_features != lin[0].out_features \
            or lin[2].in_features != lin[1].out_features:
        raise NotImplementedError("rollout_safelayer supports a g_net with two hidden layers of equal width")
    if lin[0].out_features not in HIDDEN:
        raise NotImplementedError(f"rollout_safelayer supports g_net hidden widths {HIDDEN}")
    A = lin[2].out_features
    if A < 2 or A > 16 or A % 2:
        raise NotImplementedError(f"rollout_safelayer supports an even action width <= 16; g_net has {A} outputs")
    flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for m in lin for t in (m.weight, m.bias)])
    flat = flat.to(device) if device is not None else flat
    setattr(flat, G_NET_ATTR, A)
    return flat


def correction_probe(g, a, prev_c, delta=0.0):
    """the correction alone as the kernel evaluates it (gxl_correction_probe): g, a (n, A), prev_c (n,) float32 device
    tensors -> a_safe (n, A)"""
    for t in (g, a, prev_c):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise ValueError("correction_probe: g, a and prev_c must be float32 device tensors")
    if g.dim() != 2 or g.shape != a.shape or tuple(prev_c.shape) != (g.shape[0],):
        raise ValueError("correction_probe: g and a must be (n, A), prev_c (n,)")
    g, a, prev_c = g.contiguous(), a.contiguous(), prev_c.contiguous()
    n, A = g.shape
    if n >= 2 ** 31:
        raise ValueError("correction_probe: more than 2^31 - 1 rows")
    out = torch.empty_like(a)
    lib = _safelayer_native.load()
    with torch.cuda.device(g.device):
        _safelayer_native.check(lib.gxl_correction_probe(
            n, A, g.data_ptr(), a.data_ptr(), prev_c.data_ptr(), float(delta), out.data_ptr(),
            C.c_void_p(torch._C._cuda_getCurrentRawStream(g.device.index))))
    return out


class State:
    """what the path keeps per engine: prev_c (N,), the one-set output slab of its env.step launches, and its own count
    of policy steps (the noise counter: 0 at construction, + T per call, not reset by reset())"""

    def __init__(self, env):
        self.prev_c = torch.zeros(env.env_num, dtype=torch.float32, device=env.device)
        self.slab = env._out_slab(1)
        self.steps = 0

    def reset(self):
        self.prev_c.zero_()    # safelayer.py:567


def rollout(env, params, T, g_net, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0):
    if obs0 is None:
        obs0 = env._obs
    if obs0 is None:
        raise RuntimeError("rollout_safelayer() before reset()")
    N, D, A, T = env.env_num, env.obs_flat_size, env.action_space.shape[0], int(T)
    if T < 1:
        raise ValueError("rollout_safelayer: T must be >= 1")
    if g_net is None or not torch.is_tensor(g_net) or getattr(g_net, G_NET_ATTR, None) is None:
        raise ValueError("rollout_safelayer needs g_net=Engine.pack_g_net(ac.ccritic, device=...) (the declaration "
                         "travels with the tensor pack_g_net returns, not with copies of it)")
    params = params.to(device=env.device, dtype=torch.float32).contiguous()
    gp = g_net.to(device=env.device, dtype=torch.float32).contiguous()
    obs0 = obs0.to(device=env.device, dtype=torch.float32).contiguous()
    if tuple(obs0.shape) != (N, D):
        raise ValueError(f"obs0 has shape {tuple(obs0.shape)}; expected {(N, D)}")
    hidden = next((h for h in HIDDEN if policy_floats(D, A, h) == params.numel()), None)
    if hidden is None:
        raise ValueError(f"params has {params.numel()} floats; expected one of "
                         f"{[policy_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN})")
    g_hidden = next((h for h in HIDDEN if g_floats(D, A, h) == gp.numel()), None)
    if g_hidden is None or getattr(g_net, G_NET_ATTR) != A:
        raise ValueError(f"g_net has {gp.numel()} floats and {getattr(g_net, G_NET_ATTR)} outputs; expected one of "
                         f"{[g_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN}) for {D} inputs and {A} outputs")
    lib = _safelayer_native.load()
    st = env._safelayer
    if st is None:
        st = env._safelayer = State(env)
    new = env._new
    out = dict(obs=new(T, N, D), act=new(T, N, A), act_safe=new(T, N, A), mu=new(T, N, A), g=new(T, N, A),
               logp=new(T, N), val=new(T, N), rew=new(T, N), cost=new(T, N), prev_cost=new(T, N), done=new(T, N),
               obs_last=new(N, D), val_last=new(N), logstd=new(A))
    work = new(int(lib.gxl_work_floats(D, A, hidden, g_hidden)))
    slab = st.slab
    s_obs, s_rd, s_rew, s_cost, s_done = slab[0][0], slab[1][0], slab[2][0], slab[3][0], slab[4][0]
    a = _safelayer_native.GxlStepArgs()
    a.struct_size = C.sizeof(_safelayer_native.GxlStepArgs)
    a.N, a.D, a.A, a.hidden, a.g_hidden = N, D, A, hidden, g_hidden
    a.env_offset = int(env._cfg.env_offset)
    a.T, a.t = T, 0
    a.correct, a.delta = int(bool(correct)), float(delta)
    a.seed[0], a.seed[1] = int(noise_seed[0]) & 0xFFFFFFFF, int(noise_seed[1]) & 0xFFFFFFFF
    a.step0 = st.steps & 0xFFFFFFFF
    a.d_params, a.d_g_params, a.d_work = params.data_ptr(), gp.data_ptr(), work.data_ptr()
    a.d_obs0, a.d_obs_rd = obs0.data_ptr(), s_rd.data_ptr()
    a.d_rew_in, a.d_cost_in, a.d_done_in = s_rew.data_ptr(), s_cost.data_ptr(), s_done.data_ptr()
    a.d_prev_c = st.prev_c.data_ptr()
    for k in ('obs', 'act', 'act_safe', 'mu', 'g', 'logp', 'val', 'rew', 'cost', 'done', 'prev_cost', 'obs_last',
              'val_last', 'logstd'):
        setattr(a, 'd_' + k, out[k].data_ptr())
    stream = env._raw_stream(env._dev_index)
    h, ref, spec, spec_ref = env._h, C.byref(a), env._spec, env._spec_ref
    step_fn, slab_fn, commit_fn, rd_fn = lib.gxl_policy_step, env._gx_step_slab, env._gx_commit, env._lib.gx_reset_done
    act_ptr, act_stride, slab_ptr = out['act_safe'].data_ptr(), 4 * N * A, slab[6]
    obs_ptr, rd_ptr = s_obs.data_ptr(), s_rd.data_ptr()
    env._rd_obs = None
    with torch.cuda.device(env.device):
        _safelayer_native.check(lib.gxl_prepare(D, A, hidden, g_hidden, a.d_params, a.d_g_params, a.d_work, stream))
        for t in range(T):
            a.t = t
            rc = step_fn(ref, stream)
            if rc:
                _safelayer_native.check(rc)
            # env.step(act_safe[t]) and, in the same launch, what reset_done() returns for it (flags bit 1)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 2, spec_ref, stream)
            if rc:
                _native.check(rc)
            # thread-per-env kernels (env_num > 16384) do not speculate: reset_done as a launch of its own
            rc = commit_fn(h) if spec.value else rd_fn(h, obs_ptr, rd_ptr, stream)
            if rc:
                _native.check(rc)
        a.t = T
        _safelayer_native.check(step_fn(ref, stream))
    st.steps += T
    # as rollout_policy leaves them
    env._obs, env._reward, env._done = out['obs_last'], out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out
