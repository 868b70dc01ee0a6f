"""The safety-layer rollout on the device: `Engine.rollout_safelayer` (safe_rl_libX/safelayer/safelayer.py:514-581 with
the actor-critic and the C_Critic of safelayer_core.py:147-190 evaluated there; Dalal et al. 2018).

The learner edits the action between ac.step and env.step: a_safe = a - relu((g.a + prev_c - delta) / (g.g + 1e-8)) g,
clamped to [-1, 1], where pred = g.a + prev_c exceeds delta; g = g_net(obs) and prev_c is the cost of the env's previous
step (0 after a done or a reset()).  prev_c depends on the cost of the step just made, so it sits inside the closed
loop.  Per control step: one `gxl_policy_step` launch (libguardx_safelayer.so, include/guardx_safelayer.h: the prev_c
update of the step just made, ac.step, g_net, the correction) and one `gx_step_slab` launch on act_safe[t] (env.step with
the speculated reset_done, committed on the host) -- the two launches per control step the step-wise rollout_policy
already has.  Everything runs on torch's current stream; nothing synchronises.

episode=True is the collection loop of `safelayer_one_episode` (safelayer_one_episode/safelayer.py:493-590): no
reset_done, the rows sanitised, the first-done bookkeeping, prev_c = the step's cost whatever `done` says
(guardx_safelayer_policy_step_episode and a plain env.step per control step; _closed_loop.run_episode).
"""
import ctypes as C

import torch

from . import _closed_loop as _cl, _safelayer_native
from ._closed_loop import policy_floats  # noqa: F401 (part of this module's surface)
from .critic import HIDDEN

# how pack_g_net marks what it returns (a g_net and another A-output network of the same size look alike)
G_NET_ATTR = "gx_g_net"


def g_floats(D, A, h):
    return _cl.net_floats(D, A, h)


def pack_g_net(ccritic, device=None):
    """Flatten the safety layer's g_net (`ac.ccritic` of safelayer_core.py:147-156: anything with .g_net, or the
    nn.Sequential Linear/Tanh/Linear/Tanh/Linear[/Identity] itself) into W1 b1 W2 b2 W3 b3, float32.  Anything the kernel
    would evaluate differently raises NotImplementedError."""
    net = getattr(ccritic, 'g_net', ccritic)
    lin = _cl.two_tanh_layers([m for m in net if not isinstance(m, torch.nn.Identity)], "rollout_safelayer", "g_net",
                              " and a linear output only (activation=nn.Tanh, output_activation=nn.Identity)")
    A = lin[2].out_features
    if A < 2 or A > 16 or A % 2:
        raise NotImplementedError(f"rollout_safelayer supports an even action width <= 16; g_net has {A} outputs")
    flat = _cl.flatten(lin, device)
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


class State(_cl.State):
    """the slab and the noise counter of _closed_loop.State, and prev_c (N,)"""

    def __init__(self, env):
        self.prev_c = torch.zeros(env.env_num, dtype=torch.float32, device=env.device)
        super().__init__(env)

    def reset(self):
        self.prev_c.zero_()    # safelayer.py:567


def tail_probe(params, rows, act_dim, g_net):
    """the tail of an episode=True call alone on `rows` (n, D) (guardx_safelayer_tail_probe): -> obs_last (raw), val_last"""
    lib = _safelayer_native.load()
    return _cl.tail_probe("tail_probe", params, rows, act_dim, g_net, lambda n, D, A: _cl.hidden_of(n, lambda h: g_floats(D, A, h)),
                          lib.gxl_work_floats, lib.gxl_prepare, lib.guardx_safelayer_tail_probe, _safelayer_native.check)


def rollout(env, params, T, g_net, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0, episode=False):
    obs0, N, D, A, T = _cl.begin(env, "rollout_safelayer", obs0, T)
    if g_net is None or not torch.is_tensor(g_net) or getattr(g_net, G_NET_ATTR, None) is None:
        raise ValueError("rollout_safelayer needs g_net=Engine.pack_g_net(ac.ccritic, device=...) (the declaration "
                         "travels with the tensor pack_g_net returns, not with copies of it)")
    params, gp, obs0, hidden = _cl.device_inputs(env, params, g_net, obs0, D, A)
    g_hidden = _cl.hidden_of(gp.numel(), lambda h: g_floats(D, A, h))
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
    a = _safelayer_native.GxlStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0)
    a.D, a.hidden, a.g_hidden = D, hidden, g_hidden
    a.correct, a.delta = int(bool(correct)), float(delta)
    a.d_g_params = gp.data_ptr()
    a.d_prev_c = st.prev_c.data_ptr()

    def prepare(stream):
        return lib.gxl_prepare(D, A, hidden, g_hidden, a.d_params, a.d_g_params, a.d_work, stream)

    if episode:
        return _cl.run_episode(env, st, a, out, T, prepare, lib.guardx_safelayer_policy_step_episode, _safelayer_native.check, out['act_safe'])
    _cl.run(env, st, a, out, T, prepare, lib.gxl_policy_step, _safelayer_native.check, out['act_safe'])
    return out
