"""The USL rollout on the device: `Engine.rollout_usl` (safe_rl_libX/usl/usl.py:478-553 with the actor-critic and the
C_Critic of usl_core.py:146-196, 239-248 evaluated there).

The learner evaluates a cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) next to ac.step and, after its warm-up,
walks the action down Q's gradient before env.step sees it: up to niter passes of
a = a - eta s / (max |s| + 1e-8), s = grad_scale dQ/da, while max a <= 1 and Q > delta.  Per control step: one
`gxu_policy_step` launch (libguardx_usl.so, include/guardx_usl.h: ac.step, Q on the sampled action, the iteration with
its forward and backward passes on the MFMA chains) and one `gx_step_slab` launch on act_safe[t] (env.step with the
speculated reset_done, committed on the host) -- the two launches per control step the step-wise rollout_policy already
has.  Everything runs on torch's current stream; nothing synchronises.

Two quirks of the reference, kept in the open (include/guardx_usl.h):
  * usl_core.py:184 backpropagates pred.mean(), so its gradient is the true one divided by the batch size; the division
    by max |s| takes the factor out again except against the 1e-8.  grad_scale=None means 1 / env_num, the reference's
    arithmetic for an unsharded engine; grad_scale=1.0 is the unscaled form.
  * usl_core.py:174-175 tests the SIGNED maximum, max_k a[k] > 1, not |a|: a component below -1 does not stop a row.
"""
import ctypes as C

import torch

from . import _closed_loop as _cl, _usl_native
from ._closed_loop import policy_floats, q_floats  # noqa: F401 (part of this module's surface)
from .critic import HIDDEN

# how pack_q_critic marks what it returns: c_net's input width, checked against D + A at the call
Q_CRITIC_ATTR = "gx_q_critic"


def pack_q_critic(ccritic, device=None):
    """Flatten USL's cost critic (`ac.ccritic` of usl_core.py:146-151: anything with .c_net, or the nn.Sequential
    Linear/Tanh/Linear/Tanh/Linear/Softplus itself) into W1 b1 W2 b2 W3 b3, float32.  Anything the kernel would evaluate
    differently raises NotImplementedError.  The returned tensor carries c_net's input width (Q_CRITIC_ATTR), which the
    rollout checks against its engine's D + A; copies of the tensor do not carry it."""
    nn = torch.nn
    net = getattr(ccritic, 'c_net', ccritic)
    mods = [m for m in net if not isinstance(m, nn.Identity)]
    last = mods[-1] if mods else None
    if not isinstance(last, nn.Softplus):
        raise NotImplementedError("rollout_usl supports a c_net whose output activation is nn.Softplus")
    if last.beta != 1 or last.threshold != 20:
        raise NotImplementedError("rollout_usl supports nn.Softplus(beta=1, threshold=20)")
    mods = mods[:-1]
    lin = _cl.two_tanh_layers(mods, "rollout_usl", "c_net", " (activation=nn.Tanh)")
    if lin[2].out_features != 1:
        raise NotImplementedError("rollout_usl supports a c_net with one output")
    flat = _cl.flatten(lin, device)
    setattr(flat, Q_CRITIC_ATTR, lin[0].in_features)
    return flat


def correction_probe(q_critic, obs, act, delta=0.0, niter=20, eta=0.05, grad_scale=1.0):
    """the iteration alone as the kernel evaluates it (gxu_correction_probe): q_critic from pack_q_critic, obs (n, D)
    and act (n, A) float32 device tensors -> dict a_safe (n, A), q0 (n,), grad0 (n, A) [the scaled gradient of the first
    pass, 0 for a row that stops before it], iters (n,) int32 [updates applied], stop (n,) int32 [0 niter exhausted,
    1 max a > 1, 2 q <= delta]"""
    for t in (q_critic, obs, act):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise ValueError("correction_probe: q_critic, obs and act must be float32 device tensors")
    if obs.dim() != 2 or act.dim() != 2 or obs.shape[0] != act.shape[0]:
        raise ValueError("correction_probe: obs must be (n, D) and act (n, A)")
    if int(niter) < 0:
        raise ValueError("correction_probe: niter must be >= 0")
    n, D = obs.shape
    A = act.shape[1]
    if n >= 2 ** 31:
        raise ValueError("correction_probe: more than 2^31 - 1 rows")
    if getattr(q_critic, Q_CRITIC_ATTR, D + A) != D + A:
        raise ValueError(f"correction_probe: q_critic reads {getattr(q_critic, Q_CRITIC_ATTR)} inputs, obs and act have {D} + {A}")
    hc = _cl.q_hidden(q_critic.numel(), D, A)
    if hc is None:
        raise ValueError(f"q_critic has {q_critic.numel()} floats; expected one of {[q_floats(D, A, h) for h in HIDDEN]} "
                         f"(hidden {HIDDEN}) for {D} + {A} inputs")
    cp, obs, act = q_critic.contiguous(), obs.contiguous(), act.contiguous()
    lib = _usl_native.load()
    dev = obs.device
    nw = int(lib.gxu_probe_work_floats(D, A, hc))
    if nw < 0:
        raise NotImplementedError(f"correction_probe supports an even action width <= 16, not {A}")
    work = torch.empty(nw, dtype=torch.float32, device=dev)
    out = dict(a_safe=torch.empty_like(act), q0=torch.empty(n, dtype=torch.float32, device=dev),
               grad0=torch.empty_like(act), iters=torch.empty(n, dtype=torch.int32, device=dev),
               stop=torch.empty(n, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _usl_native.check(lib.gxu_correction_probe(
            n, D, A, hc, cp.data_ptr(), work.data_ptr(), obs.data_ptr(), act.data_ptr(), float(delta), int(niter),
            float(eta), float(grad_scale), out['a_safe'].data_ptr(), out['q0'].data_ptr(), out['grad0'].data_ptr(),
            out['iters'].data_ptr(), out['stop'].data_ptr(), C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index))))
    return out


State = _cl.State


def rollout(env, params, T, q_critic, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0, niter=20, eta=0.05,
            grad_scale=None):
    obs0, N, D, A, T = _cl.begin(env, "rollout_usl", obs0, T)
    niter = int(niter)
    if niter < 0:
        raise ValueError("rollout_usl: niter must be >= 0")
    if q_critic is None or not torch.is_tensor(q_critic) or getattr(q_critic, Q_CRITIC_ATTR, None) is None:
        raise ValueError("rollout_usl needs q_critic=Engine.pack_q_critic(ac.ccritic, device=...) (the "
                         "declaration travels with the tensor pack_q_critic returns, not with copies of it)")
    params, cp, obs0, hidden = _cl.device_inputs(env, params, q_critic, obs0, D, A)
    c_hidden = _cl.q_hidden(cp.numel(), D, A)
    if c_hidden is None or getattr(q_critic, Q_CRITIC_ATTR) != D + A:
        raise ValueError(f"q_critic has {cp.numel()} floats and reads {getattr(q_critic, Q_CRITIC_ATTR)} inputs; expected "
                         f"one of {[q_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN}) for {D} + {A} inputs")
    lib = _usl_native.load()
    st = env._usl
    if st is None:
        st = env._usl = State(env)
    new = env._new
    out = dict(obs=new(T, N, D), act=new(T, N, A), act_safe=new(T, N, A), mu=new(T, N, A),
               logp=new(T, N), val=new(T, N), qc=new(T, N), iters=new(T, N), rew=new(T, N), cost=new(T, N),
               done=new(T, N), obs_last=new(N, D), val_last=new(N), logstd=new(A))
    work = new(int(lib.gxu_work_floats(D, A, hidden, c_hidden)))
    a = _usl_native.GxuStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0)
    a.D, a.hidden, a.c_hidden = D, hidden, c_hidden
    a.correct, a.niter = int(bool(correct)), niter
    a.delta, a.eta = float(delta), float(eta)
    a.grad_scale = 1.0 / N if grad_scale is None else float(grad_scale)
    a.d_c_params = cp.data_ptr()

    def prepare(stream):
        return lib.gxu_prepare(D, A, hidden, c_hidden, a.d_params, a.d_c_params, a.d_work, stream)

    _cl.run(env, st, a, out, T, prepare, lib.gxu_policy_step, _usl_native.check, out['act_safe'])
    return out
