"""The USL rollout on the device: `Engine.rollout_usl` (safe_rl_libX/usl/usl.py:478-553 with the actor-critic and the
C_Critic of usl_core.py:146-196, 239-248 evaluated there).

The learner evaluates a cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) next to ac.step and, after its warm-up,
walks the action down Q's gradient before env.step sees it: up to niter passes of
a = a - eta acc / (max |acc| + 1e-8), acc the running sum of the passes' s = grad_scale dQ/da, while max a <= 1 and
Q > delta.  Per control step: one
`gxu_policy_step` launch (libguardx_usl.so, include/guardx_usl.h: ac.step, Q on the sampled action, the iteration with
its forward and backward passes on the MFMA chains) and one `gx_step_slab` launch on act_safe[t] (env.step with the
speculated reset_done, committed on the host) -- the two launches per control step the step-wise rollout_policy already
has.  Everything runs on torch's current stream; nothing synchronises.

Three quirks of the reference, kept in the open (include/guardx_usl.h):
  * usl_core.py:184 backpropagates pred.mean(), so its gradient is the true one divided by the batch size; the division
    by max |s| takes the factor out again except against the 1e-8.  grad_scale=None means 1 / env_num, the reference's
    arithmetic for an unsharded engine; grad_scale=1.0 is the unscaled form.
  * usl_core.py:174-175 tests the SIGNED maximum, max_k a[k] > 1, not |a|: a component below -1 does not stop a row.
  * usl_core.py:180-194 never clears act.grad, so every backward() adds to it: the step of pass p follows the sum of the
    scaled gradients of the passes 1 .. p, not the gradient at the current action.
"""
import ctypes as C

import torch

from . import _closed_loop as _cl, _usl_native
from ._closed_loop import Q_CRITIC_ATTR, policy_floats, q_floats  # noqa: F401 (part of this module's surface)


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
    cp, obs, act, n, D, A, hc = _cl.q_probe_inputs("correction_probe", q_critic, obs, act)
    if int(niter) < 0:
        raise ValueError("correction_probe: niter must be >= 0")
    lib = _usl_native.load()
    dev = obs.device
    work = _cl.q_probe_work("correction_probe", int(lib.gxu_probe_work_floats(D, A, hc)), A, dev)
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


def tail_probe(params, rows, act_dim, q_critic):
    """the tail of an episode=True call alone on `rows` (n, D) (guardx_usl_tail_probe): -> obs_last (raw), val_last"""
    lib = _usl_native.load()
    return _cl.tail_probe("tail_probe", params, rows, act_dim, q_critic, _cl.q_hidden, lib.gxu_work_floats, lib.gxu_prepare,
                          lib.guardx_usl_tail_probe, _usl_native.check)


def rollout(env, params, T, q_critic, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0, niter=20, eta=0.05,
            grad_scale=None, episode=False):
    params, cp, obs0, N, D, A, T, hidden, c_hidden = _cl.q_rollout_inputs(env, "rollout_usl", params, q_critic, obs0, T)
    niter = int(niter)
    if niter < 0:
        raise ValueError("rollout_usl: niter must be >= 0")
    lib = _usl_native.load()
    st = env._usl
    if st is None:
        st = env._usl = State(env)
    out = _cl.q_rollout_out(env, T, N, D, A, 'iters')
    work = env._new(int(lib.gxu_work_floats(D, A, hidden, c_hidden)))
    a = _usl_native.GxuStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0)
    a.D, a.hidden, a.c_hidden = D, hidden, c_hidden
    a.correct, a.niter = int(bool(correct)), niter
    a.delta, a.eta = float(delta), float(eta)
    a.grad_scale = 1.0 / N if grad_scale is None else float(grad_scale)
    a.d_c_params = cp.data_ptr()

    def prepare(stream):
        return lib.gxu_prepare(D, A, hidden, c_hidden, a.d_params, a.d_c_params, a.d_work, stream)

    if episode:   # usl_one_episode/usl.py:454-554: no reset_done, the rows sanitised, the first-done bookkeeping
        return _cl.run_episode(env, st, a, out, T, prepare, lib.guardx_usl_policy_step_episode, _usl_native.check, out['act_safe'])
    _cl.run(env, st, a, out, T, prepare, lib.gxu_policy_step, _usl_native.check, out['act_safe'])
    return out
