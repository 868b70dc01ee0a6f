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

from . import _native, _usl_native
from .critic import HIDDEN
from .safelayer import policy_floats

# how pack_q_critic marks what it returns: c_net's input width, checked against D + A at the call
Q_CRITIC_ATTR = "gx_q_critic"


def q_floats(D, A, h):
    return h * (D + A) + h + h * h + h + h + 1


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
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    if len(lin) != 3:
        raise NotImplementedError("rollout_usl supports a c_net with two hidden layers (--l 2)")
    if [type(m) for m in mods] != [nn.Linear, nn.Tanh] * 2 + [nn.Linear]:
        raise NotImplementedError("rollout_usl supports a c_net with Tanh hidden activations (activation=nn.Tanh)")
    if lin[0].out_features != lin[1].out_features or lin[1].in_features != lin[0].out_features \
            or lin[2].in_features != lin[1].out_features:
        raise NotImplementedError("rollout_usl supports a c_net with two hidden layers of equal width")
    if lin[0].out_features not in HIDDEN:
        raise NotImplementedError(f"rollout_usl supports c_net hidden widths {HIDDEN}")
    if lin[2].out_features != 1:
        raise NotImplementedError("rollout_usl supports a c_net with one output")
    flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for m in lin for t in (m.weight, m.bias)])
    flat = flat.to(device) if device is not None else flat
    setattr(flat, Q_CRITIC_ATTR, lin[0].in_features)
    return flat


def _c_hidden(n, D, A):
    return next((h for h in HIDDEN if q_floats(D, A, h) == n), None)


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
    hc = _c_hidden(q_critic.numel(), D, A)
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


class State:
    """what the path keeps per engine: the one-set output slab of its env.step launches and its own count of policy
    steps (the noise counter: 0 at construction, + T per call, not reset by reset())"""

    def __init__(self, env):
        self.slab = env._out_slab(1)
        self.steps = 0


def rollout(env, params, T, q_critic, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0, niter=20, eta=0.05,
            grad_scale=None):
    if obs0 is None:
        obs0 = env._obs
    if obs0 is None:
        raise RuntimeError("rollout_usl() before reset()")
    N, D, A, T = env.env_num, env.obs_flat_size, env.action_space.shape[0], int(T)
    if T < 1:
        raise ValueError("rollout_usl: T must be >= 1")
    niter = int(niter)
    if niter < 0:
        raise ValueError("rollout_usl: niter must be >= 0")
    if q_critic is None or not torch.is_tensor(q_critic) or getattr(q_critic, Q_CRITIC_ATTR, None) is None:
        raise ValueError("rollout_usl needs q_critic=Engine.pack_q_critic(ac.ccritic, device=...) (the "
                         "declaration travels with the tensor pack_q_critic returns, not with copies of it)")
    params = params.to(device=env.device, dtype=torch.float32).contiguous()
    cp = q_critic.to(device=env.device, dtype=torch.float32).contiguous()
    obs0 = obs0.to(device=env.device, dtype=torch.float32).contiguous()
    if tuple(obs0.shape) != (N, D):
        raise ValueError(f"obs0 has shape {tuple(obs0.shape)}; expected {(N, D)}")
    hidden = next((h for h in HIDDEN if policy_floats(D, A, h) == params.numel()), None)
    if hidden is None:
        raise ValueError(f"params has {params.numel()} floats; expected one of "
                         f"{[policy_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN})")
    c_hidden = _c_hidden(cp.numel(), D, A)
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
    slab = st.slab
    s_obs, s_rd, s_rew, s_cost, s_done = slab[0][0], slab[1][0], slab[2][0], slab[3][0], slab[4][0]
    a = _usl_native.GxuStepArgs()
    a.struct_size = C.sizeof(_usl_native.GxuStepArgs)
    a.N, a.D, a.A, a.hidden, a.c_hidden = N, D, A, hidden, c_hidden
    a.env_offset = int(env._cfg.env_offset)
    a.T, a.t = T, 0
    a.correct, a.niter = int(bool(correct)), niter
    a.delta, a.eta = float(delta), float(eta)
    a.grad_scale = 1.0 / N if grad_scale is None else float(grad_scale)
    a.seed[0], a.seed[1] = int(noise_seed[0]) & 0xFFFFFFFF, int(noise_seed[1]) & 0xFFFFFFFF
    a.step0 = st.steps & 0xFFFFFFFF
    a.d_params, a.d_c_params, a.d_work = params.data_ptr(), cp.data_ptr(), work.data_ptr()
    a.d_obs0, a.d_obs_rd = obs0.data_ptr(), s_rd.data_ptr()
    a.d_rew_in, a.d_cost_in, a.d_done_in = s_rew.data_ptr(), s_cost.data_ptr(), s_done.data_ptr()
    for k in ('obs', 'act', 'act_safe', 'mu', 'logp', 'val', 'qc', 'iters', 'rew', 'cost', 'done', 'obs_last',
              'val_last', 'logstd'):
        setattr(a, 'd_' + k, out[k].data_ptr())
    stream = env._raw_stream(env._dev_index)
    h, ref, spec, spec_ref = env._h, C.byref(a), env._spec, env._spec_ref
    step_fn, slab_fn, commit_fn, rd_fn = lib.gxu_policy_step, env._gx_step_slab, env._gx_commit, env._lib.gx_reset_done
    act_ptr, act_stride, slab_ptr = out['act_safe'].data_ptr(), 4 * N * A, slab[6]
    obs_ptr, rd_ptr = s_obs.data_ptr(), s_rd.data_ptr()
    env._rd_obs = None
    with torch.cuda.device(env.device):
        _usl_native.check(lib.gxu_prepare(D, A, hidden, c_hidden, a.d_params, a.d_c_params, a.d_work, stream))
        for t in range(T):
            a.t = t
            rc = step_fn(ref, stream)
            if rc:
                _usl_native.check(rc)
            # env.step(act_safe[t]) and, in the same launch, what reset_done() returns for it (flags bit 1)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 2, spec_ref, stream)
            if rc:
                _native.check(rc)
            # thread-per-env kernels (env_num > 16384) do not speculate: reset_done as a launch of its own
            rc = commit_fn(h) if spec.value else rd_fn(h, obs_ptr, rd_ptr, stream)
            if rc:
                _native.check(rc)
        a.t = T
        _usl_native.check(step_fn(ref, stream))
    st.steps += T
    # as rollout_policy leaves them
    env._obs, env._reward, env._done = out['obs_last'], out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out
