"""The LPG rollout on the device: `Engine.rollout_lpg` (safe_rl_libX/lpg/lpg.py:486-564 with the actor-critic and the
C_Critic of lpg_core.py:148-198, 224-233 evaluated there).

The learner evaluates USL's cost critic Q(obs, act) = Softplus(c_net(cat(obs, act))) next to ac.step, keeps
Q_init = Q(o, a) of the epoch's first step per env, and, after its warm-up, projects the action before env.step sees it:
rows with Q(obs, act) > delta get a + lam G with G = grad_scale dQ(obs, 0)/da, the gradient at the ZERO action, and
lam = max((G . a - |delta - Q_init|) / (G . G), 0).  Per control step: one `gxp_policy_step` launch (libguardx_lpg.so,
include/guardx_lpg.h: ac.step, Q on the sampled action, the zero pass with its backward pass, the projection) and one
`gx_step_slab` launch on act_safe[t] -- the two launches per control step the step-wise rollout_policy already has.
Everything runs on torch's current stream; nothing synchronises.

The reference's quirks, kept in the open (include/guardx_lpg.h lists all six):
  * lpg_core.py:178 backpropagates pred_0.mean(), so G is the true gradient divided by the batch size, and here the
    factor does not cancel.  grad_scale=None means 1 / env_num, the reference's arithmetic for an unsharded engine;
    grad_scale=1.0 is the unscaled form.
  * lpg_core.py:195 adds lam G (up the gradient): step_sign=+1.0 is the reference as written, -1.0 the other sign.
  * lpg_core.py:193 hard-codes act_dim == 2; lam multiplies every component of G here.
  * the reference's lam is float64 numpy; the device works in float32.
  * no guard on G . G == 0: a zero gradient gives lam = 0 (a_safe = act) when |delta - Q_init| > 0 and a NaN action when
    it is 0 / 0, which the env's NaN guard handles.
"""
import ctypes as C

import torch

from . import _closed_loop as _cl, _lpg_native


def projection_probe(q_critic, obs, act, q_init, delta=0.0, grad_scale=1.0, step_sign=1.0):
    """the projection alone as the kernel evaluates it (gxp_projection_probe): q_critic from pack_q_critic, obs (n, D),
    act (n, A) and q_init (n,) float32 device tensors -> dict a_safe (n, A), q (n,) [Q(obs, act)], G (n, A) [the scaled
    gradient at the zero action, every row], lam (n,) [0 for branch 0], branch (n,) int32 [0 q <= delta, 1 corrected
    with lam > 0, 2 corrected with lam clipped to 0 or NaN]"""
    cp, obs, act, n, D, A, hc = _cl.q_probe_inputs("projection_probe", q_critic, obs, act, extra=(("q_init", q_init),))
    q_init = q_init.contiguous()
    lib = _lpg_native.load()
    dev = obs.device
    work = _cl.q_probe_work("projection_probe", int(lib.gxp_probe_work_floats(D, A, hc)), A, dev)
    out = dict(a_safe=torch.empty_like(act), q=torch.empty(n, dtype=torch.float32, device=dev),
               G=torch.empty_like(act), lam=torch.empty(n, dtype=torch.float32, device=dev),
               branch=torch.empty(n, dtype=torch.int32, device=dev))
    with torch.cuda.device(dev):
        _lpg_native.check(lib.gxp_projection_probe(
            n, D, A, hc, cp.data_ptr(), work.data_ptr(), obs.data_ptr(), act.data_ptr(), q_init.data_ptr(), float(delta),
            float(grad_scale), float(step_sign), out['a_safe'].data_ptr(), out['q'].data_ptr(), out['G'].data_ptr(),
            out['lam'].data_ptr(), out['branch'].data_ptr(), C.c_void_p(torch._C._cuda_getCurrentRawStream(dev.index))))
    return out


class State(_cl.State):
    """the shared state plus q_init: Q(o, a) of the epoch's first step, one float per env (C_Critic.Q_init).  Zero at
    construction, written by a call with store_init=True, kept across calls, reset() and done envs"""

    def __init__(self, env):
        super().__init__(env)
        self.q_init = env._new(env.env_num).zero_()


def tail_probe(params, rows, act_dim, q_critic):
    """the tail of an episode=True call alone on `rows` (n, D) (guardx_lpg_tail_probe): -> obs_last (raw), val_last"""
    lib = _lpg_native.load()
    return _cl.tail_probe("tail_probe", params, rows, act_dim, q_critic, _cl.q_hidden, lib.gxp_work_floats, lib.gxp_prepare,
                          lib.guardx_lpg_tail_probe, _lpg_native.check)


def rollout(env, params, T, q_critic, obs0=None, noise_seed=(0, 0), correct=True, delta=0.0, store_init=True,
            grad_scale=None, step_sign=1.0, episode=False):
    params, cp, obs0, N, D, A, T, hidden, c_hidden = _cl.q_rollout_inputs(env, "rollout_lpg", params, q_critic, obs0, T)
    lib = _lpg_native.load()
    st = env._lpg
    if st is None:
        st = env._lpg = State(env)
    out = _cl.q_rollout_out(env, T, N, D, A, 'lam')
    work = env._new(int(lib.gxp_work_floats(D, A, hidden, c_hidden)))
    a = _lpg_native.GxpStepArgs()
    _cl.fill(a, env, st, out, T, noise_seed, params, work, obs0)
    a.D, a.hidden, a.c_hidden = D, hidden, c_hidden
    a.correct, a.store_init = int(bool(correct)), int(bool(store_init))
    a.delta, a.step_sign = float(delta), float(step_sign)
    a.grad_scale = 1.0 / N if grad_scale is None else float(grad_scale)
    a.d_c_params, a.d_q_init = cp.data_ptr(), st.q_init.data_ptr()

    def prepare(stream):
        return lib.gxp_prepare(D, A, hidden, c_hidden, a.d_params, a.d_c_params, a.d_work, stream)

    if episode:   # lpg_one_episode/lpg.py:464-565: no reset_done, the rows sanitised, the first-done bookkeeping
        _cl.run_episode(env, st, a, out, T, prepare, lib.guardx_lpg_policy_step_episode, _lpg_native.check, out['act_safe'])
    else:
        _cl.run(env, st, a, out, T, prepare, lib.gxp_policy_step, _lpg_native.check, out['act_safe'])
    out['q_init'] = st.q_init.clone()   # the values this call used (stream-ordered after its launches)
    return out
