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

The host side is _closed_loop's: the per-engine State with its Book (the first-done bookkeeping), the loop
(run_episode) and the tail probe.  What is this path's own: gxe_step_args carries the bookkeeping pointers and t_base
itself, where the other libraries take a gx_first_done_state, and the tail has the optional vc_last.
"""
from . import _closed_loop as _cl, _episode_native
from ._closed_loop import policy_floats  # noqa: F401 (part of this module's surface)
from .critic import critic_hidden

State = _cl.State


def tail_probe(params, rows, act_dim, cost_critic=None):
    """The tail of a call alone on `rows` (n, D), a float32 device tensor (gxe_tail_probe): -> obs_last (the rows as
    they are), val_last and, with cost_critic, vc_last: the critics on the rows, 0 for a row with a non-finite entry."""
    _cl.refuse_softplus("tail_probe", cost_critic)
    lib = _episode_native.load()
    return _cl.tail_probe("tail_probe", params, rows, act_dim, cost_critic, lambda n, D, A: critic_hidden(D, n),
                          lib.gxe_work_floats, lib.gxe_prepare, lib.gxe_tail_probe, _episode_native.check, vc_last=True)


def rollout(env, params, T, obs0=None, noise_seed=(0, 0), cost_critic=None):
    obs0, N, D, A, T = _cl.begin(env, "rollout_episode", obs0, T)
    vcp, vc_hidden = _cl.linear_cost_critic("rollout_episode", cost_critic, D, env.device)
    has_vc = vcp is not None
    params, _, obs0, hidden = _cl.device_inputs(env, params, None, obs0, D, A)
    if not has_vc:
        vcp, vc_hidden = params[_cl.net_floats(D, A, hidden):], hidden     # the value network's block stands in
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
    a.D, a.hidden, a.vc_hidden, a.has_vc = D, hidden, vc_hidden, int(has_vc)
    a.d_vc_params = vcp.data_ptr()

    def prepare(stream):
        return lib.gxe_prepare(D, A, hidden, vc_hidden, a.d_params, a.d_vc_params, a.d_work, stream)

    return _cl.run_episode(env, st, a, out, T, prepare, lib.gxe_policy_step, _episode_native.check, out['act'],
                           book_in_args=True)
