"""What the closed-loop rollouts share (Engine.rollout_policy and pack_actor_critic; statewise.py, safelayer.py, usl.py,
lpg.py; episode.py and the one-episode form of safelayer, usl and lpg: Book, run_episode, tail_probe): the sizes of
the packed networks, the checks of the networks and of the inputs (for the two learners with a Q critic, usl.py and
lpg.py, also those of their probes and the tensors their rollouts return), the common fields of a gx?_step_args, the
loop itself -- per control step the path's policy-step launch and one `gx_step_slab` launch (env.step with the
speculated reset_done, committed on the host; a plain env.step in the one-episode form) -- and what the loop leaves on
the engine, which is what rollout_policy leaves.
"""
import ctypes as C

import torch

from . import _native
from ._sidelib import FirstDoneState
from .critic import HIDDEN, critic_floats, critic_hidden


def net_floats(D, out, h):
    """floats of one packed network: W1[h][D] b1[h] W2[h][h] b2[h] W3[out][h] b3[out]"""
    return h * D + h + h * h + h + out * h + out


def policy_floats(D, A, h):
    """pack_actor_critic: mu_net, v_net, log_std"""
    return net_floats(D, A, h) + net_floats(D, 1, h) + A


def hidden_of(n, floats):
    """the hidden width h for which a packed network has floats(h) == n floats (unique: the size grows with h), or None"""
    return next((h for h in HIDDEN if floats(h) == n), None)


def q_floats(D, A, h):
    """pack_q_critic: c_net of the USL and the LPG learners, one output on D + A inputs"""
    return net_floats(D + A, 1, h)


def q_hidden(n, D, A):
    """c_net's hidden width, read off the size of the packed tensor, or None"""
    return hidden_of(n, lambda h: q_floats(D, A, h))


# how pack_q_critic marks what it returns: c_net's input width, checked against D + A at the call
Q_CRITIC_ATTR = "gx_q_critic"


def _listed(parts):
    return ", ".join(parts[:-1]) + " and " + parts[-1]


def q_probe_inputs(name, q_critic, obs, act, extra=()):
    """The checks of a Q critic's probe `name` on q_critic, obs (n, D), act (n, A) and the per-row tensors `extra`
    ((argument name, tensor (n,)), ...) -> q_critic, obs, act contiguous, n, D, A and c_net's hidden width"""
    names = ["q_critic", "obs", "act"] + [k for k, _ in extra]
    for t in [q_critic, obs, act] + [v for _, v in extra]:
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32):
            raise ValueError(f"{name}: {_listed(names)} must be float32 device tensors")
    if obs.dim() != 2 or act.dim() != 2 or obs.shape[0] != act.shape[0] \
            or any(tuple(v.shape) != (obs.shape[0],) for _, v in extra):
        raise ValueError(f"{name}: " + _listed(["obs must be (n, D)", "act (n, A)"] + [k + " (n,)" for k, _ in extra]))
    n, D = obs.shape
    A = act.shape[1]
    if n >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 rows")
    if getattr(q_critic, Q_CRITIC_ATTR, D + A) != D + A:
        raise ValueError(f"{name}: q_critic reads {getattr(q_critic, Q_CRITIC_ATTR)} inputs, obs and act have {D} + {A}")
    hc = q_hidden(q_critic.numel(), D, A)
    if hc is None:
        raise ValueError(f"q_critic has {q_critic.numel()} floats; expected one of {[q_floats(D, A, h) for h in HIDDEN]} "
                         f"(hidden {HIDDEN}) for {D} + {A} inputs")
    return q_critic.contiguous(), obs.contiguous(), act.contiguous(), n, D, A, hc


def q_probe_work(name, floats, A, device):
    """the probe's scratch of `floats` = gx?_probe_work_floats(...) floats"""
    if floats < 0:
        raise NotImplementedError(f"{name} supports an even action width <= 16, not {A}")
    return torch.empty(floats, dtype=torch.float32, device=device)


def q_rollout_inputs(env, name, params, q_critic, obs0, T):
    """The checks of a rollout `name` with a Q critic -> params, q_critic and obs0 on the engine's device, N, D, A, T, the
    policy's hidden width and c_net's"""
    obs0, N, D, A, T = begin(env, name, obs0, T)
    if q_critic is None or not torch.is_tensor(q_critic) or getattr(q_critic, Q_CRITIC_ATTR, None) is None:
        raise ValueError(f"{name} needs q_critic=Engine.pack_q_critic(ac.ccritic, device=...) (the "
                         "declaration travels with the tensor pack_q_critic returns, not with copies of it)")
    params, cp, obs0, hidden = device_inputs(env, params, q_critic, obs0, D, A)
    c_hidden = q_hidden(cp.numel(), D, A)
    if c_hidden is None or getattr(q_critic, Q_CRITIC_ATTR) != D + A:
        raise ValueError(f"q_critic has {cp.numel()} floats and reads {getattr(q_critic, Q_CRITIC_ATTR)} inputs; expected "
                         f"one of {[q_floats(D, A, h) for h in HIDDEN]} (hidden {HIDDEN}) for {D} + {A} inputs")
    return params, cp, obs0, N, D, A, T, hidden, c_hidden


def q_rollout_out(env, T, N, D, A, own):
    """what both rollouts with a Q critic return, and the path's own (T, N) tensor `own`"""
    new = env._new
    out = dict(obs=new(T, N, D), act=new(T, N, A), act_safe=new(T, N, A), mu=new(T, N, A), logp=new(T, N), val=new(T, N),
               qc=new(T, N), rew=new(T, N), cost=new(T, N), done=new(T, N), obs_last=new(N, D), val_last=new(N),
               logstd=new(A))
    out[own] = new(T, N)
    return out


def two_tanh_layers(mods, who, net="", tanh_tail=""):
    """The three Linear modules of `mods` = Linear/Tanh/Linear/Tanh/Linear with hidden layers of one width of HIDDEN;
    anything else raises NotImplementedError in the words of `who` (and of its network `net`, when it names one)."""
    nn = torch.nn
    a_net, net_ = (f"a {net} with ", net + " ") if net else ("", "")
    lin = [m for m in mods if isinstance(m, nn.Linear)]
    if len(lin) != 3:
        raise NotImplementedError(f"{who} supports {a_net}two hidden layers (--l 2)")
    if [type(m) for m in mods] != [nn.Linear, nn.Tanh] * 2 + [nn.Linear]:
        raise NotImplementedError(f"{who} supports {a_net}Tanh hidden activations{tanh_tail}")
    if lin[0].out_features != lin[1].out_features or lin[1].in_features != lin[0].out_features \
            or lin[2].in_features != lin[1].out_features:
        raise NotImplementedError(f"{who} supports {a_net}two hidden layers of equal width")
    if lin[0].out_features not in HIDDEN:
        raise NotImplementedError(f"{who} supports {net_}hidden widths {HIDDEN}")
    return lin


def flatten(lin, device):
    """W1 b1 W2 b2 W3 b3, float32"""
    flat = torch.cat([t.detach().reshape(-1).to(torch.float32) for m in lin for t in (m.weight, m.bias)])
    return flat.to(device) if device is not None else flat


def refuse_softplus(who, cost_critic):
    """`who` evaluates its cost critic with a linear output (pack_critic's declaration travels with the tensor)"""
    if getattr(cost_critic, 'gx_output', None) == 'softplus':
        raise ValueError(f"{who} evaluates the cost critic with a linear output; cost_critic was packed with "
                         "output='softplus' (SCPO's MLPMaxCostCritic: use rollout_statewise)")


def linear_cost_critic(who, cost_critic, D, device):
    """The cost critic of rollout_policy and rollout_episode: -> the packed critic as a contiguous float32 tensor on the
    device and its hidden width, (None, None) without one"""
    if cost_critic is None:
        return None, None
    refuse_softplus(who, cost_critic)
    vcp = cost_critic.to(device=device, dtype=torch.float32).contiguous()
    vc_hidden = critic_hidden(D, vcp.numel())
    if vc_hidden is None:
        raise ValueError(f"cost_critic has {vcp.numel()} floats; expected one of "
                         f"{[critic_floats(D, h) for h in HIDDEN]} (hidden {HIDDEN})")
    return vcp, vc_hidden


class Book:
    """the first-done bookkeeping of a one-episode rollout (rollout_episode, episode=True): per env first_done / ep_len
    (int32), ep_ret / ep_cost (float32), and the number of steps the episode has made (t_base)"""

    def __init__(self, env):
        N = env.env_num
        self.ints = torch.zeros(2, N, dtype=torch.int32, device=env.device)      # [0] = first_done, [1] = ep_len
        self.sums = torch.zeros(2, N, dtype=torch.float32, device=env.device)    # [0] = ep_ret, [1] = ep_cost
        self.t_base = 0

    def reset(self):
        self.ints.zero_()
        self.sums.zero_()
        self.t_base = 0

    def c_struct(self):
        b = FirstDoneState()
        b.struct_size, b.t_base = C.sizeof(b), self.t_base
        b.d_first_done, b.d_ep_len = self.ints[0].data_ptr(), self.ints[1].data_ptr()
        b.d_ep_ret, b.d_ep_cost = self.sums[0].data_ptr(), self.sums[1].data_ptr()
        return b


class State:
    """what a path keeps per engine: the one-set output slab of its env.step launches, its own count of policy steps
    (the noise counter: 0 at construction, + T per call, not reset by reset()) and, once a one-episode call was made,
    that form's bookkeeping (`book`: advanced by one-episode calls of the path alone).  Engine.reset() calls reset(),
    which a path with state of its own overrides, and reset_book()."""
    book = None

    def __init__(self, env):
        self.slab = env._out_slab(1)
        self.steps = 0

    def reset(self):
        pass

    def reset_book(self):
        if self.book is not None:
            self.book.reset()


def begin(env, name, obs0, T, check_T=True):
    """-> obs0 (the engine's when None), N, D, A, T; check_T=False leaves T < 1 to the library's own refusal"""
    if obs0 is None:
        obs0 = env._obs
    if obs0 is None:
        raise RuntimeError(f"{name}() before reset()")
    T = int(T)
    if check_T and T < 1:
        raise ValueError(f"{name}: T must be >= 1")
    return obs0, env.env_num, env.obs_flat_size, env.action_space.shape[0], T


def device_inputs(env, params, third, obs0, Din, A, tail=""):
    """params, the third network (None where the path has none to move) and obs0 as contiguous float32 tensors on the
    engine's device, and the policy's hidden width, read off its size for Din inputs"""
    params, third, obs0 = (t if t is None else t.to(device=env.device, dtype=torch.float32).contiguous()
                           for t in (params, third, obs0))
    N, D = env.env_num, env.obs_flat_size
    if tuple(obs0.shape) != (N, D):
        raise ValueError(f"obs0 has shape {tuple(obs0.shape)}; expected {(N, D)}")
    hidden = hidden_of(params.numel(), lambda h: policy_floats(Din, A, h))
    if hidden is None:
        raise ValueError(f"params has {params.numel()} floats; expected one of "
                         f"{[policy_floats(Din, A, h) for h in HIDDEN]} (hidden {HIDDEN}){tail}")
    return params, third, obs0, hidden


def fill(a, env, st, out, T, noise_seed, params, work, obs0, rename=()):
    """the fields every gx?_step_args has; out[k] goes to d_<k> unless `rename` says otherwise"""
    rename = dict(rename)
    a.struct_size = C.sizeof(a)
    a.N, a.A = env.env_num, env.action_space.shape[0]
    a.env_offset = int(env._cfg.env_offset)
    a.T, a.t = T, 0
    a.seed[0], a.seed[1] = int(noise_seed[0]) & 0xFFFFFFFF, int(noise_seed[1]) & 0xFFFFFFFF
    a.step0 = st.steps & 0xFFFFFFFF
    slab = st.slab
    a.d_params, a.d_work, a.d_obs0 = params.data_ptr(), work.data_ptr(), obs0.data_ptr()
    a.d_obs_rd, a.d_rew_in, a.d_cost_in, a.d_done_in = (slab[i][0].data_ptr() for i in (1, 2, 3, 4))
    fields = {f[0] for f in a._fields_}
    for k, v in out.items():
        field = rename.get(k, 'd_' + k)
        if field not in fields:      # setattr would make a plain attribute of it and leave the kernel a null pointer
            raise KeyError(f"{type(a).__name__} has no field {field} for out['{k}']")
        setattr(a, field, v.data_ptr())


def run(env, st, a, out, T, prepare, step_fn, check, act):
    """prepare(stream), then T x (step_fn -> env.step(act[t]) -> reset_done) and the closing step_fn at t = T, on torch's
    current stream; `check` raises on a status of the path's library, `act` (T, N, A) is what env.step consumes."""
    slab = st.slab
    stream = env._raw_stream(env._dev_index)
    h, ref, spec, spec_ref = env._h, C.byref(a), env._spec, env._spec_ref
    slab_fn, commit_fn, rd_fn = env._gx_step_slab, env._gx_commit, env._lib.gx_reset_done
    act_ptr, act_stride, slab_ptr = act.data_ptr(), 4 * act.shape[1] * act.shape[2], slab[6]
    obs_ptr, rd_ptr = slab[0][0].data_ptr(), slab[1][0].data_ptr()
    env._rd_obs = None
    with torch.cuda.device(env.device):
        check(prepare(stream))
        for t in range(T):
            a.t = t
            rc = step_fn(ref, stream)
            if rc:
                check(rc)
            # env.step(act[t]) and, in the same launch, what reset_done() returns for it (flags bit 1)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 2, spec_ref, stream)
            if rc:
                _native.check(rc)
            # thread-per-env kernels (env_num > 16384) do not speculate: reset_done as a launch of its own
            rc = commit_fn(h) if spec.value else rd_fn(h, obs_ptr, rd_ptr, stream)
            if rc:
                _native.check(rc)
        a.t = T
        check(step_fn(ref, stream))
    st.steps += T
    # as rollout_policy leaves them
    env._obs, env._reward, env._done = out['obs_last'], out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out


def run_episode(env, st, a, out, T, prepare, step_fn, check, act, book_in_args=False):
    """The one-episode form of run(): prepare(stream), then T x (step_fn -> env.step(act[t])) and the closing step_fn at
    t = T.  No reset_done: the env launch is a plain step (flags = 0, nothing speculated, nothing committed) and the
    policy step reads the env's plain observation, set 0 of the slab.  step_fn(args, book, stream) takes the path's
    bookkeeping as a gx_first_done_state; book_in_args: step_fn(args, stream), and `a` has the same five fields itself
    (gxe_step_args).  Adds the copies of the bookkeeping and t0 to `out`; the engine is left as after a step()."""
    book = st.book
    if book is None:
        book = st.book = Book(env)
    slab = st.slab
    a.d_obs_rd = slab[0][0].data_ptr()     # a flags = 0 step writes no obs_rd piece
    b = book.c_struct()
    stream = env._raw_stream(env._dev_index)
    h, ref, spec_ref = env._h, C.byref(a), env._spec_ref
    if book_in_args:
        for f in ('t_base', 'd_first_done', 'd_ep_len', 'd_ep_ret', 'd_ep_cost'):
            setattr(a, f, getattr(b, f))
        step_args = (ref, stream)
    else:
        step_args = (ref, C.byref(b), stream)
    slab_fn = env._gx_step_slab
    act_ptr, act_stride, slab_ptr = act.data_ptr(), 4 * act.shape[1] * act.shape[2], slab[6]
    env._rd_obs = None
    with torch.cuda.device(env.device):
        check(prepare(stream))
        for t in range(T):
            a.t = t
            rc = step_fn(*step_args)
            if rc:
                check(rc)
            rc = slab_fn(h, act_ptr + t * act_stride, slab_ptr, 0, 0, spec_ref, stream)   # env.step(act[t]), nothing else
            if rc:
                _native.check(rc)
        a.t = T
        check(step_fn(*step_args))
    out['t0'] = book.t_base
    st.steps += T
    book.t_base += T
    out['first_done'], out['ep_len'] = book.ints.clone().unbind(0)
    out['ep_ret'], out['ep_cost'] = book.sums.clone().unbind(0)
    # as a step() leaves them
    env._obs, env._reward, env._done = out['obs_last'], out['rew'][-1], out['done'][-1]
    env._info = {'cost': out['cost'][-1]}
    return out


def tail_probe(name, params, rows, act_dim, third, third_hidden, work_floats, prepare_fn, probe_fn, check, vc_last=False):
    """The tail of a one-episode call alone on `rows` (n, D), a float32 device tensor, through a library's tail probe:
    -> obs_last (the rows as they are) and val_last (the critic on the sanitised rows, 0 for a row with a non-finite
    entry).  third: the packed third network; third_hidden(floats, D, A) its hidden width or None.  vc_last: the third
    network is a cost critic that may be absent (None: the value network's block of `params` stands in) and whose values
    on the rows the probe returns as vc_last (gxe_tail_probe: has_vc after the widths, d_vc_last after d_val_last)."""
    if not (torch.is_tensor(rows) and rows.is_cuda and rows.dtype == torch.float32 and rows.dim() == 2):
        raise ValueError(f"{name}: rows must be a float32 (n, D) device tensor")
    rows = rows.contiguous()
    n, D = rows.shape
    A = int(act_dim)
    if n >= 2 ** 31:
        raise ValueError(f"{name}: more than 2^31 - 1 rows")
    params = params.to(device=rows.device, dtype=torch.float32).contiguous()
    absent = vc_last and third is None      # only gxe_tail_probe's cost critic may be
    if not absent:
        third = third.to(device=rows.device, dtype=torch.float32).contiguous()
    hidden = hidden_of(params.numel(), lambda h: policy_floats(D, A, h))
    h3 = hidden if absent else third_hidden(third.numel(), D, A)
    if hidden is None or h3 is None:
        raise ValueError(f"{name}: {'params' if hidden is None else 'cost_critic' if vc_last else 'the third network'} "
                         f"does not fit {D} inputs, {A} actions and a hidden width of {HIDDEN}")
    if absent:
        third = params[net_floats(D, A, hidden):]
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=rows.device)   # noqa: E731
    out = dict(obs_last=new(n, D), val_last=new(n))
    flag, vc_ptr = (), ()
    if vc_last:
        if not absent:
            out['vc_last'] = new(n)
        flag, vc_ptr = (int(not absent),), (None if absent else out['vc_last'].data_ptr(),)
    work = new(int(work_floats(D, A, hidden, h3)))
    stream = C.c_void_p(torch._C._cuda_getCurrentRawStream(rows.device.index))
    with torch.cuda.device(rows.device):
        check(prepare_fn(D, A, hidden, h3, params.data_ptr(), third.data_ptr(), work.data_ptr(), stream))
        check(probe_fn(n, D, A, hidden, h3, *flag, params.data_ptr(), third.data_ptr(), work.data_ptr(), rows.data_ptr(),
                       out['obs_last'].data_ptr(), out['val_last'].data_ptr(), *vc_ptr, stream))
    return out
