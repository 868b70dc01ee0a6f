"""What the closed-loop rollouts with a third network share (statewise.py, safelayer.py, usl.py): the sizes of the packed
networks, the checks of the inputs, the common fields of a gx?_step_args, the loop itself -- per control step the
path's policy-step launch and one `gx_step_slab` launch (env.step with the speculated reset_done, committed on the
host) -- and what the loop leaves on the engine, which is what rollout_policy leaves.
"""
import ctypes as C

import torch

from . import _native
from .critic import HIDDEN


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


class State:
    """what a path keeps per engine: the one-set output slab of its env.step launches and its own count of policy steps
    (the noise counter: 0 at construction, + T per call, not reset by reset())"""

    def __init__(self, env):
        self.slab = env._out_slab(1)
        self.steps = 0

    def reset(self):
        pass


def begin(env, name, obs0, T):
    """-> obs0 (the engine's when None), N, D, A, T"""
    if obs0 is None:
        obs0 = env._obs
    if obs0 is None:
        raise RuntimeError(f"{name}() before reset()")
    T = int(T)
    if T < 1:
        raise ValueError(f"{name}: T must be >= 1")
    return obs0, env.env_num, env.obs_flat_size, env.action_space.shape[0], T


def device_inputs(env, params, third, obs0, Din, A, tail=""):
    """params, the third network and obs0 as contiguous float32 tensors on the engine's device, and the policy's hidden
    width, read off its size for Din inputs"""
    params, third, obs0 = (t.to(device=env.device, dtype=torch.float32).contiguous() for t in (params, third, obs0))
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
