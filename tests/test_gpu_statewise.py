"""Engine.rollout_statewise (SCPO's collection loop on the device, guardx_amd/statewise.py, libguardx_statewise.so):
bit equality with rollout_policy where the two must coincide, the M channel against the numpy float32 recurrence, the
three networks with a live M column against the float64 restatement (oracle/policy64.py), the Softplus's accuracy on
its own, errors, and that the engine is left as rollout_policy leaves it."""
import math

import numpy as np
import pytest

from oracle import policy64
from helpers import task_config, assert_state_equal
from test_policy64 import ROBOTS, make_ac, critic_net, report_line

pytestmark = pytest.mark.gpu

SEED = (11, 13)

# ---------------------------------------------------------------------------------------------------------------------
# The device Softplus's error bound, derived from the constants oracle/policy64.py already carries (U, EXP_REL,
# _log_err, MARGIN), for the form the kernel evaluates (gx_statewise.hip:softplus_f):
#     x > 20:  y = x                                   exact
#     else:    u = exp_f(-|x|); w = fl(1 + u); l = (w == 1) ? u : log_f(w) * fl(u / (w - 1)); y = fl(max(x, 0) + l)
# with L = log1p(e^-|x|) <= ln 2 the exact value of l:
#   * u carries exp_f's relative error EXP_REL; dL/du = 1 / (1 + u) and u / (1 + u) <= L, so this moves l by <= EXP_REL L;
#     below exp(-87) exp_f flushes to 0: an absolute 2^-126 covers it;
#   * w - 1 is exact (w in [1, 2]); log(w) u / (w - 1) differs from log1p(u) by the relative change of log(w) / (w - 1)
#     over the rounding of 1 + u: below U; the quotient and the product are one rounding each: 3 U L together;
#   * log_f(w) is within _log_err(log w) of log w, and the factor u / (w - 1) it is multiplied by is <= 2 (w - 1 >= u / 2
#     once w > 1): 2 _log_err(L);
#   * w == 1: u < 2^-24 and l = u against log1p(u) = u - u^2 / 2 + ..: within U L;
#   * the final sum is one rounding: U |y|.
# The float64 reference switches at the same threshold, where its two branches differ by log1p(e^-20) = 2.1e-9: counted
# in, so that the bound also covers an argument that sits on the other side of 20 by its own error.
# ---------------------------------------------------------------------------------------------------------------------
THRESH_JUMP = math.log1p(math.exp(-20.0))


def softplus64(x):
    """torch.nn.Softplus(beta=1, threshold=20) in float64: x > 20 -> x, else log1p(exp(x))"""
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def softplus_bound(x):
    x = np.asarray(x, np.float64)
    L = np.log1p(np.exp(-np.abs(x)))
    y = softplus64(x)
    b = policy64.MARGIN * ((policy64.EXP_REL + 4.0 * policy64.U) * L + 2.0 * policy64._log_err(L)
                           + policy64.U * np.abs(y)) + 2.0 ** -126 + THRESH_JUMP
    return np.where(x > 20.0, THRESH_JUMP, b)


def m_recurrence(cost, done, M0, first0):
    """the M update in numpy float32, in the kernel's order of operations (include/guardx_statewise.h):
    returns cost_inc (T, N), M_after (T, N), M_in (T + 1, N) = the M column of obs[t] / obs_last, and the final
    (M, first)"""
    f = np.float32
    T, N = cost.shape
    M, first = M0.astype(f).copy(), first0.astype(bool).copy()
    inc_o, Mn_o, M_in = np.empty((T, N), f), np.empty((T, N), f), np.empty((T + 1, N), f)
    for t in range(T):
        M_in[t] = M
        c = cost[t].astype(f)
        d = (c - M).astype(f)
        inc = np.where(first, c, np.where(d > 0, d, f(0))).astype(f)
        Mn = np.where(first, c, (M + inc).astype(f)).astype(f)
        inc_o[t], Mn_o[t] = inc, Mn
        fin = done[t] > 0
        M = np.where(fin, f(0), Mn).astype(f)
        first = fin.copy()
    M_in[T] = M
    return inc_o, Mn_o, M_in, M, first


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _cfg(robot, N, seed=3, num_steps=5, **over):
    return task_config(N, seed=seed, num_steps=num_steps, goal_size=0.9, **dict(ROBOTS[robot], **over))


def _engine(cfg, **kw):
    from guardx_amd import Engine
    return Engine(cfg, n_candidates=kw.pop("n_candidates", max(40000, 100 * cfg['env_num'])), **kw)


def _softplus_critic(Da, h, seed):
    """SCPO's MLPMaxCostCritic: critic_net's layers followed by nn.Softplus; returns (module with Softplus, bare net)"""
    import torch.nn as nn
    bare = critic_net(Da, h, seed).v_net
    mods = [m for m in bare if not isinstance(m, nn.Identity)]
    return nn.Sequential(*mods, nn.Softplus()), nn.Sequential(*mods)


def _aug_ac(D, A, h, seed, shift=0, zero_m=True):
    """an SCPO-shaped actor-critic on D + 1 inputs and, with zero_m, its D-input twin (the M column dropped)"""
    import torch
    import torch.nn as nn
    from test_policy64 import Stub, two_layer_net
    ac = make_ac(D + 1, A, h, seed=seed, shift=shift)
    if not zero_m:
        return ac, None
    twin = Stub(pi=Stub(mu_net=two_layer_net(D, h, A, nn.Tanh), log_std=ac.pi.log_std), v=Stub(v_net=two_layer_net(D, h, 1, nn.Tanh)))
    with torch.no_grad():
        for src, dst in ((ac.pi.mu_net, twin.pi.mu_net), (ac.v.v_net, twin.v.v_net)):
            ls = [m for m in src if isinstance(m, nn.Linear)]
            ld = [m for m in dst if isinstance(m, nn.Linear)]
            ls[0].weight[:, D] = 0.0
            ld[0].weight.copy_(ls[0].weight[:, :D])
            ld[0].bias.copy_(ls[0].bias)
            for a, b in zip(ls[1:], ld[1:]):
                b.weight.copy_(a.weight)
                b.bias.copy_(a.bias)
    return ac, twin


TWIN_KEYS = ('act', 'mu', 'logp', 'val', 'rew', 'cost', 'done', 'val_last', 'logstd')


def _assert_twin_equal(g, w, D, what):
    np.testing.assert_array_equal(g['obs'][..., :D], w['obs'], err_msg=f"{what} obs")
    np.testing.assert_array_equal(g['obs_last'][..., :D], w['obs_last'], err_msg=f"{what} obs_last")
    for k in TWIN_KEYS:
        np.testing.assert_array_equal(g[k], w[k], err_msg=f"{what} {k}")


def _twin_runs(cfg, h, T, T2, seed, **ekw):
    """rollout_statewise on one fresh engine, rollout_policy (step-wise form) of the D-input twin on another"""
    from guardx_amd import Engine
    E, Et = _engine(cfg, **ekw), _engine(cfg, **ekw)
    Et.set_policy_impl(3)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, twin = _aug_ac(D, A, h, seed, shift=h // 64)
    vc_mod, _ = _softplus_critic(D + 1, 64 if h == 256 else 128, seed + 1)
    p, pt = Engine.pack_actor_critic(ac).cuda(), Engine.pack_actor_critic(twin).cuda()
    vc = Engine.pack_critic(vc_mod, output='softplus', device='cuda')
    runs = []
    for steps in (T, T2):
        g = _np(E.rollout_statewise(p, steps, cost_critic=vc, noise_seed=SEED))
        w = _np(Et.rollout_policy(pt, steps, noise_seed=SEED))
        runs.append((g, w))
    return E, Et, D, runs


@pytest.mark.parametrize("N", [1, 15, 16, 17, 2000])
@pytest.mark.parametrize("h", [64, 256])
@pytest.mark.parametrize("robot", ["point", "swimmer", "ant", "walker"])
def test_bit_equal_to_rollout_policy_with_a_zero_m_column(robot, h, N):
    """A zero first-layer weight on M adds exactly 0 to every hidden unit's chain, so the actor, v, the noise and the env
    must give rollout_policy's bits on the D-input twin: over resets inside the call (num_steps 5 < T) and a second call
    that continues the noise counter."""
    T, T2 = (12, 5) if N < 2000 else (8, 3)
    E, Et, D, runs = _twin_runs(_cfg(robot, N), h, T, T2, seed=h + N)
    for i, (g, w) in enumerate(runs):
        _assert_twin_equal(g, w, D, f"{robot} h={h} N={N} call {i}")
    assert runs[0][0]['done'][:-1].sum() > 0
    np.testing.assert_array_equal(runs[1][0]['obs'][0], runs[0][0]['obs_last'])
    E.close()
    Et.close()


def test_bit_equal_on_the_thread_per_env_path():
    """env_num = 20000: the step launch does not speculate reset_done (speculated == 0), gx_reset_done runs as a launch of
    its own"""
    wide = dict(placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)       # enough valid layouts for 20000 envs
    E, Et, D, runs = _twin_runs(_cfg("point", 20000, seed=4, **wide), 64, 9, 2, seed=9, n_candidates=400000)
    assert E._spec.value == 0                                                   # the launch did not speculate
    for i, (g, w) in enumerate(runs):
        _assert_twin_equal(g, w, D, f"N=20000 call {i}")
    assert runs[0][0]['done'][:-1].sum() > 0
    E.close()
    Et.close()


# hazards wider than their keep-out: robots start inside some, so costs come and go from the first step (checked on the CPU
# checker's engine: about half of all steps of every robot carry a cost); short episodes: resets inside a call
COSTLY = dict(hazards_size=0.9, hazards_keepout=0.2, num_steps=6)


def test_m_channel_exact_across_calls_and_reset():
    """cost_inc, M and the last column of obs / obs_last from the returned cost and done, bit for bit: an env done at
    t = 0 (its episode's last step is the call's first), envs never done, continuation across two calls, and a
    reset() (M back to 0, first set)"""
    import torch
    from guardx_amd import Engine
    N = 203
    E = _engine(_cfg("point", N, seed=5, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, _ = _aug_ac(D, A, 64, seed=2, zero_m=False)
    vc_mod, _ = _softplus_critic(D + 1, 64, 3)
    p, vc = Engine.pack_actor_critic(ac).cuda(), Engine.pack_critic(vc_mod, output='softplus', device='cuda')
    M, first = np.zeros(N, np.float32), np.ones(N, bool)
    seen_done0 = False
    for call, T in enumerate((6, 9, 4)):          # num_steps = 6: the time-out falls on the episode's 7th step, t = 0 of call 1
        g = _np(E.rollout_statewise(p, T, cost_critic=vc, noise_seed=SEED))
        inc, Mn, M_in, M, first = m_recurrence(g['cost'], g['done'], M, first)
        np.testing.assert_array_equal(g['cost_inc'], inc, err_msg=f"call {call}")
        np.testing.assert_array_equal(g['M'], Mn, err_msg=f"call {call}")
        np.testing.assert_array_equal(g['obs'][..., D], M_in[:T], err_msg=f"call {call}")
        np.testing.assert_array_equal(g['obs_last'][..., D], M_in[T], err_msg=f"call {call}")
        seen_done0 = seen_done0 or bool(g['done'][0].any())
        if call == 1:
            assert (g['M'] > 0).any() and (g['obs'][..., D] > 0).any() and (g['cost_inc'] < g['cost']).any()
    assert seen_done0
    assert tuple(E._obs.shape) == (N, D)
    o = E.reset()
    g = _np(E.rollout_statewise(p, 4, cost_critic=vc, noise_seed=SEED))
    np.testing.assert_array_equal(g['obs'][0][:, :D], o.cpu().numpy())
    np.testing.assert_array_equal(g['obs'][0][:, D], np.zeros(N, np.float32))
    inc, Mn, M_in, _, _ = m_recurrence(g['cost'], g['done'], np.zeros(N, np.float32), np.ones(N, bool))
    np.testing.assert_array_equal(g['cost_inc'], inc)
    np.testing.assert_array_equal(g['M'], Mn)
    np.testing.assert_array_equal(g['obs_last'][..., D], M_in[4])
    np.testing.assert_array_equal(g['cost_inc'][0], g['cost'][0])     # an episode's first step stores the whole cost
    E.close()
    # an env that is never done within the calls: long episodes, small goal
    E = _engine(task_config(64, seed=6, num_steps=500, goal_size=0.05, hazards_size=0.9, hazards_keepout=0.2))
    E.reset()
    g = _np(E.rollout_statewise(p, 12, cost_critic=vc, noise_seed=SEED))
    assert g['done'].sum() == 0 and (g['cost'] > 0).any()
    inc, Mn, M_in, _, _ = m_recurrence(g['cost'], g['done'], np.zeros(64, np.float32), np.ones(64, bool))
    np.testing.assert_array_equal(g['cost_inc'], inc)
    np.testing.assert_array_equal(g['M'], np.maximum.accumulate(g['cost'], 0))   # no reset: the running maximum itself
    np.testing.assert_array_equal(g['obs_last'][..., D], M_in[12])
    E.close()


def test_softplus_probe_within_its_derived_bound():
    """the device Softplus alone (gxs_softplus_probe) against float64 over a dense sweep of [-100, 100] and 20 +- 1 ulp;
    the bound is softplus_bound above (derivation at the top of this file).  Measured on the MI355X: largest error
    4.8e-7 (x = 14.6, half an ulp of the result), largest error / bound 0.98 at x = 8.0, where the bound (4.85e-7) is the
    final rounding alone; the identity beyond 20 is exact."""
    import torch
    from guardx_amd.statewise import softplus_probe
    x = np.concatenate([np.linspace(-100.0, 100.0, 2_000_001), np.linspace(-2.0, 2.0, 400_001),
                        np.linspace(19.0, 21.0, 200_001)]).astype(np.float32)
    t20 = np.float32(20.0)
    x = np.concatenate([x, np.array([t20, np.nextafter(t20, np.float32(0)), np.nextafter(t20, np.float32(100)), 0.0, -0.0,
                                     -87.0, -88.0, -104.0], np.float32)])
    y = softplus_probe(torch.from_numpy(x).cuda()).cpu().numpy().astype(np.float64)
    want, bound = softplus64(x), softplus_bound(x)
    err = np.abs(y - want)
    i = int(np.argmax(err / bound))
    small = x < -20
    rel_tail = float(np.max(err[small] / np.maximum(want[small], 2.0 ** -126)))
    print(f"softplus probe: {x.size} points, largest |err| {err.max():.3e} at x = {x[int(np.argmax(err))]!r}, largest "
          f"err / bound {err[i] / bound[i]:.3f} at x = {x[i]!r} (bound {bound[i]:.3e}); x > 20: largest |err| "
          f"{err[x > 20].max():.1e}; x < -20: largest relative error {rel_tail:.2e}")
    assert np.isfinite(y).all() and (y >= 0).all()
    assert (err <= bound).all(), (x[i], y[i], want[i], bound[i])
    assert (y[x > t20] == x[x > t20]).all()                      # torch's threshold: the identity beyond 20
    assert (y[(x < -20) & (x >= -87)] > 0).all()                 # the small tail is kept, not rounded to log1p(0)
    nan = softplus_probe(torch.tensor([float('nan'), float('inf'), float('-inf')], device='cuda')).cpu().numpy()
    assert np.isnan(nan[0]) and nan[1] == np.inf and nan[2] == 0.0


@pytest.mark.parametrize("robot,h,h_vc", [("point", 64, 64), ("point", 256, 128), ("swimmer", 128, 256), ("ant", 64, 192),
                                          ("ant", 256, 256), ("walker", 192, 64)])
def test_live_m_column_matches_policy64(robot, h, h_vc):
    """Random non-zero M weights.  mu, act, logp, val, val_last: policy64.rollout on the recorded (T, N, D + 1) rows with
    its own bounds.  vc, vc_last: the float64 pre-activation and its bound from policy64.mlp on the critic without its
    Softplus module, then softplus64; allowed error = that pre-activation bound (Softplus is 1-Lipschitz) + the device
    Softplus's own bound, softplus_bound at the float64 pre-activation widened by the pre-activation bound (U |y| is
    the only term that grows with x, so it is taken at |y| + the pre-activation bound)."""
    from guardx_amd import Engine
    N, T = 203, 12
    E = _engine(_cfg(robot, N, seed=7, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, _ = _aug_ac(D, A, h, seed=h + A, shift=h // 64, zero_m=False)
    vc_mod, vc_bare = _softplus_critic(D + 1, h_vc, seed=12)
    p, vc = Engine.pack_actor_critic(ac).cuda(), Engine.pack_critic(vc_mod, output='softplus', device='cuda')
    with pytest.raises(ValueError):
        policy64.layers(vc_mod)                              # (why the Softplus is stripped for policy64)
    report = {}
    t0 = 0
    for steps in (T, 5):
        g = _np(E.rollout_statewise(p, steps, cost_critic=vc, noise_seed=SEED))
        what = f"statewise {robot} h={h} vc={h_vc} t0={t0}"
        want = policy64.rollout(policy64.ActorCritic(ac), g, SEED, t0=t0)
        res = policy64.compare(g, want, what=what, report=report)
        lay = policy64.layers(vc_bare)
        worst = 0.0
        for key, rows in (('vc', g['obs']), ('vc_last', g['obs_last'])):
            pre, dpre, _ = policy64.mlp(lay, rows)
            pre, dpre = pre[..., 0], dpre[..., 0]
            bound = dpre + softplus_bound(pre) + policy64.MARGIN * policy64.U * dpre
            err = np.abs(g[key].astype(np.float64) - softplus64(pre))
            assert np.isfinite(g[key]).all() and (err <= bound).all(), (what, key, float((err / bound).max()))
            worst = max(worst, float((err / bound).max()))
            if key == 'vc':
                assert (pre > 0).any() and (pre < 0).any()    # both sides of the Softplus's knee
        res['vc'] = (worst, float(np.median(bound)))
        report_line(what, res)
        if t0 == 0:
            assert (g['obs'][..., D] > 0).any() and g['done'][:-1].sum() > 0     # a live M column, resets inside
        t0 += steps
    E.close()


def test_errors():
    import torch
    from guardx_amd import Engine
    N = 32
    E = _engine(_cfg("point", N))
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, twin = _aug_ac(D, A, 64, seed=1)
    vc_mod, vc_bare = _softplus_critic(D + 1, 64, 2)
    p = Engine.pack_actor_critic(ac).cuda()
    vc = Engine.pack_critic(vc_mod, output='softplus', device='cuda')
    with pytest.raises(RuntimeError, match="before reset"):
        E.rollout_statewise(p, 3, cost_critic=vc)
    E.reset()
    state = E.get_state()
    with pytest.raises(ValueError, match=r"params has \d+ floats; expected one of"):
        E.rollout_statewise(Engine.pack_actor_critic(twin).cuda(), 3, cost_critic=vc)      # built on D, not D + 1
    vc_d, _ = _softplus_critic(D, 64, 2)
    with pytest.raises(ValueError, match=r"cost_critic has \d+ floats; expected one of"):
        E.rollout_statewise(p, 3, cost_critic=Engine.pack_critic(vc_d, output='softplus', device='cuda'))
    with pytest.raises(ValueError, match="cost_critic"):
        E.rollout_statewise(p, 3)
    # a linear-head critic where Softplus is declared, and the reverse: the sizes agree, the declaration decides
    linear = Engine.pack_critic(vc_bare, device='cuda')
    assert linear.numel() == vc.numel()
    with pytest.raises(ValueError, match="output='identity'"):
        E.rollout_statewise(p, 3, cost_critic=linear)
    with pytest.raises(ValueError, match="output=None"):
        E.rollout_statewise(p, 3, cost_critic=vc.clone())            # a copy carries no declaration
    vc_on_d = Engine.pack_critic(vc_d, output='softplus', device='cuda')
    with pytest.raises(ValueError, match="softplus"):
        E.rollout_policy(Engine.pack_actor_critic(twin).cuda(), 3, cost_critic=vc_on_d)
    torch.cuda.synchronize()
    assert_state_equal(E.get_state(), state)                         # nothing ran
    E.close()


def test_engine_left_as_rollout_policy_leaves_it():
    """after rollout_statewise (zero M column), after rollout_policy of the twin, and after step() + reset_done() with the
    same actions, three engines hold the same state; step / reset_done on top give the same results, and so does a
    rollout_policy (whose own noise counter rollout_statewise does not advance: compared with the step()-driven engine,
    which made no policy steps either)"""
    import torch
    from guardx_amd import Engine
    N, T = 203, 9
    cfg = _cfg("ant", N, seed=8)
    E, Et, Es = _engine(cfg), _engine(cfg), _engine(cfg)
    for e in (E, Et, Es):
        e.set_policy_impl(3)
        e.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, twin = _aug_ac(D, A, 128, seed=5)
    vc_mod, _ = _softplus_critic(D + 1, 64, 6)
    pt = Engine.pack_actor_critic(twin).cuda()
    g = E.rollout_statewise(Engine.pack_actor_critic(ac).cuda(), T, noise_seed=SEED,
                            cost_critic=Engine.pack_critic(vc_mod, output='softplus', device='cuda'))
    Et.rollout_policy(pt, T, noise_seed=SEED)
    for t in range(T):
        Es.step(g['act'][t])
        rd = Es.reset_done()
    torch.cuda.synchronize()
    assert g['done'][:-1].sum().item() > 0
    assert_state_equal(E.get_state(), Et.get_state())
    assert_state_equal(E.get_state(), Es.get_state())
    np.testing.assert_array_equal(E._obs.cpu().numpy(), rd.cpu().numpy())
    for a, b in ((E._obs, Et._obs), (E._reward, Et._reward), (E._done, Et._done), (E._info['cost'], Et._info['cost'])):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    act = torch.rand(N, A, device='cuda', generator=torch.Generator(device='cuda').manual_seed(1)) * 2 - 1
    for _ in range(7):
        res = [e.step(act) for e in (E, Et, Es)]
        rds = [e.reset_done() for e in (E, Et, Es)]
        for rb, ob in zip(res[1:], rds[1:]):
            for a, b in zip(res[0][:3], rb[:3]):
                np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
            np.testing.assert_array_equal(res[0][3]['cost'].cpu().numpy(), rb[3]['cost'].cpu().numpy())
            np.testing.assert_array_equal(rds[0].cpu().numpy(), ob.cpu().numpy())
    a = _np(E.rollout_policy(pt, 5, obs0=rds[0], noise_seed=SEED))
    b = _np(Es.rollout_policy(pt, 5, obs0=rds[2], noise_seed=SEED))
    for k in a:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)
    assert_state_equal(E.get_state(), Es.get_state())
    for e in (E, Et, Es):
        e.close()


def test_statewise_rollout_batch_on_device():
    """the batch helper on a real rollout against the numpy restatement of SCPOBufferX (tests/test_statewise_host.py)"""
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import statewise_rollout_batch
    from test_statewise_host import scpo_batch_np
    N, T = 67, 24
    E = _engine(_cfg("point", N, seed=9, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, _ = _aug_ac(D, A, 64, seed=3, zero_m=False)
    vc_mod, _ = _softplus_critic(D + 1, 64, 4)
    out = E.rollout_statewise(Engine.pack_actor_critic(ac).cuda(), T, noise_seed=SEED,
                              cost_critic=Engine.pack_critic(vc_mod, output='softplus', device='cuda'))
    g = _np(out)
    assert g['done'][:-1].sum() > 0 and (g['cost_inc'] != g['M']).any()
    for signal in ('increment', 'reference'):
        got = _np(statewise_rollout_batch(out, cost_signal=signal))
        want = scpo_batch_np(g, signal)
        assert set(got) == set(want)
        for k in want:
            tol = 2e-4 if k in ('adv', 'adc') else 2e-5
            np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=tol, err_msg=f"{signal} {k}")
    E.close()
