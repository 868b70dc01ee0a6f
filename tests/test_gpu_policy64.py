"""The HIP policy forms against the float64 restatement of `ac.step` (oracle/policy64.py): mu, act, logp, val,
val_last, logstd and the cost critic's vc / vc_last, each evaluated by policy64 on the GPU's own recorded
observations.  Every dispatch form, env counts at the workgroup edges, the noise stream's bookkeeping (continuation,
reset_done between calls, a sharded engine) and the cost critic at unequal widths."""
import numpy as np
import pytest

from oracle import policy64
from test_policy64 import config, make_ac, critic_net, assert_saturation_crossed, report_line

pytestmark = pytest.mark.gpu

SEED = (11, 13)


def dispatch_form(robot, h, impl, N):
    """the form gx_rollout_policy runs (Engine.set_policy_impl): impl 3 always the step-wise MFMA form; width 64 the
    fused kernel (VALU with impl 1, else MFMA); wider networks in one launch (register-resident at 128, L2-streamed
    at 192 / 256) under impl 0 on the light robots at their default observation width and N <= 65536; otherwise the
    step-wise form (VALU with impl 1, else MFMA).  The engine does not report the form it ran, so this restates the
    native rule (guardx_amd/csrc/gx_api.hip, gx_rollout_policy: the fusedw / fused128 / impl choice) and must follow
    it when that rule changes."""
    if impl == 3:
        return "stepwise-mfma"
    if h == 64:
        return "fused64-valu" if impl == 1 else "fused64-mfma"
    if impl == 0 and robot in ("point", "swimmer") and N <= 65536:
        return "regs128" if h == 128 else f"stream{h}"
    return "stepwise-valu" if impl == 1 else "stepwise-mfma"


def _np(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _engine(cfg, impl=0, **kw):
    from guardx_amd import Engine
    E = Engine(cfg, n_candidates=kw.pop("n_candidates", max(40000, 100 * cfg['env_num'])), **kw)
    E.set_policy_impl(impl)
    return E


def _rollout(E, ac, T, t0, obs0=None, env_offset=0, what="", cost_critic=None):
    from guardx_amd import Engine
    params = Engine.pack_actor_critic(ac).cuda()
    vc = Engine.pack_critic(cost_critic).cuda() if cost_critic is not None else None
    g = _np(E.rollout_policy(params, T, obs0=obs0, noise_seed=SEED, cost_critic=vc))
    want = policy64.rollout(policy64.ActorCritic(ac), g, SEED, t0=t0, env_offset=env_offset, cost_critic=cost_critic)
    keys = policy64.OUTPUTS + (('vc', 'vc_last') if cost_critic is not None else ())
    report_line(what, policy64.compare(g, want, keys=keys, what=what))
    return g, want


FORM_CASES = [("fused64-valu", "point", 64, 1), ("fused64-mfma", "point", 64, 2), ("fused64-mfma", "swimmer", 64, 0),
              ("fused64-mfma", "ant", 64, 0), ("fused64-valu", "walker", 64, 1), ("fused64-mfma", "point-narrow", 64, 0),
              ("regs128", "point", 128, 0), ("regs128", "swimmer", 128, 0),
              ("stream192", "point", 192, 0), ("stream192", "swimmer", 192, 0),
              ("stream256", "point", 256, 0), ("stream256", "swimmer", 256, 0),
              ("stepwise-mfma", "point", 64, 3), ("stepwise-mfma", "config5", 64, 3),
              ("stepwise-mfma", "ant", 128, 0), ("stepwise-mfma", "walker", 256, 2),
              ("stepwise-mfma", "point-narrow", 128, 0), ("stepwise-mfma", "config5", 128, 0),
              ("stepwise-valu", "point", 128, 1), ("stepwise-valu", "ant", 192, 1), ("stepwise-valu", "walker", 128, 1),
              ("stepwise-valu", "point-narrow", 256, 1)]


@pytest.mark.parametrize("form,robot,h,impl", FORM_CASES, ids=[f"{f}-{r}-{h}" for f, r, h, _ in FORM_CASES])
def test_form_matches_policy64(form, robot, h, impl):
    """one rollout with resets inside it, a second call that continues the stream (t0 = T), then step() +
    reset_done() and a third call from its observation (obs0=; step() does not advance the stream)"""
    import torch
    N, T = 203, 12
    assert dispatch_form(robot, h, impl, N) == form
    E = _engine(config(robot, N), impl)
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac = make_ac(D, A, h, seed=h + A, shift=h // 64)
    g, want = _rollout(E, ac, T, 0, what=f"{form} {robot} h={h}")
    assert_saturation_crossed(want)
    assert g['done'][:-1].sum() > 0          # rows re-initialised by reset_done inside the rollout are among those checked
    g2, _ = _rollout(E, ac, 5, T, what="  continued")
    np.testing.assert_array_equal(g2['obs'][0], g['obs_last'])
    E.step(torch.zeros(N, A, device=E.device))
    rd = E.reset_done()
    g3, _ = _rollout(E, ac, 4, T + 5, obs0=rd, what="  after step + reset_done")
    np.testing.assert_array_equal(g3['obs'][0], rd.cpu().numpy())
    E.close()


EDGE_FORMS = [("fused64-valu", "point", 64, 1), ("fused64-mfma", "point", 64, 0), ("regs128", "point", 128, 0),
              ("stream256", "swimmer", 256, 0), ("stepwise-mfma", "ant", 128, 0), ("stepwise-valu", "point", 192, 1)]


@pytest.mark.parametrize("N", [1, 15, 16, 17, 203, 4099])
@pytest.mark.parametrize("form,robot,h,impl", EDGE_FORMS, ids=[f"{f}-{r}-{h}" for f, r, h, _ in EDGE_FORMS])
def test_env_counts_at_workgroup_edges(form, robot, h, impl, N):
    """16 envs per MFMA workgroup, 4 envs per wave in the lane-group forms: partial workgroups and waves"""
    assert dispatch_form(robot, h, impl, N) == form
    E = _engine(config(robot, N, seed=5), impl)
    E.reset()
    ac = make_ac(E.obs_flat_size, E.action_space.shape[0], h, seed=N, shift=N)
    _rollout(E, ac, 4, 0, what=f"{form} {robot} h={h} N={N}")
    E.close()


@pytest.mark.parametrize("h,form", [(64, "fused64-mfma"), (128, "regs128"), (256, "stream256")])
def test_env_limit(h, form):
    """N = 65536, the largest env count of the one-launch forms"""
    from helpers import task_config
    N = 65536
    assert dispatch_form("point", h, 0, N) == form
    over = dict(hazards_num=15, lidar_num_bins=16, placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)
    E = _engine(task_config(N, seed=8, num_steps=30, goal_size=0.9, **over), n_candidates=60000)
    E.reset(check=False)
    ac = make_ac(E.obs_flat_size, 2, h, seed=9)
    _rollout(E, ac, 2, 0, what=f"limit h={h} N={N}")
    E.close()


def test_config5_width64_is_refused_by_the_fused_kernel():
    """config 5 has 1 + 8 + 8 = 17 objects; the fused width-64 kernel serves at most 16, so rollout_policy refuses it
    with an error rather than computing something else (the step-wise form serves it: test_form_matches_policy64)"""
    from guardx_amd import Engine
    from guardx_amd._native import GxError
    E = _engine(config("config5", 16))
    E.reset()
    ac = make_ac(E.obs_flat_size, E.action_space.shape[0], 64)
    with pytest.raises(GxError, match="hazards_num <= 15"):
        E.rollout_policy(Engine.pack_actor_critic(ac).cuda(), 2, noise_seed=SEED)
    E.close()


def test_bench_shape():
    """the benchmark's shape: N = 2000, T = 200, width 64 (one fused launch)"""
    N, T = 2000, 200
    E = _engine(config("point", N, seed=2, num_steps=30))
    E.reset()
    ac = make_ac(E.obs_flat_size, 2, 64, seed=1)
    g, _ = _rollout(E, ac, T, 0, what=f"bench shape N={N} T={T}")
    assert g['done'].sum() > N
    E.close()


@pytest.mark.parametrize("robot,h,impl", [("ant", 64, 0), ("walker", 128, 1), ("point", 256, 0)])
def test_sharded_engine_uses_the_global_env_index(robot, h, impl):
    """rank 1 of 2: the noise counter's env is env_offset + i, and a second call continues at t0 = T"""
    N, T = 203, 8
    E = _engine(config(robot, N, seed=6), impl, shard=(1, 2))
    E.reset()
    ac = make_ac(E.obs_flat_size, E.action_space.shape[0], h, seed=3, shift=1)
    _rollout(E, ac, T, 0, env_offset=N, what=f"shard 1/2 {robot} h={h}")
    _rollout(E, ac, 3, T, env_offset=N, what="  continued")
    E.close()


@pytest.mark.parametrize("robot,h_pi,h_vc", [("point", 64, 256), ("point", 256, 64), ("ant", 64, 256),
                                              ("walker", 256, 64), ("config5", 128, 192)])
def test_cost_critic_matches_policy64(robot, h_pi, h_vc):
    N, T = 203, 10
    E = _engine(config(robot, N, seed=7))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac = make_ac(D, A, h_pi, seed=4)
    g, _ = _rollout(E, ac, T, 0, cost_critic=critic_net(D, h_vc, seed=12).v_net,
                    what=f"cost critic {robot} pi={h_pi} vc={h_vc}")
    assert g['done'][:-1].sum() > 0
    E.close()


@pytest.mark.parametrize("h", [64, 256])
@pytest.mark.parametrize("D", [1, 43, 70])
def test_critic_values_matches_policy64(D, h):
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    net = critic_net(D, h, seed=D).v_net
    rng = np.random.default_rng(D + h)
    x = (rng.normal(size=(3, 347, D)) * rng.choice([0.1, 1.0, 5.0], size=(3, 347, 1))).astype(np.float32)
    got = critic_values(Engine.pack_critic(net).cuda(), torch.from_numpy(x).cuda()).cpu().numpy()
    v, b = policy64.critic(net, x)
    report_line(f"critic_values D={D} h={h}", policy64.compare({'vc': got}, {'vc': v, 'vc_b': b}, keys=('vc',),
                                                                what=f"critic_values D={D} h={h}"))
