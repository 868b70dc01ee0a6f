"""The policy layer against its float64 restatement (oracle/policy64.py): hand-worked cases, the Threefry noise
pinned on published known answers, the checker's rollout_policy on every robot and width, and the packing's
rejection of actor-critics the kernels would evaluate differently."""
import math

import numpy as np
import pytest

from helpers import task_config, SWIMMER, ANT, WALKER
from oracle import policy64
from test_oracle_prng import KAT

LOG_STD_CYCLE = (-5.0, -0.5, 0.0, 1.5)
SAT = 9.0           # |x| beyond which the fp32 tanh is +-1


def two_layer_net(D, h, out, act, out_act=None):
    """a network with the module structure of the learner's MLPs at hidden_sizes (h, h): Linear(D, h), act,
    Linear(h, h), act, Linear(h, out), then the output activation (Identity unless given)"""
    import torch.nn as nn
    return nn.Sequential(nn.Linear(D, h), act(), nn.Linear(h, h), act(), nn.Linear(h, out), (out_act or nn.Identity)())


class Stub:
    """what MLPActorCritic looks like from outside: .pi.mu_net, .pi.log_std, .v.v_net"""
    def __init__(self, **kw):
        self.__dict__.update(kw)


def log_std_for(A, shift=0):
    """per-dimension distinct values around -5, -0.5, 0, 1.5 (rolled by `shift`)"""
    import torch
    return torch.tensor([LOG_STD_CYCLE[(d + shift) % 4] + 0.01 * (d // 4) for d in range(A)], dtype=torch.float32)


def make_ac(D, A, h, seed=0, shift=0, activation=None):
    """an actor-critic (h, h) whose hidden pre-activations cross the tanh saturation at |x| = 9 on both sides"""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    activation = activation or nn.Tanh
    mu_net, v_net = two_layer_net(D, h, A, activation), two_layer_net(D, h, 1, activation)
    with torch.no_grad():
        for net in (mu_net, v_net):
            lin = [m for m in net if isinstance(m, nn.Linear)]
            nn.init.normal_(lin[0].weight, std=4.0 / math.sqrt(D))
            nn.init.normal_(lin[0].bias, std=4.0)
            nn.init.normal_(lin[1].weight, std=6.0 / math.sqrt(h))
            nn.init.normal_(lin[1].bias, std=2.0)
            nn.init.normal_(lin[2].weight, std=1.0 / math.sqrt(h))
            nn.init.normal_(lin[2].bias, std=0.5)
    return Stub(pi=Stub(mu_net=mu_net, log_std=log_std_for(A, shift)), v=Stub(v_net=v_net))


def critic_net(D, h, seed):
    return make_ac(D, 1, h, seed=seed).v


def assert_saturation_crossed(want):
    for pre in want['pre']:
        frac = float((np.abs(pre) > SAT).mean())
        assert 0.02 < frac < 0.98, frac


def report_line(what, res):
    print(what + "  " + "  ".join(f"{k} {r:.3f} ({b:.2e})" for k, (r, b) in res.items()))


# ---------------------------------------------------------------------------------------------------------------------
# hand-worked cases
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("key,ctr,want", KAT)
def test_threefry_known_answers(key, ctr, want):
    y0, y1 = policy64.threefry2x32(key[0], key[1], ctr[0], ctr[1])
    assert (int(y0), int(y1)) == want


def test_known_block_gives_known_normals():
    # block (0x6b200159, 0x99ba4efe) of key (0, 0), counter (0, 0) [Random123 known answer]:
    #   b0 >> 8 = 7020545 -> u1 = 7020546 / 2^24 = 0.41845715045928955
    #   b1 >> 8 = 10074702 -> u2 = 10074702 / 2^24 = 0.6004990339279175
    #   r = sqrt(-2 ln u1) = 1.3201..., 2 pi u2 = 3.7731... rad (third quadrant: both negative)
    z0, z1, b = policy64.normal_pair((0, 0), 0, 0)
    assert abs(float(z0) - -1.0654526572765741) < 1e-14
    assert abs(float(z1) - -0.7792125515346809) < 1e-14
    assert 0 < float(b) < 2e-6
    # pair p of step s of env i is block (i, 16 s + p): dims 2p, 2p + 1
    z, _ = policy64.noise((0, 0), 0, 0, 2)
    np.testing.assert_array_equal(z, [z0, z1])
    z, _ = policy64.noise((5, 6), [3], [7], 6)
    for p in range(3):
        w0, w1, _ = policy64.normal_pair((5, 6), 3, 7 * 16 + p)
        np.testing.assert_array_equal(z[0, 2 * p:2 * p + 2], [w0, w1])


def test_zero_hidden_weights_give_output_bias(oracle):
    import torch
    from guardx_amd import Engine
    O = oracle.OracleEngine(task_config(5, seed=1), n_candidates=20000)
    o0 = O.reset()
    ac = make_ac(O.D, O.na, 64, seed=1)
    with torch.no_grad():
        for net in (ac.pi.mu_net, ac.v.v_net):
            for m in list(net)[:4]:
                if isinstance(m, torch.nn.Linear):
                    m.weight.zero_()
                    m.bias.zero_()
    b3, b3v = ac.pi.mu_net[4].bias.detach().numpy(), float(ac.v.v_net[4].bias.detach())
    w = policy64.ActorCritic(ac).step(o0, (1, 2), np.arange(5), 0)
    np.testing.assert_array_equal(w['mu'], np.broadcast_to(b3.astype(np.float64), (5, 2)))
    np.testing.assert_array_equal(w['val'], np.full(5, b3v))
    out = O.rollout_policy(Engine.pack_actor_critic(ac).numpy(), 3, o0, noise_seed=(1, 2))
    np.testing.assert_array_equal(out['mu'], np.broadcast_to(b3, (3, 5, 2)))
    np.testing.assert_array_equal(out['val'], np.full((3, 5), b3v, np.float32))


@pytest.mark.parametrize("A", [2, 8, 10])
def test_logp_at_the_mean(A):
    ls = log_std_for(A).double().numpy()
    mu = np.random.default_rng(A).normal(size=(3, A))
    want = -ls.sum() - A * math.log(math.sqrt(2 * math.pi))
    np.testing.assert_allclose(policy64.gaussian_logp(mu, mu, ls), want, rtol=0, atol=1e-12)
    # one standard deviation off in one dim costs exactly 1/2
    a = mu.copy()
    a[:, A - 1] += np.exp(ls[A - 1])
    np.testing.assert_allclose(policy64.gaussian_logp(a, mu, ls), want - 0.5, rtol=0, atol=1e-12)


def test_policy64_matches_torch_distribution():
    """the restatement against torch's own Normal / Sequential in float64 (not part of its inputs: the weights are)"""
    import torch
    ac = make_ac(46, 2, 64, seed=3)
    obs = np.random.default_rng(1).normal(size=(50, 46)).astype(np.float32)
    w = policy64.ActorCritic(ac).step(obs, (9, 9), np.arange(50), 4)
    with torch.no_grad():
        x = torch.from_numpy(obs).double()
        mu = ac.pi.mu_net.double()(x)
        std = torch.exp(ac.pi.log_std.double())
        pi = torch.distributions.Normal(mu, std)
        logp = pi.log_prob(torch.from_numpy(w['act'])).sum(-1)
        v = ac.v.v_net.double()(x).squeeze(-1)
    np.testing.assert_allclose(w['mu'], mu.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(w['logp'], logp.numpy(), rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(w['val'], v.numpy(), rtol=1e-12, atol=1e-12)


def test_bounds_are_not_vacuous():
    """the bound is tight enough that a one-ulp-of-fp32-per-layer restatement sits well inside it, and far below
    what a wrong pair / row / log_std changes"""
    ac = make_ac(70, 10, 256, seed=4)
    obs = np.random.default_rng(2).normal(size=(200, 70)).astype(np.float32)
    w = policy64.ActorCritic(ac).step(obs, (1, 1), np.arange(200), 3)
    assert np.median(w['mu_b']) < 1e-3 and np.median(w['act_b']) < 2e-3 and np.median(w['logp_b']) < 1e-3
    assert np.median(w['val_b']) < 1e-3 and np.max(w['logstd_b']) < 1e-6 and np.max(w['z_b']) < 1e-5


# ---------------------------------------------------------------------------------------------------------------------
# the checker against policy64
# ---------------------------------------------------------------------------------------------------------------------
ROBOTS = {"point": {}, "point-narrow": {"lidar_num_bins": 8}, "swimmer": SWIMMER, "ant": ANT, "walker": WALKER}


def config(robot, N, seed=3, num_steps=5):
    if robot == "config5":
        from guardx_amd import configuration
        cfg = dict(configuration("Ant_8Hazards_8Pillars_synthetic"))
        cfg.update(env_num=N, _seed=seed, num_steps=num_steps, goal_size=2.4)
        return cfg
    return task_config(N, seed=seed, num_steps=num_steps, goal_size=0.9, **ROBOTS[robot])


CHECKER_CASES = [("point", 64), ("point", 128), ("point", 192), ("point", 256), ("swimmer", 64), ("swimmer", 192),
                 ("ant", 64), ("ant", 256), ("walker", 128), ("walker", 192), ("point-narrow", 64),
                 ("point-narrow", 256), ("config5", 64), ("config5", 128)]


@pytest.mark.parametrize("robot,h", CHECKER_CASES)
def test_checker_matches_policy64(oracle, robot, h):
    from guardx_amd import Engine
    N, T = 24, 10
    O = oracle.OracleEngine(config(robot, N), n_candidates=30000)
    o0 = O.reset()
    D, A = O.D, O.na
    ac = make_ac(D, A, h, seed=h + A, shift=h // 64)
    params = Engine.pack_actor_critic(ac).numpy()
    out = O.rollout_policy(params, T, o0, noise_seed=(21, 22), hidden=h)
    assert out['done'][:-1].sum() > 0                    # rows re-initialised by reset_done inside the rollout
    ref = policy64.ActorCritic(ac)
    want = policy64.rollout(ref, out, (21, 22))
    assert_saturation_crossed(want)
    report_line(f"checker {robot} h={h}", policy64.compare(out, want, what=f"checker {robot} h={h}"))
    # the continuation: t0 = T
    out2 = O.rollout_policy(params, 4, out['obs_last'], noise_seed=(21, 22), t0=T, hidden=h)
    policy64.compare(out2, policy64.rollout(ref, out2, (21, 22), t0=T), what="continued")


def test_checker_sharded_matches_policy64(oracle):
    """rank 1 of 2: the noise counter takes the global env index"""
    from guardx_amd import Engine
    N, T = 16, 6
    O = oracle.OracleEngine(config("ant", N), n_candidates=30000, env_total=2 * N, env_offset=N)
    o0 = O.reset()
    ac = make_ac(O.D, O.na, 64, seed=7, shift=1)
    out = O.rollout_policy(Engine.pack_actor_critic(ac).numpy(), T, o0, noise_seed=(4, 5), t0=3)
    policy64.compare(out, policy64.rollout(policy64.ActorCritic(ac), out, (4, 5), t0=3, env_offset=N), what="shard")


# ---------------------------------------------------------------------------------------------------------------------
# packing
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_actor_critic_layout_follows_the_modules():
    import torch
    from guardx_amd import Engine
    ac = make_ac(46, 2, 64, seed=2)
    flat = Engine.pack_actor_critic(ac)
    want = [t.detach().reshape(-1) for net in (ac.pi.mu_net, ac.v.v_net) for m in net
            if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)] + [ac.pi.log_std]
    assert torch.equal(flat, torch.cat(want))
    # nets built without the trailing Identity are the same network
    bare = Stub(pi=Stub(mu_net=torch.nn.Sequential(*list(ac.pi.mu_net)[:5]), log_std=ac.pi.log_std),
                v=Stub(v_net=torch.nn.Sequential(*list(ac.v.v_net)[:5])))
    assert torch.equal(Engine.pack_actor_critic(bare), flat)


@pytest.mark.parametrize("what", ["relu", "elu", "mixed", "out-tanh", "out-relu", "log_std-short", "log_std-long",
                                  "input-widths", "critic-outputs"])
def test_pack_actor_critic_rejects_what_the_kernels_would_not_compute(what):
    import torch
    import torch.nn as nn
    from guardx_amd import Engine
    D, A, h = 43, 2, 64
    if what == "relu":
        ac = make_ac(D, A, h, activation=nn.ReLU)
    elif what == "elu":
        ac = make_ac(D, A, h, activation=nn.ELU)
    else:
        ac = make_ac(D, A, h)
    if what == "mixed":
        ac.v.v_net[3] = nn.ReLU()
    elif what == "out-tanh":
        ac.pi.mu_net = two_layer_net(D, h, A, nn.Tanh, nn.Tanh)
    elif what == "out-relu":
        ac.v.v_net = two_layer_net(D, h, 1, nn.Tanh, nn.ReLU)
    elif what == "log_std-short":
        ac.pi.log_std = torch.zeros(A - 1)
    elif what == "log_std-long":
        ac.pi.log_std = torch.zeros(A + 2)
    elif what == "input-widths":
        ac.v.v_net = two_layer_net(D + 3, h, 1, nn.Tanh)
    elif what == "critic-outputs":
        ac.v.v_net = two_layer_net(D, h, 2, nn.Tanh)
    with pytest.raises(NotImplementedError):
        Engine.pack_actor_critic(ac)
    with pytest.raises(NotImplementedError):
        Engine.pack_actor_critic(mu_net=ac.pi.mu_net, v_net=ac.v.v_net, log_std=ac.pi.log_std)


@pytest.mark.parametrize("h", [64, 128, 192, 256])
def test_pack_actor_critic_accepts_the_default_structure(h):
    import torch.nn as nn
    from guardx_amd import Engine
    ac = make_ac(70, 10, h, activation=nn.Tanh)
    assert Engine.pack_actor_critic(ac).numel() == Engine._policy_floats(70, 10, h)
