"""The cost critic `ac.vc` of the CPO-family learners on the device (libguardx_critic.so, guardx_amd.critic):
Engine.pack_critic, rollout_policy(..., cost_critic=) -> vc / vc_last, critic_values, cost_rollout_batch.

The value head never influences the trajectory, so a rollout whose `v` slot carries the cost critic's weights follows
the same trajectory and returns Vc as its `val`: the fused kernels and the CPU checker are the reference for vc."""
import numpy as np
import pytest

from helpers import task_config, assert_state_equal, SWIMMER, ANT, WALKER

ROBOTS = {"point": {}, "swimmer": SWIMMER, "ant": ANT, "walker": WALKER}


def _net(D, out, h, seed):
    import torch
    torch.manual_seed(seed)
    net = torch.nn.Sequential(torch.nn.Linear(D, h), torch.nn.Tanh(), torch.nn.Linear(h, h), torch.nn.Tanh(),
                              torch.nn.Linear(h, out), torch.nn.Identity())
    for m in net:                      # livelier than the default init so tanh is exercised
        if isinstance(m, torch.nn.Linear):
            torch.nn.init.normal_(m.weight, std=0.5 * (64 / h) ** 0.5 if m.in_features == h else 0.5)
            torch.nn.init.normal_(m.bias, std=0.3)
    return net


class _VC:                             # what cpo_core.py's MLPCritic looks like from outside: .v_net
    def __init__(self, net):
        self.v_net = net


def _log_std(A):
    import torch
    return torch.tensor([-0.5, -0.3, -0.7, -0.1, -0.9, -0.4, -0.6, -0.2, -0.8, -0.35][:A])


# ---------------------------------------------------------------------------------------------------------------------
# an independent restatement of the arithmetic contract in numpy: fmaf exactly (the product is exact in float64, the sum
# rounded to odd, then once to float32), the checker's tanh (oracle.math_probe2), the 16-partial butterfly head
# ---------------------------------------------------------------------------------------------------------------------
def _fmaf(a, b, c):
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float64) for v in (a, b, c)))
    p = a * b
    with np.errstate(invalid='ignore', over='ignore'):
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fix = np.isfinite(s) & np.isfinite(err) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def _tanh(oracle, x):
    return oracle.math_probe2(x.reshape(-1))[1].reshape(x.shape)


def _vc_numpy(oracle, params, x):
    x = np.asarray(x, np.float32)
    M, D = x.shape
    n = params.size
    h = next(h for h in (64, 128, 192, 256) if h * D + 3 * h + h * h + 1 == n)
    W1 = params[:h * D].reshape(h, D); b1 = params[h * D:h * D + h]
    o = h * D + h
    W2 = params[o:o + h * h].reshape(h, h); b2 = params[o + h * h:o + h * h + h]
    o += h * h + h
    W3, b3 = params[o:o + h], params[o + h]
    acc = np.broadcast_to(b1, (M, h)).astype(np.float32)
    for k in range(D):
        acc = _fmaf(x[:, k:k + 1], W1[None, :, k], acc)
    h1 = _tanh(oracle, acc)
    acc = np.broadcast_to(b2, (M, h)).astype(np.float32)
    for k in range(h):
        acc = _fmaf(h1[:, k:k + 1], W2[None, :, k], acc)
    h2 = _tanh(oracle, acc)
    pl = np.zeros((M, 16), np.float32)
    for lane in range(16):
        for c in range(h // 64):
            for j in range(4):
                u = 64 * c + 4 * lane + j
                pl[:, lane] = _fmaf(h2[:, u], W3[u], pl[:, lane])
    for off in (8, 4, 2, 1):
        pl = (pl + pl[:, np.arange(16) ^ off]).astype(np.float32)
    return (np.float32(b3) + pl[:, 0]).astype(np.float32)


def _oracle_rows(oracle, cfg, vc_net, rows, hidden):
    """Vc(rows) through the checker: a T = 1 oracle rollout whose obs0 is the rows, with an actor of vc's width and vc
    in the v slot (val[0] = Vc(obs0))"""
    from guardx_amd import Engine
    N, D = rows.shape
    O = oracle.OracleEngine(dict(cfg, env_num=N), n_candidates=40000)
    O.reset()
    A = O.na
    p = Engine.pack_actor_critic(mu_net=_net(D, A, hidden, 77), v_net=vc_net, log_std=_log_std(A)).numpy()
    return O.rollout_policy(p, 1, rows, noise_seed=(1, 2), hidden=hidden)['val'][0]


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_pack_critic_layout_and_rejections():
    import torch
    from guardx_amd import Engine
    net = _net(43, 1, 128, 3)
    flat = Engine.pack_critic(_VC(net))
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    want = torch.cat([t.detach().reshape(-1) for m in lin for t in (m.weight, m.bias)])
    assert flat.dtype == torch.float32 and flat.numel() == 128 * 43 + 128 + 128 * 128 + 128 + 128 + 1
    assert torch.equal(flat, want) and torch.equal(Engine.pack_critic(net), want)
    from guardx_amd.critic import critic_hidden
    assert critic_hidden(43, flat.numel()) == 128
    L, Th = torch.nn.Linear, torch.nn.Tanh
    bad = {
        "one hidden layer": torch.nn.Sequential(L(43, 64), Th(), L(64, 1)),
        "three hidden layers": torch.nn.Sequential(L(43, 64), Th(), L(64, 64), Th(), L(64, 64), Th(), L(64, 1)),
        "unequal widths": torch.nn.Sequential(L(43, 64), Th(), L(64, 128), Th(), L(128, 1)),
        "width 96": torch.nn.Sequential(L(43, 96), Th(), L(96, 96), Th(), L(96, 1)),
        "ReLU": torch.nn.Sequential(L(43, 64), torch.nn.ReLU(), L(64, 64), torch.nn.ReLU(), L(64, 1)),
        "output activation": torch.nn.Sequential(L(43, 64), Th(), L(64, 64), Th(), L(64, 1), Th()),
        "two outputs": torch.nn.Sequential(L(43, 64), Th(), L(64, 64), Th(), L(64, 2)),
    }
    for why, net in bad.items():
        with pytest.raises(NotImplementedError):
            Engine.pack_critic(net)
            pytest.fail(why)


def test_pack_actor_critic_still_ignores_vc():
    from guardx_amd import Engine

    class AC:
        pass
    ac = AC()
    ac.pi, ac.v, ac.vc = AC(), _VC(_net(43, 1, 64, 1)), _VC(_net(43, 1, 256, 2))
    ac.pi.mu_net, ac.pi.log_std = _net(43, 2, 64, 0), _log_std(2)
    assert Engine.pack_actor_critic(ac).numel() == Engine._policy_floats(43, 2, 64)


@pytest.fixture(scope="module")
def critic_lib():
    from guardx_amd import build, _critic_native
    build.build()
    return _critic_native.load()


def test_critic_sizes_and_bad_arguments_are_errors_not_crashes(critic_lib):
    from guardx_amd import _critic_native as n
    lib = critic_lib
    for D in (1, 43, 80):
        for h in (64, 128, 192, 256):
            assert lib.gxc_critic_floats(D, h) == h * D + h + h * h + h + h + 1
            assert lib.gxc_critic_work_floats(D, h) == ((D + 3) // 4 * 4) * h + h * h
    assert lib.gxc_critic_floats(43, 96) == -1 and lib.gxc_critic_floats(0, 64) == -1
    assert lib.gxc_critic_work_floats(43, 32) == -1
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call
    assert lib.gxc_critic_values(4, 43, 64, None, fake, fake, fake, None) == n.GXC_ERR_ARG
    assert b"null" in lib.gxc_last_error()
    assert lib.gxc_critic_values(4, 43, 64, fake, None, fake, fake, None) == n.GXC_ERR_ARG
    assert lib.gxc_critic_values(4, 43, 64, fake, fake, None, fake, None) == n.GXC_ERR_ARG
    assert lib.gxc_critic_values(4, 43, 64, fake, fake, fake, None, None) == n.GXC_ERR_ARG
    assert lib.gxc_critic_values(-1, 43, 64, fake, fake, fake, fake, None) == n.GXC_ERR_ARG
    assert lib.gxc_critic_values(4, 0, 64, fake, fake, fake, fake, None) == n.GXC_ERR_ARG
    assert lib.gxc_critic_values(4, -3, 64, fake, fake, fake, fake, None) == n.GXC_ERR_ARG
    for h in (0, 32, 96, 512, -64):
        assert lib.gxc_critic_values(4, 43, h, fake, fake, fake, fake, None) == n.GXC_ERR_UNSUPPORTED
    assert b"hidden" in lib.gxc_last_error()
    assert lib.gxc_critic_values(4, 5000, 256, fake, fake, fake, fake, None) == n.GXC_ERR_UNSUPPORTED
    assert lib.gxc_critic_values(0, 43, 64, fake, fake, fake, fake, None) == n.GXC_OK   # M == 0: nothing to do


@pytest.mark.parametrize("h", [64, 128, 256])
def test_numpy_restatement_equals_the_checker(oracle, h):
    """the numpy restatement used below for widths no task produces is the checker's arithmetic, bit for bit"""
    from guardx_amd import Engine
    cfg = task_config(33, seed=2)
    O = oracle.OracleEngine(cfg, n_candidates=20000)
    rows = O.reset()
    rows[4, 0], rows[6, :] = np.nan, 0.0
    net = _net(43, 1, h, 9)
    np.testing.assert_array_equal(_vc_numpy(oracle, Engine.pack_critic(net).numpy(), rows),
                                  _oracle_rows(oracle, cfg, net, rows, h))


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
def _engines_rollout(cfg, hidden_pi, hidden_vc, T, impl=0, seed=5):
    """engine A: actor + cost critic; B: vc in the v slot (when the widths agree, else None); C: no cost critic --
    engines seeded identically"""
    import torch
    from guardx_amd import Engine
    runs = []
    for kind in ("A", "B", "C"):
        if kind == "B" and hidden_pi != hidden_vc:
            runs.append((None, None, None))
            continue
        E = Engine(cfg, n_candidates=40000)
        if impl:
            E.set_policy_impl(impl)
        E.reset()
        D, A = E.obs_flat_size, E.action_space.shape[0]
        mu_net, v_net, vc_net = _net(D, A, hidden_pi, seed), _net(D, 1, hidden_pi, seed + 1), _net(D, 1, hidden_vc, seed + 2)
        if kind == "B":
            p = Engine.pack_actor_critic(mu_net=mu_net, v_net=vc_net, log_std=_log_std(A))
            out = E.rollout_policy(p.cuda(), T, noise_seed=(11, 13))
        else:
            p = Engine.pack_actor_critic(mu_net=mu_net, v_net=v_net, log_std=_log_std(A))
            kw = dict(cost_critic=Engine.pack_critic(_VC(vc_net)).cuda()) if kind == "A" else {}
            out = E.rollout_policy(p.cuda(), T, noise_seed=(11, 13), **kw)
        torch.cuda.synchronize()
        runs.append((E, out, vc_net))
    return runs


@pytest.mark.gpu
@pytest.mark.parametrize("robot,hidden", [("point", 64), ("point", 128), ("point", 192), ("point", 256),
                                          ("swimmer", 64), ("swimmer", 256), ("ant", 64), ("ant", 256),
                                          ("walker", 64), ("walker", 256), ("config5", 128)])
def test_vc_bit_equal_to_value_head(oracle, robot, hidden):
    from guardx_amd import Engine, configuration
    N, T = 203, 50
    if robot == "config5":
        cfg = dict(configuration("Ant_8Hazards_8Pillars_synthetic"))
        cfg.update(env_num=N, _seed=3, num_steps=30, goal_size=2.4)
    else:
        cfg = task_config(N, seed=3, num_steps=30, goal_size=0.9, **ROBOTS[robot])
    (EA, a, vc_net), (EB, b, _), (EC, c, _) = _engines_rollout(cfg, hidden, hidden, T)
    if robot == "config5":
        assert EA.obs_flat_size == 80
    assert a['done'].sum().item() > 0
    assert a['vc'].shape == (T, N) and a['vc_last'].shape == (N,)
    np.testing.assert_array_equal(a['vc'].cpu().numpy(), b['val'].cpu().numpy())
    np.testing.assert_array_equal(a['vc_last'].cpu().numpy(), b['val_last'].cpu().numpy())
    assert set(a) == set(c) | {'vc', 'vc_last'}
    for k in c:                                    # the option changes nothing else
        np.testing.assert_array_equal(a[k].cpu().numpy(), c[k].cpu().numpy(), err_msg=k)
    assert_state_equal(EA.get_state(), EC.get_state())
    # and the checker: vc in the v slot of the oracle's rollout
    O = oracle.OracleEngine(cfg, n_candidates=40000)
    o0 = O.reset()
    D, A = EA.obs_flat_size, EA.action_space.shape[0]
    p = Engine.pack_actor_critic(mu_net=_net(D, A, hidden, 5), v_net=vc_net, log_std=_log_std(A)).numpy()
    o = O.rollout_policy(p, T, o0, noise_seed=(11, 13), hidden=hidden)
    np.testing.assert_array_equal(a['obs'].cpu().numpy(), o['obs'])
    np.testing.assert_array_equal(a['vc'].cpu().numpy(), o['val'])
    np.testing.assert_array_equal(a['vc_last'].cpu().numpy(), o['val_last'])
    for E in (EA, EB, EC):
        E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["point", "ant"])
def test_vc_same_under_every_policy_form(robot):
    N, T = 203, 40
    cfg = task_config(N, seed=4, num_steps=25, goal_size=0.9, **ROBOTS[robot])
    ref = None
    for impl in (1, 2, 3):
        (EA, a, _), (EB, b, _), (EC, c, _) = _engines_rollout(cfg, 64, 64, T, impl=impl)
        np.testing.assert_array_equal(a['vc'].cpu().numpy(), b['val'].cpu().numpy())
        np.testing.assert_array_equal(a['vc_last'].cpu().numpy(), b['val_last'].cpu().numpy())
        got = (a['vc'].cpu().numpy(), a['vc_last'].cpu().numpy())
        if ref is None:
            ref = got
        np.testing.assert_array_equal(got[0], ref[0])
        np.testing.assert_array_equal(got[1], ref[1])
        for E in (EA, EB, EC):
            E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("robot,h_pi,h_vc", [("point", 64, 256), ("point", 256, 64), ("ant", 64, 256)])
def test_vc_width_differs_from_actor(oracle, robot, h_pi, h_vc):
    N, T = 203, 30
    cfg = task_config(N, seed=6, num_steps=20, goal_size=0.9, **ROBOTS[robot])
    (EA, a, vc_net), _, (EC, c, _) = _engines_rollout(cfg, h_pi, h_vc, T)
    for k in c:
        np.testing.assert_array_equal(a[k].cpu().numpy(), c[k].cpu().numpy(), err_msg=k)
    obs = a['obs'].cpu().numpy()
    for t in range(T):
        np.testing.assert_array_equal(a['vc'][t].cpu().numpy(), _oracle_rows(oracle, cfg, vc_net, obs[t], h_vc))
    np.testing.assert_array_equal(a['vc_last'].cpu().numpy(),
                                  _oracle_rows(oracle, cfg, vc_net, a['obs_last'].cpu().numpy(), h_vc))
    for E in (EA, EC):
        E.close()


@pytest.mark.gpu
def test_cost_critic_size_error_launches_nothing():
    import torch
    from guardx_amd import Engine
    E = Engine(task_config(16, seed=1), n_candidates=20000)
    E.reset()
    D, A = E.obs_flat_size, 2
    p = Engine.pack_actor_critic(mu_net=_net(D, A, 64, 0), v_net=_net(D, 1, 64, 1), log_std=_log_std(A)).cuda()
    before = E.get_state()
    with pytest.raises(ValueError, match="cost_critic"):
        E.rollout_policy(p, 3, cost_critic=torch.zeros(1234, device='cuda'))
    with pytest.raises(ValueError, match="cost_critic"):   # a critic for another observation width
        E.rollout_policy(p, 3, cost_critic=Engine.pack_critic(_net(D + 1, 1, 64, 2)).cuda())
    assert_state_equal(E.get_state(), before)
    E.close()


def _rows(rng, M, D):
    x = rng.normal(0, 1.5, (M, D)).astype(np.float32)
    if M >= 17:
        x[3, 0] = np.nan
        x[5, D - 1] = np.inf
        x[7, :] = -np.inf
        x[9, D // 2] = 3e38
        x[11, :] = 0.0
        x[13, 0] = 1e-40                 # a subnormal input
    return x


@pytest.mark.gpu
@pytest.mark.parametrize("D", [1, 3, 43, 61, 80])
@pytest.mark.parametrize("h", [64, 128, 192, 256])
def test_critic_values_standalone(oracle, D, h):
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    net = _net(D, 1, h, 21 + D)
    params = Engine.pack_critic(net)
    pd = params.cuda()
    rng = np.random.default_rng(D * 1000 + h)
    for M in (0, 1, 17, 4099):
        x = _rows(rng, M, D)
        got = critic_values(pd, torch.from_numpy(x).cuda())
        assert got.shape == (M,) and got.dtype == torch.float32
        if M == 0:
            continue
        got = got.cpu().numpy()
        if M <= 17 or h == 64:
            np.testing.assert_array_equal(got, _vc_numpy(oracle, params.numpy(), x), err_msg=f"M={M}")
        finite = np.isfinite(x).all(1) & (np.abs(x).max(1) < 1e30)
        with torch.no_grad():
            tv = net(torch.from_numpy(x)).squeeze(-1).numpy()
        np.testing.assert_allclose(got[finite], tv[finite], rtol=2e-5, atol=2e-5)
        assert np.isnan(got[3]) if M >= 17 else True
    # (..., D) shapes and out=
    x = torch.from_numpy(_rows(rng, 4 * 5 * 7, D).reshape(4, 5, 7, D)).cuda()
    out = torch.empty(4, 5, 7, device='cuda')
    r = critic_values(pd, x, out=out)
    assert r is out
    np.testing.assert_array_equal(out.cpu().numpy().reshape(-1), critic_values(pd, x.reshape(-1, D)).cpu().numpy())
    # the checker's own route where a task has this width
    if D == 43:
        cfg = task_config(17, seed=2)
        x = _rows(rng, 17, D)
        np.testing.assert_array_equal(critic_values(pd, torch.from_numpy(x).cuda()).cpu().numpy(),
                                      _oracle_rows(oracle, cfg, net, x, h))


@pytest.mark.gpu
@pytest.mark.parametrize("h", [64, 256])
def test_critic_values_full_rollout_size(h):
    """M = 402 000 rows (T = 200 at env_num = 2000, plus the last observations): rows gathered from a rollout's
    observations, whose values the value-head route fixed bit for bit"""
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    N, T = 203, 50
    cfg = task_config(N, seed=3, num_steps=30, goal_size=0.9)
    (EA, a, vc_net), (EB, b, _), (EC, _, _) = _engines_rollout(cfg, h, h, T)
    rows = torch.cat([b['obs'].reshape(T * N, -1), b['obs_last']])
    vals = torch.cat([b['val'].reshape(T * N), b['val_last']])
    idx = torch.from_numpy(np.random.default_rng(h).integers(0, rows.shape[0], 402000)).cuda()
    got = critic_values(Engine.pack_critic(vc_net).cuda(), rows[idx].contiguous())
    assert torch.equal(got, vals[idx])
    for E in (EA, EB, EC):
        E.close()


@pytest.mark.gpu
@pytest.mark.parametrize("robot", ["point", "ant"])
def test_cost_rollout_batch_equals_cpo_buffer(robot):
    import torch
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import DeviceCostRolloutBuffer, cost_rollout_batch
    N, T = 203, 50
    cfg = task_config(N, seed=8, num_steps=30, goal_size=0.9, hazards_size=0.6, **ROBOTS[robot])
    E = Engine(cfg, n_candidates=40000)
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    p = Engine.pack_actor_critic(mu_net=_net(D, A, 64, 1), v_net=_net(D, 1, 64, 2), log_std=_log_std(A))
    out = E.rollout_policy(p.cuda(), T, noise_seed=(3, 4), cost_critic=Engine.pack_critic(_net(D, 1, 128, 3)).cuda())
    assert out['done'].sum().item() > 0 and out['cost'].abs().sum().item() > 0
    batch = cost_rollout_batch(out)
    buf = DeviceCostRolloutBuffer(N, T, (D,), (A,), device='cuda')       # CPO's loop, cpo.py:596-660
    logstd = out['logstd'].reshape(1, A).expand(N, A)
    for t in range(T):
        buf.store(out['obs'][t], out['act'][t], out['rew'][t], out['val'][t], out['logp'][t], out['cost'][t],
                  out['vc'][t], out['mu'][t], logstd)
        done = out['done'][t]
        if t + 1 == T:
            z = torch.zeros(N, device='cuda')
            buf.finish_path(z, z, torch.ones(N, device='cuda'))
        elif done.any():
            v, vc = out['val'][t].clone(), out['vc'][t].clone()
            v[done == 1] = 0
            vc[done == 1] = 0
            buf.finish_path(v, vc, done)
    ref = buf.get()
    assert set(batch) == set(ref) == {'obs', 'act', 'ret', 'adv', 'cost_ret', 'adc', 'logp', 'mu', 'logstd'}
    for k in ('obs', 'act', 'logp', 'mu', 'logstd', 'ret', 'cost_ret'):
        assert batch[k].shape == ref[k].shape, k
        np.testing.assert_allclose(batch[k].cpu().numpy(), ref[k].cpu().numpy(), rtol=1e-6, atol=1e-6, err_msg=k)
    for k in ('adv', 'adc'):
        np.testing.assert_allclose(batch[k].cpu().numpy(), ref[k].cpu().numpy(), rtol=2e-5, atol=2e-5, err_msg=k)
    E.close()
