"""Engine.rollout_episode (the `*_one_episode` learners' collection loop on the device, guardx_amd/episode.py,
libguardx_episode.so) and rollout_buffer.episode_rollout_batch: the rows before an env's first done against
rollout_policy bit for bit, the env side of ALL rows against step() without reset_done, the networks of all rows against
the batched critic pass (bits) and oracle/policy64.py (its bounds), the first-done bookkeeping against a sequential
float32 restatement, the sanitising of non-finite observations, the tail's rule through gxe_tail_probe, the batch helper
against torch and its own host-tensor path, and that nothing is ever re-initialised.

First-done steps that differ: a random plausible state (helpers.random_state, no env done, steps = 0) is planted after
reset().  Goals planted next to a robot finish it at step 1, num_steps = 12 finishes the others inside a 16-step call,
num_steps = 1000 leaves most of them unfinished after 8 steps.  Every test that relies on such coverage asserts it."""
import numpy as np
import pytest

from oracle import policy64
from helpers import random_state
from test_policy64 import make_ac, critic_net, report_line
from test_gpu_statewise import _cfg, _engine, _np, SEED

pytestmark = pytest.mark.gpu

STATE_SEED = 1


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _planted(robot, N, num_steps, seed=STATE_SEED, **ekw):
    """an engine after reset() with a random state planted (no env done, every episode at its start), and that state"""
    E = _engine(_cfg(robot, N, num_steps=num_steps), **ekw)
    E.reset()
    s = random_state(N, 8, np.random.default_rng(seed), done_frac=0, robot=robot)
    s['steps'][:] = 0
    E.set_state(s)
    return E, s


def _nets(E, h, h_vc, seed):
    from guardx_amd import Engine
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac = make_ac(D, A, h, seed=seed, shift=h // 64)
    vcn = critic_net(D, h_vc, seed=seed + 7).v_net if h_vc else None
    return ac, vcn, Engine.pack_actor_critic(ac).cuda(), (Engine.pack_critic(vcn, device='cuda') if h_vc else None)


def _lengths(first_done, T):
    return np.where(first_done > 0, np.minimum(first_done, T), T)


def _coverage(g, T):
    """which of the classes the planted state is meant to produce a call shows"""
    fd, done = g['first_done'], g['done']
    after = np.array([fd[e] > 0 and (done[fd[e]:, e] == 0).any() for e in range(len(fd))])
    return dict(first=(fd == 1).any(), inside=((fd > 1) & (fd < T)).any(), never=(fd == 0).any(), undone=after.any())


# (robot, actor width, cost critic width or 0, N, num_steps, T)
TWIN_CASES = [("point", 64, 0, 1, 12, 16), ("point", 64, 64, 16, 12, 16), ("point", 64, 0, 17, 12, 16),
              ("point", 64, 64, 48, 12, 16), ("point", 64, 0, 48, 1000, 8), ("ant", 256, 128, 17, 12, 16)]


@pytest.mark.parametrize("robot,h,h_vc,N,num_steps,T", TWIN_CASES)
def test_rows_before_the_first_done_are_rollout_policys(robot, h, h_vc, N, num_steps, T):
    """two engines, same config, seed, planted state, params and noise seed: for every env the rows at t < L are
    rollout_policy's (step-wise form) bit for bit; the engine is left as after a step()"""
    E, _ = _planted(robot, N, num_steps)
    Et, _ = _planted(robot, N, num_steps)
    Et.set_policy_impl(3)
    ac, vcn, p, vcp = _nets(E, h, h_vc, seed=h + N)
    out = E.rollout_episode(p, T, noise_seed=SEED, cost_critic=vcp)
    assert E._rd_obs is None and E._obs is out['obs_last'] and out['t0'] == 0
    g = _np({k: v for k, v in out.items() if k != 't0'})
    w = _np(Et.rollout_policy(p, T, noise_seed=SEED, cost_critic=vcp))
    L = _lengths(g['first_done'], T)
    keys = ('obs', 'act', 'mu', 'logp', 'val', 'rew', 'cost', 'done') + (('vc',) if h_vc else ())
    assert ('vc' in g) == bool(h_vc) == ('vc_last' in g)
    for e in range(N):
        for k in keys:
            np.testing.assert_array_equal(bits(g[k][:L[e], e]), bits(w[k][:L[e], e]), err_msg=f"env {e} {k}")
    np.testing.assert_array_equal(bits(g['logstd']), bits(w['logstd']))
    never = g['first_done'] == 0                                # never finished: the bootstrap is rollout_policy's too
    for k in ('obs_last', 'val_last') + (('vc_last',) if h_vc else ()):
        np.testing.assert_array_equal(bits(g[k][never]), bits(w[k][never]), err_msg=k)
    cov = _coverage(g, T)
    print(f"{robot} N={N} num_steps={num_steps}: first_done values {sorted(set(g['first_done'].tolist()))} coverage {cov}")
    if N >= 16:
        assert (g['first_done'] > 0).any()                       # the comparison stops somewhere: L < T for some env
    if N == 48 and num_steps == 12:
        assert cov['first'] and cov['inside'] and cov['undone']
        assert (w['done'][:-1].sum(0) > 0).any()                # and rollout_policy did reset rows that are compared no further
    if N == 48 and num_steps == 1000:
        assert cov['never'] and cov['first']
    E.close()
    Et.close()


def _shared_run(num_steps, T, need):
    """Point (64, 64) with a cost critic, N = 48: one call on a planted engine, with the coverage classes `need` asserted"""
    E, s = _planted("point", 48, num_steps)
    stats0 = E.prefetch_stats()
    ac, vcn, p, vcp = _nets(E, 64, 64, seed=5)
    out = E.rollout_episode(p, T, noise_seed=SEED, cost_critic=vcp)
    g = _np({k: v for k, v in out.items() if k != 't0'})
    cov = _coverage(g, T)
    assert all(cov[k] for k in need), cov
    return dict(E=E, s=s, ac=ac, vcn=vcn, p=p, vcp=vcp, out=out, g=g, stats0=stats0, T=T, N=48)


@pytest.fixture(scope="module")
def main_run():
    """num_steps = 12, T = 16: every env finishes inside the call, at step 1, later, and with done back at 0 afterwards;
    shared, read only"""
    run = _shared_run(12, 16, ('first', 'inside', 'undone'))
    yield run
    run['E'].close()


@pytest.fixture(scope="module")
def open_run():
    """num_steps = 1000, T = 8: most envs never finish (first_done == 0: the bootstrap, L == T), some finish at step 1;
    shared, read only"""
    run = _shared_run(1000, 8, ('never', 'first'))
    yield run
    run['E'].close()


def test_the_env_side_of_all_rows_is_step_without_reset_done(main_run):
    """a second engine driven from Python by step(act[t]) and no reset_done(): obs[t + 1], obs_last, rew, cost and done
    of every row, past the first done included"""
    import torch
    g, T = main_run['g'], main_run['T']
    E2, _ = _planted("point", main_run['N'], 12)
    for t in range(T):
        obs, rew, done, info = E2.step(main_run['out']['act'][t])
        nxt = g['obs'][t + 1] if t + 1 < T else g['obs_last']
        np.testing.assert_array_equal(bits(obs.cpu().numpy()), bits(nxt), err_msg=f"obs after step {t}")
        for k, v in (('rew', rew), ('done', done), ('cost', info['cost'])):
            np.testing.assert_array_equal(bits(v.cpu().numpy()), bits(g[k][t]), err_msg=f"{k}[{t}]")
    assert np.isfinite(g['obs']).all()
    torch.cuda.synchronize()
    E2.close()


def test_the_networks_on_all_rows(main_run):
    """val and vc are the batched critic pass's bits on the recorded rows (INTEGRATION.md promises that of the critic
    pass); mu, act, logp, val, val_last and vc / vc_last within policy64's bounds on every row, those at t >= L included"""
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    out, g, ac, vcn = main_run['out'], main_run['g'], main_run['ac'], main_run['vcn']
    v = critic_values(Engine.pack_critic(ac.v.v_net, device='cuda'), out['obs']).cpu().numpy()
    np.testing.assert_array_equal(bits(v), bits(g['val']))
    vc = critic_values(main_run['vcp'], out['obs']).cpu().numpy()
    np.testing.assert_array_equal(bits(vc), bits(g['vc']))
    vl = critic_values(main_run['vcp'], out['obs_last']).cpu().numpy()
    np.testing.assert_array_equal(bits(vl), bits(g['vc_last']))
    L = _lengths(g['first_done'], main_run['T'])
    assert (L < main_run['T']).sum() > 4                         # rows past a first done are among those checked
    want = policy64.rollout(policy64.ActorCritic(ac), g, SEED, t0=0, env_offset=0, cost_critic=vcn)
    report_line("episode point 64/64 all rows", policy64.compare(g, want, keys=policy64.OUTPUTS + ('vc', 'vc_last'),
                                                                 what="rollout_episode"))
    torch.cuda.synchronize()


def bookkeeping_np(rew, cost, done, state=None, t_base=0):
    """first_done, ep_ret, ep_cost, ep_len after the steps of (T, N) rew / cost / done, float32 adds in step order"""
    T, N = rew.shape
    f = np.float32
    fd, ret, cst, ln = state if state else (np.zeros(N, np.int32), np.zeros(N, f), np.zeros(N, f), np.zeros(N, np.int32))
    fd, ret, cst, ln = fd.copy(), ret.copy(), cst.copy(), ln.copy()
    for t in range(T):
        k = t_base + t + 1
        live = fd == 0
        ret = np.where(live, (ret + rew[t]).astype(f), ret)
        cst = np.where(live, (cst + cost[t]).astype(f), cst)
        ln = np.where(live, k, ln).astype(np.int32)
        fd = np.where(live & (done[t] > 0), k, fd).astype(np.int32)
    return fd, ret, cst, ln


def _assert_state(g, want, what):
    for k, w in zip(('first_done', 'ep_ret', 'ep_cost', 'ep_len'), want):
        assert g[k].dtype == w.dtype, k
        np.testing.assert_array_equal(g[k].view(np.uint32), w.view(np.uint32), err_msg=f"{what} {k}")


def test_bookkeeping_across_calls_reset_and_other_paths(main_run):
    """the state against the sequential restatement; two calls of T / 2 against one call of T (same engine config and
    planted state; the path's noise counter is 0 at construction and advances by T / 2 with the first call, so the second
    call draws what steps T / 2 .. T - 1 of the single call drew -- nothing has to be arranged); step() and
    rollout_policy leave the state alone, reset() clears it"""
    import torch
    g, T, N = main_run['g'], main_run['T'], main_run['N']
    _assert_state(g, bookkeeping_np(g['rew'], g['cost'], g['done']), "one call")
    assert (g['ep_len'] == _lengths(g['first_done'], T)).all()
    E, _ = _planted("point", N, 12)
    p, vcp = main_run['p'], main_run['vcp']
    a = E.rollout_episode(p, T // 2, noise_seed=SEED, cost_critic=vcp)
    ga = _np({k: v for k, v in a.items() if k != 't0'})
    _assert_state(ga, bookkeeping_np(ga['rew'], ga['cost'], ga['done']), "first half")
    b = E.rollout_episode(p, T // 2, noise_seed=SEED, cost_critic=vcp)
    gb = _np({k: v for k, v in b.items() if k != 't0'})
    assert (a['t0'], b['t0']) == (0, T // 2)
    for k in ('obs', 'act', 'mu', 'logp', 'val', 'vc', 'rew', 'cost', 'done'):
        np.testing.assert_array_equal(bits(np.concatenate([ga[k], gb[k]])), bits(g[k]), err_msg=k)
    for k in ('obs_last', 'val_last', 'vc_last', 'logstd'):
        np.testing.assert_array_equal(bits(gb[k]), bits(g[k]), err_msg=k)
    _assert_state(gb, tuple(g[k] for k in ('first_done', 'ep_ret', 'ep_cost', 'ep_len')), "two halves")
    # other paths neither read nor write the state
    st = E._episode
    before = (st.book.ints.clone(), st.book.sums.clone(), st.book.t_base, st.steps)
    E.step(torch.zeros(N, 2, device='cuda'))
    E.reset_done()
    E.rollout_policy(p, 3, noise_seed=SEED)
    assert torch.equal(st.book.ints, before[0]) and torch.equal(st.book.sums, before[1]) and (st.book.t_base, st.steps) == before[2:]
    assert (before[0][0] > 0).any()
    E.reset()
    assert int(st.book.ints.abs().sum()) == 0 and float(st.book.sums.abs().sum()) == 0 and st.book.t_base == 0
    assert st.steps == T                                         # the noise counter is not reset
    c = E.rollout_episode(p, 2, noise_seed=SEED)
    assert c['t0'] == 0 and 'vc' not in c
    E.close()


def test_bookkeeping_with_envs_that_never_finish(open_run):
    """the state restatement where first_done stays 0: the sums run over all T steps and ep_len == T"""
    g, T = open_run['g'], open_run['T']
    never = g['first_done'] == 0
    assert never.any() and (~never).any()
    _assert_state(g, bookkeeping_np(g['rew'], g['cost'], g['done']), "open run")
    assert (g['ep_len'][never] == T).all() and (g['ep_len'] == _lengths(g['first_done'], T)).all()


def test_non_finite_observations_are_zeroed_for_the_networks():
    """obs0 with NaN, +Inf and -Inf planted: obs[0] holds +0.0 there and the other entries untouched, and every output of
    the call equals that of a call with zeros planted instead, bit for bit"""
    import torch
    N, T = 17, 2
    runs = []
    for fill in (None, 0.0):
        E, _ = _planted("point", N, 12)
        ac, vcn, p, vcp = _nets(E, 64, 64, seed=3)
        obs0 = E._obs.clone()
        clean = obs0.clone()
        for (e, k), v in {(0, 0): np.nan, (0, 5): np.inf, (3, 2): -np.inf, (16, obs0.shape[1] - 1): np.nan, (16, 1): np.inf}.items():
            obs0[e, k] = v if fill is None else fill
        runs.append(_np({k: v for k, v in E.rollout_episode(p, T, obs0=obs0, noise_seed=SEED, cost_critic=vcp).items() if k != 't0'}))
        E.close()
    g, z = runs
    bad = [(0, 0), (0, 5), (3, 2), (16, g['obs'].shape[2] - 1), (16, 1)]
    mask = np.zeros(g['obs'][0].shape, bool)
    for e, k in bad:
        mask[e, k] = True
        assert bits(g['obs'][0])[e, k] == 0                      # +0.0, not -0.0
    np.testing.assert_array_equal(bits(g['obs'][0][~mask]), bits(clean.cpu().numpy()[~mask]))
    for k in g:
        np.testing.assert_array_equal(g[k].view(np.uint32), z[k].view(np.uint32), err_msg=k)
    assert np.isfinite(g['val']).all() and np.isfinite(g['act']).all()


@pytest.mark.parametrize("h,h_vc,D,A,n", [(64, 64, 43, 2, 37), (256, 128, 70, 8, 16), (64, 0, 43, 2, 1)])
def test_the_tail_rule_through_the_probe(h, h_vc, D, A, n):
    """rows with a non-finite entry get val_last = vc_last = 0 and obs_last raw; finite rows are the critic pass's bits"""
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    from guardx_amd.episode import tail_probe
    ac = make_ac(D, A, h, seed=n)
    vcn = critic_net(D, h_vc, seed=n + 1).v_net if h_vc else None
    p = Engine.pack_actor_critic(ac).cuda()
    vcp = Engine.pack_critic(vcn, device='cuda') if h_vc else None
    rng = np.random.default_rng(n)
    rows = rng.normal(size=(n, D)).astype(np.float32)
    bad = {0: np.nan, 5: np.inf, 16: -np.inf, 36: np.nan} if n > 16 else ({3: np.inf, 15: np.nan} if n > 1 else {})
    for e, v in bad.items():
        rows[e, (7 * e) % D] = v
    if n > 16:
        rows[5, D - 1] = np.nan                                   # two entries of one row
    x = torch.from_numpy(rows).cuda()
    got = _np(tail_probe(p, x, A, cost_critic=vcp))
    assert ('vc_last' in got) == bool(h_vc)
    np.testing.assert_array_equal(bits(got['obs_last']), bits(rows))                    # raw, NaN payloads included
    finite = np.isfinite(rows).all(1)
    assert (~finite).sum() == len(bad)
    clean = torch.from_numpy(np.where(np.isfinite(rows), rows, 0).astype(np.float32)).cuda()
    v = critic_values(Engine.pack_critic(ac.v.v_net, device='cuda'), clean).cpu().numpy()
    np.testing.assert_array_equal(bits(got['val_last'][finite]), bits(v[finite]))
    assert (bits(got['val_last'][~finite]) == 0).all()
    if h_vc:
        vc = critic_values(vcp, clean).cpu().numpy()
        np.testing.assert_array_equal(bits(got['vc_last'][finite]), bits(vc[finite]))
        assert (bits(got['vc_last'][~finite]) == 0).all()


@pytest.mark.parametrize("with_cost", [True, False])
@pytest.mark.parametrize("which", ["main_run", "open_run"])
def test_episode_rollout_batch_on_the_device(request, which, with_cost):
    """n_valid, the gathered rows against torch's transpose + boolean gather, and ret / adv / cost_ret / adc against the
    helper's own host-tensor path on the result moved to the CPU: BIT-equal, because the kernel keeps that recursion's
    operation order (include/guardx_episode.h; the library is built with -ffp-contract=off).  On the run whose envs all
    finish (every path closed with 0) and on the run where most never do (first_done == 0: L == T and the bootstrap with
    val_last / vc_last, which is also checked on the last row of every env directly).  Rows beyond n_valid are left
    unwritten (the outputs are torch.empty): the caller gets views of the first n_valid rows only."""
    import torch
    from guardx_amd.rollout_buffer import episode_rollout_batch, _env_major
    run = request.getfixturevalue(which)
    out = dict(run['out'])
    if not with_cost:
        for k in ('vc', 'vc_last'):
            out.pop(k)
    g, T, N = run['g'], run['T'], run['N']
    never = g['first_done'] == 0
    assert (~never).any() and never.any() == (which == "open_run")
    L = _lengths(g['first_done'], T)
    got = episode_rollout_batch(out)
    assert got['n_valid'] == int(L.sum()) < N * T
    valid = torch.from_numpy((np.arange(T)[None, :] < L[:, None]).reshape(N * T)).cuda()
    for k in ('obs', 'act', 'mu', 'logp'):
        want = _env_major(out[k]).view(N * T, *out[k].shape[2:])[valid]
        assert torch.equal(got[k], want), k
        assert got[k]._base is not None and got[k]._base.shape[0] == N * T       # a view of the first rows of N T
    host = episode_rollout_batch({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()})
    assert host['n_valid'] == got['n_valid']
    keys = ('ret', 'adv') + (('cost_ret', 'adc') if with_cost else ())
    assert ('adc' in got) == with_cost
    for k in keys:
        np.testing.assert_array_equal(bits(got[k].cpu().numpy()), bits(host[k].numpy()), err_msg=k)
    # the last row of every env: rew + gamma b with b = val_last where the env never finished and 0 where it did (one
    # fp32 product and sum in float64, rounded once: a few ulp of the fp32 result at most)
    last = np.cumsum(L) - 1
    for ch, rk, bk in (('ret', 'rew', 'val_last'),) + ((('cost_ret', 'cost', 'vc_last'),) if with_cost else ()):
        boot = np.where(never, g[bk], np.float32(0)).astype(np.float64)
        want = g[rk][L - 1, np.arange(N)].astype(np.float64) + float(np.float32(0.99)) * boot
        np.testing.assert_allclose(got[ch].cpu().numpy()[last], want, rtol=1e-6, atol=1e-6, err_msg=ch)
        if never.any():
            assert (np.abs(boot[never]) > 1e-3).any()             # the bootstrap is not a zero that would hide its absence
    assert torch.equal(got['logstd'], out['logstd'].reshape(1, -1).expand(got['n_valid'], -1))
    with pytest.raises(ValueError, match="t0"):
        episode_rollout_batch(dict(out, t0=4))
    with pytest.raises(ValueError, match="shape"):
        episode_rollout_batch(dict(out, first_done=out['first_done'][:-1]))
    with pytest.raises(ValueError, match="shape"):
        episode_rollout_batch(dict(out, val=out['val'][:-1]))


def test_nothing_is_reset(main_run):
    """after rollout_episode no env was re-initialised (the planted layout rows are all there: a reset_done would have
    drawn new ones for the envs that finished) and the layout-pool prefetch saw nothing"""
    import torch
    E, s, g = main_run['E'], main_run['s'], main_run['g']
    torch.cuda.synchronize()
    after = E.get_state()
    assert (g['first_done'] > 0).any()
    np.testing.assert_array_equal(after['objs'], s['objs'])
    assert E.prefetch_stats() == main_run['stats0']
