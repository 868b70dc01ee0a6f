"""The one-episode form of the three safe-action rollouts, Engine.rollout_safelayer / rollout_usl / rollout_lpg(...,
episode=True) (guardx_<library>_policy_step_episode and a plain env.step per control step, guardx_amd/_closed_loop.py:run_episode),
and rollout_buffer.episode_rollout_batch on their results.  Everything is compared bit for bit: the warm-up branch against
rollout_episode, the rows before an env's first done against the same path's reset_done form on a twin engine, the env
side of ALL rows against step() without reset_done, the correction of all rows against the library's own probe, the
sanitising against a call on pre-zeroed rows, the tail's rule through the three tail probes, the bookkeeping across
calls, and the batch helper against its host-tensor path and a numpy restatement of the learners' buffers.

Engines, planted states and coverage classes are tests/test_gpu_episode.py's; the networks are those of the safelayer,
USL and LPG suites.  That the corrections below act on at least a tenth of the compared rows was sized on the CPU
checker's engine with the float64 restatements (tests/test_episode_safe_host.py::test_the_chosen_inputs_are_corrected)."""
import numpy as np
import pytest

from test_gpu_statewise import _np, SEED
from test_gpu_episode import _planted, _coverage, _lengths, bits, bookkeeping_np, _assert_state
from test_gpu_safelayer import corr_nets
from test_gpu_usl import rollout_nets
import test_gpu_usl
import test_gpu_lpg

pytestmark = pytest.mark.gpu

LEARNERS = ("safelayer", "usl", "lpg")
NUM_STEPS, T = 12, 16
# (robot, actor width, third network's width, N)
SHAPES = [("point", 64, 64, 1), ("point", 64, 64, 16), ("point", 64, 64, 17), ("point", 64, 64, 48), ("ant", 256, 128, 17)]
SHARE = 0.1          # of the compared rows, at least: the correction did something
USL_DELTA = {"point": 0.6, "ant": 0.3}       # tests/test_gpu_usl.py:ROLLOUT_CASES
STATE = ('first_done', 'ep_ret', 'ep_cost', 'ep_len')     # the order of test_gpu_episode._assert_state


def nets(learner, D, A, h, h3):
    """the actor-critic and the learner's third module: the correction tests' of the learner's own suite"""
    return corr_nets(D, A, h, h3) if learner == "safelayer" else rollout_nets(D, A, h, h3)


def correct_kw(learner, robot):
    """the keywords of a correct=True call: safelayer delta = 0 (pred = g . a + prev_c > 0 on about half of the rows);
    USL its own suite's delta; LPG delta = 0, grad_scale = 1 and store_init=False on a fresh engine (q_init = 0), so that
    eps = 0, every row is projected and lam > 0 wherever G . act > 0"""
    if learner == "safelayer":
        return dict(delta=0.0)
    if learner == "usl":
        return dict(delta=USL_DELTA[robot])
    return dict(delta=0.0, grad_scale=1.0, store_init=False)


def _pack(E, learner, h, h3):
    from guardx_amd import Engine
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, third = nets(learner, D, A, h, h3)
    p = Engine.pack_actor_critic(ac).cuda()
    tp = Engine.pack_g_net(third, device='cuda', act_dim=A) if learner == "safelayer" else Engine.pack_q_critic(third, device='cuda')
    return ac, p, tp


def _call(E, learner, p, tp, steps, **kw):
    fn = getattr(E, "rollout_" + learner)
    return fn(p, steps, noise_seed=SEED, **{"g_net" if learner == "safelayer" else "q_critic": tp}, **kw)


def _npo(out):
    return _np({k: v for k, v in out.items() if k != 't0'})


def _did_something(learner, g):
    """(T, N) bool: the rows on which the correction acted"""
    return (g['lam'] > 0) if learner == "lpg" else (g['act_safe'] != g['act']).any(-1)


# ---------------------------------------------------------------------------------------------------------------------
# 1. correct=False is rollout_episode
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,h,h3,N", SHAPES)
@pytest.mark.parametrize("learner", LEARNERS)
def test_warmup_is_rollout_episode(learner, robot, h, h3, N):
    """two planted engines: every key rollout_episode (no cost critic) returns has the same bits in the episode=True
    output of the warm-up branch, all T rows, the tail and the bookkeeping; act_safe is act"""
    E, _ = _planted(robot, N, NUM_STEPS)
    Ee, _ = _planted(robot, N, NUM_STEPS)
    ac, p, tp = _pack(E, learner, h, h3)
    out = _call(E, learner, p, tp, T, episode=True, correct=False, **({"store_init": False} if learner == "lpg" else {}))
    w = Ee.rollout_episode(p, T, noise_seed=SEED)
    assert E._rd_obs is None and E._obs is out['obs_last'] and out['t0'] == w['t0'] == 0
    g, w = _npo(out), _npo(w)
    for k in w:
        assert g[k].dtype == w[k].dtype, k
        np.testing.assert_array_equal(g[k].view(np.uint32), w[k].view(np.uint32), err_msg=f"{learner} {robot} N={N} {k}")
    np.testing.assert_array_equal(bits(g['act_safe']), bits(g['act']))
    if N == 48:
        cov = _coverage(g, T)
        assert cov['first'] and cov['inside'] and cov['undone'], cov
    E.close()
    Ee.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the rows before the first done are the reset form's
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot,h,h3,N", SHAPES)
@pytest.mark.parametrize("learner", LEARNERS)
def test_rows_before_the_first_done_are_the_reset_forms(learner, robot, h, h3, N):
    """correct=True on twin engines: per env every shared key at t < L equals the episode=False form, the corrected
    action and the path's own tensors included; and the correction acted on at least a tenth of those rows"""
    E, _ = _planted(robot, N, NUM_STEPS)
    Et, _ = _planted(robot, N, NUM_STEPS)
    ac, p, tp = _pack(E, learner, h, h3)
    kw = correct_kw(learner, robot)
    g = _npo(_call(E, learner, p, tp, T, episode=True, **kw))
    w = _np(_call(Et, learner, p, tp, T, **kw))
    own = ('g', 'prev_cost') if learner == "safelayer" else ('qc', 'iters' if learner == "usl" else 'lam')
    keys = ('obs', 'act', 'act_safe', 'mu', 'logp', 'val', 'rew', 'cost', 'done') + own
    assert set(w) - set(keys) <= {'obs_last', 'val_last', 'logstd', 'q_init'} and set(w) <= set(g)
    L = _lengths(g['first_done'], T)
    did = _did_something(learner, g)
    rows = acted = 0
    for e in range(N):
        for k in keys:
            np.testing.assert_array_equal(bits(g[k][:L[e], e]), bits(w[k][:L[e], e]), err_msg=f"{learner} env {e} {k}")
        rows += int(L[e])
        acted += int(did[:L[e], e].sum())
    np.testing.assert_array_equal(bits(g['logstd']), bits(w['logstd']))
    print(f"{learner} {robot} N={N}: {acted} of {rows} compared rows corrected, first_done {sorted(set(g['first_done'].tolist()))}")
    assert acted >= SHARE * rows
    if N >= 16:
        assert (L < T).any()                                      # the comparison stops somewhere
    E.close()
    Et.close()


# ---------------------------------------------------------------------------------------------------------------------
# shared runs: Point (64, 64), N = 48, correct=True, one call of T
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def runs():
    """learner -> its shared run, made on first use, read only"""
    made = {}

    def get(learner):
        if learner not in made:
            E, s = _planted("point", 48, NUM_STEPS)
            stats0 = E.prefetch_stats()
            ac, p, tp = _pack(E, learner, 64, 64)
            out = _call(E, learner, p, tp, T, episode=True, **correct_kw(learner, "point"))
            g = _npo(out)
            cov = _coverage(g, T)
            assert cov['first'] and cov['inside'] and cov['undone'], cov
            made[learner] = dict(E=E, s=s, ac=ac, p=p, tp=tp, out=out, g=g, stats0=stats0, N=48)
        return made[learner]
    yield get
    for r in made.values():
        r['E'].close()


# ---------------------------------------------------------------------------------------------------------------------
# 3. the env side of all rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_the_env_side_of_all_rows_is_step_without_reset_done(runs, learner):
    """a second engine driven by step(act_safe[t]) and no reset_done(): obs[t + 1], obs_last, rew, cost, done of every
    row, past the first done included; safelayer's prev_cost[t + 1] is cost[t] on every row, done or not"""
    import torch
    run = runs(learner)
    g = run['g']
    E2, _ = _planted("point", run['N'], NUM_STEPS)
    for t in range(T):
        obs, rew, done, info = E2.step(run['out']['act_safe'][t])
        nxt = g['obs'][t + 1] if t + 1 < T else g['obs_last']
        np.testing.assert_array_equal(bits(obs.cpu().numpy()), bits(nxt), err_msg=f"obs after step {t}")
        for k, v in (('rew', rew), ('done', done), ('cost', info['cost'])):
            np.testing.assert_array_equal(bits(v.cpu().numpy()), bits(g[k][t]), err_msg=f"{k}[{t}]")
    assert (_lengths(g['first_done'], T) < T).sum() > 4          # rows past a first done are among those compared
    if learner == "safelayer":
        np.testing.assert_array_equal(bits(g['prev_cost'][1:]), bits(g['cost'][:-1]))
        assert (bits(g['prev_cost'][0]) == 0).all()
        after_done = g['done'][:-1] > 0
        assert after_done.any() and (g['cost'][:-1][after_done] > 0).any()   # a done step whose cost is carried, not zeroed
        np.testing.assert_array_equal(bits(run['E']._safelayer.prev_c.cpu().numpy()), bits(g['cost'][-1]))   # the tail's update
    torch.cuda.synchronize()
    E2.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the correction on all rows
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_the_correction_on_all_rows_is_the_probes(runs, learner):
    """all T N rows, those past a first done included: act_safe (and qc, iters / lam) from the library's own probe on the
    recorded obs[t], act[t] (g and prev_cost for the safety layer, q_init = 0 for LPG)"""
    import torch
    from guardx_amd.safelayer import correction_probe
    run = runs(learner)
    g, out, N = run['g'], run['out'], run['N']
    kw = correct_kw(learner, "point")
    if learner == "safelayer":
        A = g['act'].shape[-1]
        a = correction_probe(out['g'].reshape(-1, A), out['act'].reshape(-1, A), out['prev_cost'].reshape(-1), kw['delta'])
        np.testing.assert_array_equal(bits(a.cpu().numpy()), bits(g['act_safe'].reshape(-1, A)))
    for t in range(T if learner != "safelayer" else 0):
        if learner == "usl":
            r = test_gpu_usl._probe(run['tp'], g['obs'][t], g['act'][t], delta=kw['delta'], niter=20, eta=0.05, grad_scale=1.0 / N)
            np.testing.assert_array_equal(bits(g['qc'][t]), bits(r['q0']), err_msg=f"t={t}")
            np.testing.assert_array_equal(g['iters'][t], r['iters'].astype(np.float32), err_msg=f"t={t}")
        else:
            r = test_gpu_lpg._probe(run['tp'], g['obs'][t], g['act'][t], np.zeros(N, np.float32), delta=0.0, grad_scale=1.0)
            np.testing.assert_array_equal(bits(g['qc'][t]), bits(r['q']), err_msg=f"t={t}")
            np.testing.assert_array_equal(bits(g['lam'][t]), bits(r['lam']), err_msg=f"t={t}")
        np.testing.assert_array_equal(bits(g['act_safe'][t]), bits(r['a_safe']), err_msg=f"t={t}")
    assert _did_something(learner, g).mean() >= SHARE
    if learner == "lpg":
        assert (bits(g['q_init']) == 0).all()                    # store_init=False on a fresh engine
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# 5. sanitising
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_non_finite_observations_are_zeroed_for_every_network(learner):
    """obs0 with NaN, +Inf, -Inf planted and one row non-finite throughout, T = 1: obs[0] is the zeroed row and every
    output equals that of a call on the pre-zeroed obs0"""
    N = 17
    runs_ = []
    for fill in (None, 0.0):
        E, _ = _planted("point", N, NUM_STEPS)
        ac, p, tp = _pack(E, learner, 64, 64)
        obs0 = E._obs.clone()
        clean = obs0.clone()
        D = obs0.shape[1]
        plant = {(0, 0): np.nan, (0, 5): np.inf, (3, 2): -np.inf, (16, D - 1): np.nan, (16, 1): np.inf}
        plant.update({(9, k): (np.nan, np.inf, -np.inf)[k % 3] for k in range(D)})       # a row that is all non-finite
        for (e, k), v in plant.items():
            obs0[e, k] = v if fill is None else fill
        runs_.append(_npo(_call(E, learner, p, tp, 1, obs0=obs0, episode=True, **correct_kw(learner, "point"))))
        E.close()
    g, z = runs_
    mask = np.zeros(g['obs'][0].shape, bool)
    for e, k in plant:
        mask[e, k] = True
    assert (bits(g['obs'][0])[mask] == 0).all()                    # +0.0, not -0.0
    np.testing.assert_array_equal(bits(g['obs'][0][~mask]), bits(clean.cpu().numpy()[~mask]))
    own = ('g',) if learner == "safelayer" else ('qc',)
    for k in ('obs', 'mu', 'val', 'act', 'act_safe', 'logp') + own:
        np.testing.assert_array_equal(bits(g[k]), bits(z[k]), err_msg=k)
        assert np.isfinite(g[k]).all(), k
    for k in g:                                                    # and everything else the call returns
        np.testing.assert_array_equal(g[k].view(np.uint32), z[k].view(np.uint32), err_msg=k)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the tail's rule
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 16, 37])
@pytest.mark.parametrize("learner", LEARNERS)
def test_the_tail_rule_through_the_probe(learner, n):
    """a row with one NaN, one with one Inf, the others clean: obs_last comes back raw, val_last is 0 on the bad rows and
    the batched critic pass's bits on the clean ones"""
    import importlib
    import torch
    from guardx_amd import Engine
    from guardx_amd.critic import critic_values
    D, A, h, h3 = (43, 2, 64, 64) if n != 16 else (70, 8, 256, 128)
    ac, third = nets(learner, D, A, h, h3)
    p = Engine.pack_actor_critic(ac).cuda()
    tp = Engine.pack_g_net(third, device='cuda') if learner == "safelayer" else Engine.pack_q_critic(third, device='cuda')
    rows = np.random.default_rng(n).normal(size=(n, D)).astype(np.float32)
    bad = {0: np.nan} if n == 1 else {3: np.nan, n - 1: np.inf}
    for e, v in bad.items():
        rows[e, (7 * e) % D] = v
    got = _np(importlib.import_module("guardx_amd." + learner).tail_probe(p, torch.from_numpy(rows).cuda(), A, tp))
    np.testing.assert_array_equal(bits(got['obs_last']), bits(rows))                    # raw, NaN payloads included
    finite = np.isfinite(rows).all(1)
    assert (~finite).sum() == len(bad) and (n == 1 or finite.any())
    clean = torch.from_numpy(np.where(np.isfinite(rows), rows, 0).astype(np.float32)).cuda()
    v = critic_values(Engine.pack_critic(ac.v.v_net, device='cuda'), clean).cpu().numpy()
    np.testing.assert_array_equal(bits(got['val_last'][finite]), bits(v[finite]))
    assert (bits(got['val_last'][~finite]) == 0).all()
    if n == 1:                                                     # the lone clean row
        rows[0] = np.where(np.isfinite(rows[0]), rows[0], 1.0)
        got = _np(importlib.import_module("guardx_amd." + learner).tail_probe(p, torch.from_numpy(rows).cuda(), A, tp))
        v = critic_values(Engine.pack_critic(ac.v.v_net, device='cuda'), torch.from_numpy(rows).cuda()).cpu().numpy()
        np.testing.assert_array_equal(bits(got['val_last']), bits(v))


# ---------------------------------------------------------------------------------------------------------------------
# 7. the bookkeeping across calls
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_bookkeeping_across_calls_reset_and_other_paths(runs, learner):
    """the state against the sequential restatement; two calls of T / 2 equal one of T with t0 = 0 then T / 2; an
    episode=False call of the same path, step() and rollout_episode leave the bookkeeping alone; reset() clears it"""
    import torch
    run = runs(learner)
    g, N, p, tp = run['g'], run['N'], run['p'], run['tp']
    kw = correct_kw(learner, "point")
    _assert_state(g, bookkeeping_np(g['rew'], g['cost'], g['done']), "one call")
    assert (g['ep_len'] == _lengths(g['first_done'], T)).all()
    E, _ = _planted("point", N, NUM_STEPS)
    a = _call(E, learner, p, tp, T // 2, episode=True, **kw)
    b = _call(E, learner, p, tp, T // 2, episode=True, **kw)
    assert (a['t0'], b['t0']) == (0, T // 2)
    ga, gb = _npo(a), _npo(b)
    _assert_state(ga, bookkeeping_np(ga['rew'], ga['cost'], ga['done']), "first half")
    for k in g:
        if g[k].ndim >= 2 and g[k].shape[0] == T and k != 'obs_last':
            np.testing.assert_array_equal(bits(np.concatenate([ga[k], gb[k]])), bits(g[k]), err_msg=k)
    for k in ('obs_last', 'val_last', 'logstd'):
        np.testing.assert_array_equal(bits(gb[k]), bits(g[k]), err_msg=k)
    _assert_state(gb, tuple(g[k] for k in STATE), "two halves")
    st = getattr(E, "_" + learner)
    book = st.book
    before = (book.ints.clone(), book.sums.clone(), book.t_base)
    assert (before[0][0] > 0).any()
    _call(E, learner, p, tp, 3, **kw)                            # the reset_done form of the same path
    E.step(torch.zeros(N, 2, device='cuda'))
    E.reset_done()
    E.rollout_episode(p, 2, noise_seed=SEED)
    assert torch.equal(book.ints, before[0]) and torch.equal(book.sums, before[1]) and book.t_base == before[2]
    assert E._episode.book.t_base == 2 and st.steps == T + 3          # each path its own counters
    E.reset()
    assert int(book.ints.abs().sum()) == 0 and float(book.sums.abs().sum()) == 0 and book.t_base == 0
    assert st.steps == T + 3                                     # the noise counter is not reset
    c = _call(E, learner, p, tp, 2, episode=True, **kw)
    assert c['t0'] == 0
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. episode_rollout_batch on the device
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("open_", [False, True])
@pytest.mark.parametrize("learner", LEARNERS)
def test_episode_rollout_batch_on_the_device(runs, learner, open_):
    """the device path against the host-tensor path on the same `out` (bit for bit) and against the numpy restatement of
    the learner's buffer (tests/test_episode_safe_host.py): n_valid == sum(L), the extra columns gathered, targetc at
    t = L - 1 (the cost alone) and on envs with L == T.  open_: num_steps = 1000, T = 8, where most envs never finish"""
    import torch
    from guardx_amd.rollout_buffer import episode_rollout_batch
    import test_episode_safe_host as th
    if open_:
        E, _ = _planted("point", 48, 1000)
        ac, p, tp = _pack(E, learner, 64, 64)
        out, steps = _call(E, learner, p, tp, 8, episode=True, **correct_kw(learner, "point")), 8
    else:
        out, steps = runs(learner)['out'], T
    g = _npo(out)
    L = _lengths(g['first_done'], steps)
    assert (L < steps).any() and (L == steps).any() == open_     # L == T needs an env that never finishes
    got = episode_rollout_batch(out)
    host = episode_rollout_batch({k: (v.cpu() if torch.is_tensor(v) else v) for k, v in out.items()})
    extra = ('act_safe', 'cost', 'prev_cost') if learner == "safelayer" else ('act_safe', 'cost', 'targetc')
    assert set(got) == set(host) == {'obs', 'act', 'ret', 'adv', 'logp', 'mu', 'logstd', 'n_valid'} | set(extra)
    assert got['n_valid'] == host['n_valid'] == int(L.sum())
    for k in got:
        if k != 'n_valid':
            np.testing.assert_array_equal(bits(got[k].cpu().numpy()), bits(host[k].numpy()), err_msg=k)
            assert got[k].shape[0] == got['n_valid']
    want = th.safe_episode_batch_np(g, learner)
    for k in ('obs', 'act', 'logp', 'mu', 'logstd') + extra:
        np.testing.assert_array_equal(bits(got[k].cpu().numpy()), bits(want[k]), err_msg=k)
    th._close(host, want, ('ret', 'adv'))
    if learner != "safelayer":
        last = np.cumsum(L) - 1                                    # t = L - 1: qc counts as 0, the target is the cost
        tc = got['targetc'].cpu().numpy()
        np.testing.assert_array_equal(bits(tc[last]), bits(g['cost'][L - 1, np.arange(len(L))] + np.float32(0)))
        for e in np.flatnonzero(L == steps):                       # L == T: every target but the last looks one row ahead
            off = int(L[:e].sum())
            np.testing.assert_array_equal(bits(tc[off:off + steps - 1]),
                                          bits(g['cost'][:-1, e] + np.float32(0.99) * g['qc'][1:, e]))
    if open_:
        E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. nothing is reset
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("learner", LEARNERS)
def test_nothing_is_reset(runs, learner):
    """after an episode=True call no env was re-initialised (the planted layout rows are all there) and the layout-pool
    prefetch saw nothing"""
    import torch
    run = runs(learner)
    torch.cuda.synchronize()
    after = run['E'].get_state()
    assert (run['g']['first_done'] > 0).any()
    np.testing.assert_array_equal(after['objs'], run['s']['objs'])
    assert run['E'].prefetch_stats() == run['stats0']
