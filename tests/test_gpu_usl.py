"""Engine.rollout_usl (the USL learner's collection loop on the device, guardx_amd/usl.py, libguardx_usl.so): bit equality
with rollout_policy in the warm-up branch, the iteration against a host loop that carries the running sum of the
passes' gradients and, pass by pass, against float64, the rollout against the probe and against a second engine driven
by act_safe, the update against its numpy float32 transcription, one pass against the float64 restatement
(tests/usl64.py, where the bounds are derived), the noise counter, errors and the batch helper.

Largest err / bound per output of test_single_pass_against_float64 are printed by the test (pytest -s) and recorded in
INTEGRATION.md.  Edge rows (tests/usl64.py) may differ in `stop` only and are at most 2 % of every case
(tests/test_usl_host.py::test_probe_inputs_are_sized sizes the inputs on the CPU)."""
import math

import numpy as np
import pytest

from helpers import assert_state_equal
from test_policy64 import make_ac, two_layer_net, Stub
from test_gpu_statewise import _cfg, _engine, _np, COSTLY, SEED
import usl64

pytestmark = pytest.mark.gpu

EDGE_CAP = 0.02
ETA = 0.05
F = np.float32


def make_q(D, A, hc, seed, w1=1.5, w2=2.0, w3=2.0, b3=0.0, zero_action=False):
    """a C_Critic-shaped module: .c_net = mlp([D + A, hc, hc, 1], tanh, output_activation=Softplus)"""
    import torch
    import torch.nn as nn
    torch.manual_seed(seed)
    net = two_layer_net(D + A, hc, 1, nn.Tanh, nn.Softplus)
    lin = [m for m in net if isinstance(m, nn.Linear)]
    with torch.no_grad():
        nn.init.normal_(lin[0].weight, std=w1 / math.sqrt(D + A))
        nn.init.normal_(lin[0].bias, std=0.5)
        nn.init.normal_(lin[1].weight, std=w2 / math.sqrt(hc))
        nn.init.normal_(lin[1].bias, std=0.3)
        nn.init.normal_(lin[2].weight, std=w3 / math.sqrt(hc))
        lin[2].bias.fill_(b3)
        if zero_action:
            lin[0].weight[:, D:] = 0.0
    return Stub(c_net=net)


# name: (D, A, hc, make_q keywords, delta).  The first three: plain networks at the robots' widths with delta near the
# median of q0, so that every stop reason occurs; then saturated tanh units, z3 around the Softplus threshold 20, z3 below
# -87 (exp flushes to zero: s = 0, Z = 0, the 1e-8 decides; delta = -1 keeps q > delta on both sides), and a zero
# action block (a zero gradient in exact arithmetic too)
PROBE_CASES = {
    "point64": (43, 2, 64, {}, 0.9),
    "ant256": (64, 8, 256, {}, 0.9),
    "walker128": (70, 10, 128, {}, 0.9),
    "saturated192": (46, 2, 192, dict(w1=12.0, w2=8.0), 0.7),
    "threshold20": (43, 2, 64, dict(b3=20.0, w3=1.0), 0.0),
    "below-87": (43, 2, 64, dict(b3=-95.0, w3=1.0), -1.0),
    "zero-gradient": (43, 2, 128, dict(zero_action=True), 0.0),
}
PROBE_N = 3000


def probe_inputs(name):
    """(module, obs, act, delta) of a case: random rows, a tenth of them with one component exactly 1 and none above"""
    D, A, hc, kw, delta = PROBE_CASES[name]
    seed = sorted(PROBE_CASES).index(name)
    qm = make_q(D, A, hc, 50 + seed, **kw)
    rng = np.random.default_rng(seed)
    obs = rng.normal(size=(PROBE_N, D)).astype(F)
    act = (rng.normal(size=(PROBE_N, A)) * 0.6).astype(F)
    one = np.arange(PROBE_N) % 10 == 0
    act[one] = np.minimum(act[one], F(0.99))
    act[one, rng.integers(0, A, size=int(one.sum()))] = F(1.0)
    return qm, obs, act, delta


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def _probe(qp, obs, act, **kw):
    import torch
    from guardx_amd.usl import correction_probe
    out = correction_probe(qp, torch.from_numpy(np.ascontiguousarray(obs, F)).cuda(),
                           torch.from_numpy(np.ascontiguousarray(act, F)).cuda(), **kw)
    return {k: v.cpu().numpy() for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------------------
# 1. the warm-up branch
# ---------------------------------------------------------------------------------------------------------------------
TWIN_KEYS = ('obs', 'act', 'mu', 'logp', 'val', 'rew', 'cost', 'done', 'obs_last', 'val_last', 'logstd')


def _warmup_runs(cfg, h, hc, T, T2, seed, **ekw):
    from guardx_amd import Engine
    E, Et = _engine(cfg, **ekw), _engine(cfg, **ekw)
    Et.set_policy_impl(3)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = make_ac(D, A, h, seed=seed, shift=h // 64), make_q(D, A, hc, seed + 1)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    runs = []
    for steps in (T, T2):
        g = _np(E.rollout_usl(p, steps, q_critic=qp, noise_seed=SEED, correct=False))
        w = _np(Et.rollout_policy(p, steps, noise_seed=SEED))
        runs.append((g, w))
    return E, Et, runs, qm


def _assert_warmup_equal(g, w, what):
    for k in TWIN_KEYS:
        np.testing.assert_array_equal(bits(g[k]), bits(w[k]), err_msg=f"{what} {k}")
    np.testing.assert_array_equal(bits(g['act_safe']), bits(g['act']), err_msg=f"{what} act_safe")
    assert (g['iters'] == 0).all() and np.isfinite(g['qc']).all() and (g['qc'] >= 0).all()


@pytest.mark.parametrize("robot,h,hc,N", [("point", 64, 64, 1), ("point", 256, 256, 2000), ("swimmer", 64, 64, 17),
                                          ("swimmer", 256, 256, 203), ("ant", 64, 64, 2000), ("ant", 256, 256, 17),
                                          ("walker", 64, 64, 203), ("walker", 256, 256, 1)])
def test_warmup_is_bit_equal_to_rollout_policy(robot, h, hc, N):
    """correct=False: the actor, v, the noise and the env give rollout_policy's bits (step-wise form on a twin engine),
    over resets inside the call (num_steps 5 < T) and a second call that continues the noise counter; qc is Q(obs, act)
    within the float64 bound; and the engine is left as rollout_policy leaves it"""
    import torch
    T, T2 = (12, 5) if N < 2000 else (8, 3)
    E, Et, runs, qm = _warmup_runs(_cfg(robot, N), h, hc, T, T2, seed=h + N)
    for i, (g, w) in enumerate(runs):
        _assert_warmup_equal(g, w, f"{robot} h={h} N={N} call {i}")
    assert N < 17 or runs[0][0]['done'][:-1].sum() > 0
    np.testing.assert_array_equal(runs[1][0]['obs'][0], runs[0][0]['obs_last'])
    g = runs[0][0]
    r = usl64.QCritic(qm).forward(g['obs'][:3], g['act'][:3])
    assert (np.abs(g['qc'][:3] - r['q']) <= r['dq']).all()
    torch.cuda.synchronize()
    assert_state_equal(E.get_state(), Et.get_state())
    for a, b in ((E._obs, Et._obs), (E._reward, Et._reward), (E._done, Et._done), (E._info['cost'], Et._info['cost'])):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    E.close()
    Et.close()


def test_warmup_bit_equal_on_the_thread_per_env_path():
    """env_num = 20000: the step launch does not speculate reset_done, gx_reset_done runs as a launch of its own"""
    wide = dict(placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)       # enough valid layouts for 20000 envs
    E, Et, runs, _ = _warmup_runs(_cfg("point", 20000, seed=4, **wide), 64, 64, 9, 2, seed=9, n_candidates=400000)
    assert E._spec.value == 0                                                   # the launch did not speculate
    for i, (g, w) in enumerate(runs):
        _assert_warmup_equal(g, w, f"N=20000 call {i}")
    assert runs[0][0]['done'][:-1].sum() > 0
    E.close()
    Et.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the iteration carries the running sum of its passes' gradients (usl_core.py:180-194: act.grad is never cleared)
# ---------------------------------------------------------------------------------------------------------------------
MULTI_CASES = ["point64", "ant256", "walker128", "saturated192"]
MULTI_ROWS = (1, 15, 16, 17, 33)                  # 16 rows per workgroup
MULTI_SCALES = (1.0, 1.0 / 2000)
MULTI_PASSES = 20
# Rows MULTI_ROW0[case] .. of probe_inputs: with 33 rows or fewer the 2 % cap on edge rows allows none, and over 20 passes
# float64 finds one to three in most windows of 33 rows (q within dq of delta at some pass).  Each case starts at the first
# row (for ant256 the window used so far) from which float64 finds no edge row in 33 rows at either scale, whose first row
# runs all 20 passes -- so that n = 1 carries a running sum too -- and whose first 15 rows hold a row that never moves
# (tests/test_usl_host.py::test_multi_pass_inputs_are_sized)
MULTI_ROW0 = {"point64": 34, "ant256": 99, "walker128": 45, "saturated192": 14}
_host_loops = {}


def host_loop(name, n, gs):
    """The iteration on n rows of a case (from MULTI_ROW0[case]), driven by the host from niter = 1 probes, computed once per (case, n,
    grad_scale) and shared: at each pass the probe's grad0 at the current a is added in float32 to the host's acc (the
    first pass's grad0 IS acc), the step is usl64.update32(a, acc, eta), a stopped row stays where it is.  -> (qp, obs,
    act, delta, passes); passes[p - 1] = dict(a_in, grad0, stop1 (the niter = 1 probe's stop at a_in), live (rows that
    moved in pass p), a, iters, stop (the state after p passes: what correction_probe(niter = p) has to return))"""
    key = (name, n, gs)
    if key not in _host_loops:
        from guardx_amd import Engine
        qm, obs, act, delta = probe_inputs(name)
        r0 = MULTI_ROW0[name]
        obs, act = obs[r0:r0 + n], act[r0:r0 + n]
        qp = Engine.pack_q_critic(qm, device='cuda')
        _host_loops[key] = (qm, qp, obs, act, delta, _drive_passes(qp, obs, act, delta, gs, MULTI_PASSES))
    return _host_loops[key]


def _drive_passes(qp, obs, act, delta, gs, npasses):
    """host_loop's passes on given rows"""
    n = len(act)
    a, acc = act.copy(), None
    iters, stop, passes = np.zeros(n, np.int64), np.zeros(n, np.int64), []
    for p in range(1, npasses + 1):
        r = _probe(qp, obs, a, delta=delta, niter=1, eta=ETA, grad_scale=gs)
        fixed = r['stop'] != 0
        np.testing.assert_array_equal(bits(r['a_safe'][fixed]), bits(a[fixed]))      # a stopped row is a fixed point
        assert (r['iters'][fixed] == 0).all() and (r['iters'][~fixed] == 1).all()
        assert (r['stop'][stop != 0] == stop[stop != 0]).all()                       # and stops for the same reason
        stop = np.where(stop == 0, r['stop'], stop)
        live = stop == 0
        acc = r['grad0'].copy() if acc is None else (acc + r['grad0']).astype(F)
        a_in, a = a, np.where(live[:, None], usl64.update32(a, acc, ETA), a).astype(F)
        iters = iters + live
        passes.append(dict(a_in=a_in, grad0=r['grad0'].copy(), stop1=r['stop'].copy(), live=live, a=a.copy(),
                           iters=iters.copy(), stop=stop.copy()))
    return passes


@pytest.mark.parametrize("gs", MULTI_SCALES)
@pytest.mark.parametrize("n", MULTI_ROWS)
@pytest.mark.parametrize("name", MULTI_CASES)
def test_iteration_accumulates_the_gradient(name, n, gs):
    """correction_probe(niter = k) equals the host loop of host_loop() after k passes for k = 2, 3, 5, 20: a_safe bit for
    bit, iters and stop equal.  (The memoryless iteration -- niter = 1 applied k times, feeding a_safe back -- which the
    library computed before, differs from it on every row that moves twice.)"""
    qm, qp, obs, act, delta, passes = host_loop(name, n, gs)
    for k in (2, 3, 5, 20):
        r = _probe(qp, obs, act, delta=delta, niter=k, eta=ETA, grad_scale=gs)
        w = passes[k - 1]
        np.testing.assert_array_equal(bits(r['a_safe']), bits(w['a']), err_msg=f"{name} n={n} k={k}")
        np.testing.assert_array_equal(r['iters'], w['iters'], err_msg=f"{name} n={n} k={k}")
        np.testing.assert_array_equal(r['stop'], w['stop'], err_msg=f"{name} n={n} k={k}")
        np.testing.assert_array_equal(bits(r['grad0']), bits(passes[0]['grad0']), err_msg=f"{name} n={n} k={k}")
    assert r['iters'][0] == MULTI_PASSES and passes[1]['live'][0]      # at every n the first row carries a running sum
    if n == 33:
        # the sizing of tests/test_usl_host.py::test_multi_pass_inputs_are_sized: rows that run all 20 passes, rows that
        # stop, and the running sum matters (some row moves twice or more and its second step is not the memoryless one)
        assert r['iters'].max() == MULTI_PASSES and len(set(np.unique(r['stop']))) >= 2
        twice = passes[1]['live']
        memoryless = usl64.update32(passes[1]['a_in'], passes[1]['grad0'], ETA)
        assert twice.any() and (bits(memoryless[twice]) != bits(passes[1]['a'][twice])).any()


@pytest.mark.parametrize("A", [2, 4, 6, 8, 10, 12, 14, 16])
def test_accumulation_at_every_action_width(A):
    """the row update is compiled once per action width (gx_usl.hip:q_update<A>): every width against the host loop,
    niter = 1 .. 6 bit for bit, on 17 rows of a 64-wide c_net with delta at the median of q0"""
    from guardx_amd import Engine
    n, D = 17, 43
    qm = make_q(D, A, 64, 80 + A)
    rng = np.random.default_rng(300 + A)
    obs = rng.normal(size=(n, D)).astype(F)
    act = (rng.normal(size=(n, A)) * 0.4 / math.sqrt(A / 2)).astype(F)
    delta = float(F(np.median(usl64.QCritic(qm).forward(obs, act)['q'])))
    qp = Engine.pack_q_critic(qm, device='cuda')
    passes = _drive_passes(qp, obs, act, delta, 1.0 / n, 6)
    for k in range(1, 7):
        r = _probe(qp, obs, act, delta=delta, niter=k, eta=ETA, grad_scale=1.0 / n)
        w = passes[k - 1]
        np.testing.assert_array_equal(bits(r['a_safe']), bits(w['a']), err_msg=f"A={A} k={k}")
        np.testing.assert_array_equal(r['iters'], w['iters'], err_msg=f"A={A} k={k}")
        np.testing.assert_array_equal(r['stop'], w['stop'], err_msg=f"A={A} k={k}")
    assert r['iters'].max() >= 3 and (r['iters'] == 0).any()          # rows that carry a sum, rows that never move
    assert np.isfinite(r['a_safe']).all()


@pytest.mark.parametrize("gs", MULTI_SCALES)
@pytest.mark.parametrize("n", MULTI_ROWS)
@pytest.mark.parametrize("name", MULTI_CASES)
def test_multi_pass_against_float64(name, n, gs):
    """Pass by pass over the 20 passes: from the device's own action before the pass (correction_probe(niter = p - 1)'s
    a_safe) and the float64 sum of the device's own grad0s of the passes before it, correction_probe(niter = p)'s a_safe
    lies within usl64.one_pass's bound of the float64 step, and its stop equals float64's, on the rows that have not been
    edge rows so far; edge rows are at most 2 % of the rows."""
    qm, qp, obs, act, delta, passes = host_loop(name, n, gs)
    Q = usl64.QCritic(qm)
    acc, dacc = None, None
    ok, stopped = np.ones(n, bool), np.zeros(n, bool)
    a_dev, worst = act, 0.0
    for p in range(1, MULTI_PASSES + 1):
        r = _probe(qp, obs, act, delta=delta, niter=p, eta=ETA, grad_scale=gs)
        w = Q.one_pass(obs, a_dev, delta, ETA, gs, acc=acc, dacc=dacc)
        ok &= stopped | ~w['edge']
        rows = ok & ~stopped
        moved = rows & (w['stop'] < 0)
        np.testing.assert_array_equal(r['stop'][rows], np.where(w['stop'][rows] < 0, 0, w['stop'][rows]), err_msg=f"pass {p}")
        np.testing.assert_array_equal(bits(r['a_safe'][rows & ~moved]), bits(a_dev[rows & ~moved]), err_msg=f"pass {p}")
        err = np.abs(r['a_safe'] - w['a_next'])[moved]
        if moved.any():
            with np.errstate(divide='ignore', invalid='ignore'):
                worst = max(worst, float(np.where(err == 0, 0.0, err / w['da_next'][moved]).max()))
        stopped |= w['stop'] > 0
        # the float64 sum of the device's own grad0s at the device's own actions, and what the device's fp32 sum may be off
        g = passes[p - 1]['grad0'].astype(np.float64)
        np.testing.assert_array_equal(bits(passes[p - 1]['a_in'][rows]), bits(a_dev[rows]))
        acc = g if acc is None else acc + g
        dacc = np.zeros_like(g) if dacc is None else dacc + usl64.MARGIN * usl64.U * np.abs(acc)
        a_dev = r['a_safe']
    share = float((~ok).mean())
    print(f"usl multi pass {name} n={n} gs={gs:g}: edge rows {share:.4f}  a_safe err / bound {worst:.3f}  "
          f"rows at 20 passes {int((r['iters'] == MULTI_PASSES).sum())}")
    assert share <= EDGE_CAP, share
    assert np.isfinite(a_dev).all()
    assert worst <= 1.0, worst


# ---------------------------------------------------------------------------------------------------------------------
# 3. the rollout against the probe and against a second engine
# ---------------------------------------------------------------------------------------------------------------------
ROLLOUT_CASES = [("point", 64, 64, 0.6), ("ant", 256, 128, 0.3), ("swimmer", 128, 256, 0.0)]
ROLLOUT_N, ROLLOUT_CFG_SEED = 203, 7


def rollout_nets(D, A, h, hc):
    """the networks of the rollout tests: an actor whose samples stay inside the box (output layer scaled by 0.3,
    log_std = -1.5: |a| stays well below 1 even at A = 8), so that rows pass the max a > 1 test and iterate, and a c_net
    whose q0 straddles the cases' delta.  Sized on the CPU checker's engine with the float64 restatement alone
    (tests/test_usl_host.py::test_rollout_inputs_are_sized): on the first step at least 45 % of the rows move, which
    leaves room for the 30 % the GPU test asks for over the whole trajectory."""
    import torch
    import torch.nn as nn
    ac, qm = make_ac(D, A, h, seed=h + A, shift=1), make_q(D, A, hc, 3 + hc)
    with torch.no_grad():
        ac.pi.log_std.fill_(-1.5)
        last = [m for m in ac.pi.mu_net if isinstance(m, nn.Linear)][2]
        last.weight.mul_(0.3)
        last.bias.mul_(0.3)
    return ac, qm


@pytest.mark.parametrize("robot,h,hc,delta", ROLLOUT_CASES)
def test_rollout_equals_the_probe_and_steps_the_env_on_act_safe(robot, h, hc, delta):
    import torch
    from guardx_amd import Engine
    N, T = ROLLOUT_N, 9
    cfg = _cfg(robot, N, seed=ROLLOUT_CFG_SEED, **COSTLY)
    E, Et = _engine(cfg), _engine(cfg)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = rollout_nets(D, A, h, hc)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    out = E.rollout_usl(p, T, q_critic=qp, noise_seed=SEED, delta=delta)
    g = _np(out)
    stops = set()
    for t in range(T):
        r = _probe(qp, g['obs'][t], g['act'][t], delta=delta, niter=20, eta=0.05, grad_scale=1.0 / N)
        np.testing.assert_array_equal(bits(g['act_safe'][t]), bits(r['a_safe']), err_msg=f"t={t}")
        np.testing.assert_array_equal(bits(g['qc'][t]), bits(r['q0']), err_msg=f"t={t}")
        np.testing.assert_array_equal(g['iters'][t], r['iters'].astype(F), err_msg=f"t={t}")
        stops |= set(np.unique(r['stop']).tolist())
    assert (g['iters'] > 0).mean() > 0.3 and (g['act_safe'] != g['act']).any() and len(stops) >= 2
    obs, rew, cost, done = (x.cpu().numpy() for x in Et.rollout(out['act_safe']))
    np.testing.assert_array_equal(bits(obs[:-1]), bits(g['obs'][1:]))
    np.testing.assert_array_equal(bits(obs[-1]), bits(g['obs_last']))
    for k, w in (('rew', rew), ('cost', cost), ('done', done)):
        np.testing.assert_array_equal(bits(g[k]), bits(w), err_msg=k)
    assert g['done'][:-1].sum() > 0
    E.close()
    Et.close()


# ---------------------------------------------------------------------------------------------------------------------
# 4. one update is the float32 transcription
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROBE_CASES))
def test_one_update_is_update32_bit_for_bit(name):
    from guardx_amd import Engine
    qm, obs, act, delta = probe_inputs(name)
    qp = Engine.pack_q_critic(qm, device='cuda')
    for gs in (1.0, 1.0 / 2000):
        r = _probe(qp, obs, act, delta=delta, niter=1, eta=ETA, grad_scale=gs)
        moved = r['iters'] == 1
        np.testing.assert_array_equal(moved, r['stop'] == 0)
        np.testing.assert_array_equal(bits(r['a_safe'][moved]), bits(usl64.update32(act[moved], r['grad0'][moved], ETA)))
        np.testing.assert_array_equal(bits(r['a_safe'][~moved]), bits(act[~moved]))
        assert (r['grad0'][~moved] == 0).all()
        assert moved.any()


# ---------------------------------------------------------------------------------------------------------------------
# 5. one pass against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROBE_CASES))
def test_single_pass_against_float64(name):
    """q0, grad0 and the one-step a_safe within the bounds derived in tests/usl64.py on the rows that are not edge rows,
    stop equal there; edge rows at most 2 %"""
    from guardx_amd import Engine
    qm, obs, act, delta = probe_inputs(name)
    qp = Engine.pack_q_critic(qm, device='cuda')
    r = _probe(qp, obs, act, delta=delta, niter=1, eta=ETA, grad_scale=1.0)
    w = usl64.QCritic(qm).one_pass(obs, act, delta, ETA, 1.0)
    ok = ~w['edge']
    share = float(w['edge'].mean())
    moved = (w['stop'] < 0) & ok
    def ratio(got, want, bound, rows):
        err = np.abs(got - want)[rows]
        with np.errstate(divide='ignore', invalid='ignore'):          # an exact value with a zero bound counts as 0
            return float(np.where(err == 0, 0.0, err / bound[rows]).max()) if rows.any() else 0.0

    ratios = dict(q0=ratio(r['q0'], w['q'], w['dq'], np.ones(len(obs), bool)), grad0=ratio(r['grad0'], w['s'], w['ds'], moved),
                  a_safe=ratio(r['a_safe'], w['a_next'], w['da_next'], moved))
    print(f"usl single pass {name}: edge rows {share:.4f}  " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + f"  median bounds q0 {np.median(w['dq']):.2e} grad0 {np.median(w['ds']):.2e} a_safe {np.median(w['da_next'][moved]) if moved.any() else 0:.2e}")
    assert share <= EDGE_CAP, share
    assert np.isfinite(r['q0']).all() and np.isfinite(r['a_safe']).all()
    np.testing.assert_array_equal(r['stop'][ok], np.where(w['stop'][ok] < 0, 0, w['stop'][ok]))
    np.testing.assert_array_equal(bits(r['a_safe'][ok & (w['stop'] > 0)]), bits(act[ok & (w['stop'] > 0)]))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the noise counter
# ---------------------------------------------------------------------------------------------------------------------
def test_noise_counter_across_calls_reset_and_other_paths():
    """three calls of 5 + 4 + 3 steps match policy64 at the step counters 0 .. 11 and not at 0 again; a reset(), step(),
    reset_done() and interleaved rollout_policy, rollout_statewise and rollout_safelayer calls leave the counter alone,
    and rollout_usl leaves theirs alone"""
    import torch
    from guardx_amd import Engine
    from oracle import policy64
    from test_gpu_safelayer import make_g
    from test_gpu_statewise import _aug_ac, _softplus_critic
    N = 64
    E = _engine(_cfg("point", N, seed=5))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = make_ac(D, A, 64, seed=3), make_q(D, A, 64, 4)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    gp = Engine.pack_g_net(make_g(D, A, 64, 5), device='cuda')
    acs, _ = _aug_ac(D, A, 64, seed=6, zero_m=False)
    ps = Engine.pack_actor_critic(acs).cuda()
    vcs = Engine.pack_critic(_softplus_critic(D + 1, 64, 7)[0], output='softplus', device='cuda')
    A64 = policy64.ActorCritic(ac)
    t0 = 0
    for call, T in enumerate((5, 4, 3)):
        g = _np(E.rollout_usl(p, T, q_critic=qp, noise_seed=SEED))
        want = policy64.rollout(A64, g, SEED, t0=t0)
        policy64.compare(g, want, keys=('mu', 'act', 'logp', 'val'), what=f"call {call} t0={t0}")
        if t0:
            wrong = policy64.rollout(A64, g, SEED, t0=0)
            assert (np.abs(g['act'] - wrong['act']) > wrong['act_b']).any()
        t0 += T
        if call == 0:
            E.step(torch.zeros(N, A, device='cuda'))
            E.reset_done()
            E.rollout_policy(p, 3, noise_seed=SEED)
            E.rollout_safelayer(p, 2, g_net=gp, noise_seed=SEED)
            E.rollout_statewise(ps, 2, cost_critic=vcs, noise_seed=SEED)
        if call == 1:
            E.reset()
    assert E._usl.steps == 12 and E._safelayer.steps == 2 and E._statewise.steps == 2
    # the safelayer path's own counter was not advanced by rollout_usl: its next call continues at 2
    g = _np(E.rollout_safelayer(p, 2, g_net=gp, noise_seed=SEED, correct=False))
    want = policy64.rollout(A64, g, SEED, t0=2)
    policy64.compare(g, want, keys=('act',), what="safelayer after usl")
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import ctypes as C
    import torch
    from guardx_amd import Engine, _usl_native as n
    from guardx_amd.usl import correction_probe
    N = 32
    E = _engine(_cfg("point", N))
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = make_ac(D, A, 64, seed=1), make_q(D, A, 64, 2)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    with pytest.raises(RuntimeError, match="before reset"):
        E.rollout_usl(p, 3, q_critic=qp)
    E.reset()
    state = E.get_state()
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_usl(p, 3, q_critic=qp.clone())                    # a copy carries no declaration
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_usl(p, 3, q_critic=None)
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_usl(p, 3, q_critic=Engine.pack_critic(make_ac(D, 1, 64).v, device='cuda'))
    with pytest.raises(ValueError, match=r"q_critic has \d+ floats"):
        E.rollout_usl(p, 3, q_critic=Engine.pack_q_critic(make_q(D + 1, A, 64, 2), device='cuda'))   # a wrong input width
    with pytest.raises(ValueError, match="T must be >= 1"):
        E.rollout_usl(p, 0, q_critic=qp)
    with pytest.raises(ValueError, match="niter must be >= 0"):
        E.rollout_usl(p, 3, q_critic=qp, niter=-1)
    with pytest.raises(ValueError, match=r"params has \d+ floats"):
        E.rollout_usl(p[:-1], 3, q_critic=qp)
    obs, act = torch.zeros(4, D, device='cuda'), torch.zeros(4, A, device='cuda')
    with pytest.raises(ValueError, match="niter"):
        correction_probe(qp, obs, act, niter=-1)
    with pytest.raises(ValueError, match=r"floats"):
        correction_probe(qp[:-1].clone(), obs, act)
    lib = n.load()
    out = [torch.zeros(4 * 3, device='cuda') for _ in range(5)]
    work = torch.zeros(int(lib.gxu_probe_work_floats(D, A, 64)), device='cuda')

    def raw(D_, A_, hc, niter=1):
        return lib.gxu_correction_probe(4, D_, A_, hc, qp.data_ptr(), work.data_ptr(), obs.data_ptr(), act.data_ptr(), 0.0,
                                        niter, 0.05, 1.0, *(o.data_ptr() for o in out), None)
    assert raw(D, A, 64, niter=-1) == n.GXU_ERR_ARG
    assert raw(D, A, 96) == n.GXU_ERR_UNSUPPORTED                   # a width outside the four
    assert raw(D, 3, 64) == n.GXU_ERR_UNSUPPORTED                   # an odd A
    a = n.GxuStepArgs()
    a.struct_size = C.sizeof(n.GxuStepArgs) - 8
    assert lib.gxu_policy_step(C.byref(a), None) == n.GXU_ERR_ARG and b"struct_size" in lib.gxu_last_error()
    torch.cuda.synchronize()
    assert all((o == 0).all() for o in out)                         # nothing was launched
    assert_state_equal(E.get_state(), state)
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. the batch helper
# ---------------------------------------------------------------------------------------------------------------------
def test_usl_rollout_batch_on_device():
    """the batch helper's device path on a real rollout against its host form and the numpy restatement of USLBufferX"""
    import torch
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import usl_rollout_batch
    from test_usl_host import usl_batch_np
    N, T = 67, 24
    E = _engine(_cfg("point", N, seed=9, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = rollout_nets(D, A, 64, 64)
    out = E.rollout_usl(Engine.pack_actor_critic(ac).cuda(), T, q_critic=Engine.pack_q_critic(qm, device='cuda'),
                        noise_seed=SEED, delta=0.5)
    g = _np(out)
    assert g['done'][:-1].sum() > 0 and (g['act_safe'] != g['act']).any()
    got, want = _np(usl_rollout_batch(out)), usl_batch_np(g)
    host = _np(usl_rollout_batch({k: v.cpu() for k, v in out.items()}))
    assert set(got) == set(want) == set(host)
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=tol, err_msg=k)
        np.testing.assert_allclose(got[k], host[k], rtol=tol, atol=tol, err_msg=k)
    E.close()
