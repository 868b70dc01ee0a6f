"""Engine.rollout_lpg (the LPG learner's collection loop on the device, guardx_amd/lpg.py, libguardx_lpg.so): bit equality
with rollout_policy in the warm-up branch, the projection as a pure map, c_net against the USL library's verified chain,
the projection against its numpy float32 transcription and against the float64 restatement (tests/lpg64.py, where the
bounds are derived), the rollout against the probe and against a second engine driven by act_safe, q_init and the noise
counter, errors and the batch helper.

Largest err / bound per output of test_probe_against_float64 are printed by the test (pytest -s) and recorded in
INTEGRATION.md.  Edge rows (tests/lpg64.py) may differ in `branch` only and are at most 2 % of every case
(tests/test_lpg_host.py::test_probe_inputs_are_sized sizes the inputs on the CPU)."""
import functools

import numpy as np
import pytest

from helpers import assert_state_equal
from test_policy64 import make_ac
from test_gpu_statewise import _cfg, _engine, _np, COSTLY, SEED
from test_gpu_usl import make_q, rollout_nets, bits, TWIN_KEYS
import lpg64
import usl64

pytestmark = pytest.mark.gpu

EDGE_CAP = 0.02
F = np.float32

# name: (D, A, hc, make_q keywords, spread of q_init around delta).  Plain networks at the robots' widths (A = 2: Point,
# A = 8: Ant with its padded action k-steps, A = 10), every h_c (64: W2 in LDS; 128, 192: 8 and 12 waves; 256: two tiles
# per wave, streamed), a first layer with about half of its tanh units saturated, and z3 on both sides of the Softplus
# threshold 20.  delta is the 30 % quantile of q, so 30 % of the rows keep their action; q_init lies close to delta, so
# that eps = |delta - q_init| is small against G . a and the corrected rows fall on both sides of lam = 0.  The weight
# scales are smaller than the USL tests': the float64 bound on G (tests/usl64.py) is an absolute one per hidden unit, and
# with these scales it stays below 1e-3 of what it bounds (tests/test_lpg_host.py::test_probe_inputs_are_sized).
_PLAIN = dict(w1=0.5, w2=0.5, w3=1.0)
PROBE_CASES = {
    "point64": (43, 2, 64, _PLAIN, 0.002),
    "ant256": (64, 8, 256, _PLAIN, 0.002),
    "walker128": (70, 10, 128, _PLAIN, 0.002),
    "saturated192": (46, 2, 192, dict(w1=4.0, w2=0.15, w3=0.5), 0.002),
    "threshold20": (43, 2, 64, dict(_PLAIN, b3=19.3), 0.002),
}
PROBE_N = 3000


@functools.lru_cache(maxsize=None)
def probe_inputs(name):
    """(module, obs, act, q_init, delta) of a case; computed once and shared (callers do not modify the arrays)"""
    D, A, hc, kw, spread = PROBE_CASES[name]
    seed = sorted(PROBE_CASES).index(name)
    qm = make_q(D, A, hc, 70 + seed, **kw)
    rng = np.random.default_rng(100 + seed)
    obs = rng.normal(size=(PROBE_N, D)).astype(F)
    act = (rng.normal(size=(PROBE_N, A)) * 0.6).astype(F)
    delta = float(F(np.quantile(usl64.QCritic(qm).forward(obs, act)['q'], 0.3)))
    q_init = (delta + spread * rng.normal(size=PROBE_N)).astype(F)
    return qm, obs, act, q_init, delta


def _probe(qp, obs, act, q_init, **kw):
    import torch
    from guardx_amd.lpg import projection_probe
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x, F)).cuda()   # noqa: E731
    return {k: v.cpu().numpy() for k, v in projection_probe(qp, dev(obs), dev(act), dev(q_init), **kw).items()}


def _assert_bits_or_nan(got, want, msg):
    """bit equality, except that a NaN matches any NaN (numpy and the device may disagree on its sign and payload)"""
    got, want = np.asarray(got, F), np.asarray(want, F)
    nan = np.isnan(want)
    assert np.isnan(got[nan]).all(), msg
    np.testing.assert_array_equal(bits(got[~nan]), bits(want[~nan]), err_msg=msg)


# ---------------------------------------------------------------------------------------------------------------------
# 1. the warm-up branch
# ---------------------------------------------------------------------------------------------------------------------
def _warmup(cfg, h, hc, T, seed, **ekw):
    from guardx_amd import Engine
    E, Et = _engine(cfg, **ekw), _engine(cfg, **ekw)
    Et.set_policy_impl(3)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = make_ac(D, A, h, seed=seed, shift=h // 64), make_q(D, A, hc, seed + 1)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    g = _np(E.rollout_lpg(p, T, q_critic=qp, noise_seed=SEED, correct=False))
    w = _np(Et.rollout_policy(p, T, noise_seed=SEED))
    for k in TWIN_KEYS:
        np.testing.assert_array_equal(bits(g[k]), bits(w[k]), err_msg=k)
    np.testing.assert_array_equal(bits(g['act_safe']), bits(g['act']))
    assert (g['lam'] == 0).all() and np.isfinite(g['qc']).all() and (g['qc'] >= 0).all()
    np.testing.assert_array_equal(bits(g['q_init']), bits(g['qc'][0]))
    return E, Et, g, qm


@pytest.mark.parametrize("robot,h,hc,N", [("point", 64, 64, 1), ("swimmer", 64, 128, 17), ("ant", 256, 256, 33)])
def test_warmup_is_bit_equal_to_rollout_policy(robot, h, hc, N):
    """correct=False: the actor, v, the noise and the env give rollout_policy's bits (step-wise form on a twin engine),
    with a reset_done inside the call (num_steps = 3: the env times out on its step 4, counted from 0, so T = 6 takes
    one more step from the reset state); qc is Q(obs, act) within the float64 bound; and the engine is left as
    rollout_policy leaves it"""
    import torch
    E, Et, g, qm = _warmup(_cfg(robot, N, num_steps=3), h, hc, 6, seed=h + N)
    assert g['done'][:-1].any()                                 # the time-out, and its reset_done, fell inside the call
    r = usl64.QCritic(qm).forward(g['obs'][:2], g['act'][:2])
    assert (np.abs(g['qc'][:2] - r['q']) <= r['dq']).all()
    torch.cuda.synchronize()
    assert_state_equal(E.get_state(), Et.get_state())
    for a, b in ((E._obs, Et._obs), (E._reward, Et._reward), (E._done, Et._done), (E._info['cost'], Et._info['cost'])):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    E.close()
    Et.close()


def test_warmup_bit_equal_on_the_thread_per_env_path():
    """env_num = 16400 (> 16384): the step launch does not speculate reset_done, gx_reset_done runs as a launch of its
    own"""
    wide = dict(placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)       # enough valid layouts for 16400 envs
    E, Et, g, _ = _warmup(_cfg("point", 16400, seed=4, num_steps=1, **wide), 64, 64, 2, seed=9, n_candidates=400000)
    assert E._spec.value == 0                                                   # the launch did not speculate
    E.close()
    Et.close()


# ---------------------------------------------------------------------------------------------------------------------
# 2. the probe is a pure map
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["point64", "ant256", "saturated192"])
def test_probe_is_a_pure_map(name):
    """the same rows in another order and another batch size (1001 of the 3000, shuffled: other workgroups, other lanes,
    a last workgroup with 9 rows) give the same bits"""
    from guardx_amd import Engine
    qm, obs, act, q_init, delta = probe_inputs(name)
    qp = Engine.pack_q_critic(qm, device='cuda')
    full = _probe(qp, obs, act, q_init, delta=delta)
    pick = np.random.default_rng(1).permutation(PROBE_N)[:1001]
    part = _probe(qp, obs[pick], act[pick], q_init[pick], delta=delta)
    for k in ('a_safe', 'q', 'G', 'lam'):
        np.testing.assert_array_equal(bits(part[k]), bits(full[k][pick]), err_msg=f"{name} {k}")
    np.testing.assert_array_equal(part['branch'], full['branch'][pick])
    assert set(np.unique(full['branch'])) == {0, 1, 2}


# ---------------------------------------------------------------------------------------------------------------------
# 3. c_net against the USL library's chain
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hc,A", [(64, 2), (128, 8), (192, 2), (256, 8)])
def test_q_and_gradient_equal_the_usl_probe_bit_for_bit(hc, A):
    """q is USL's q0 on the same (obs, act); G is USL's first-pass gradient at act = 0 (niter = 1, delta = -1: every row
    moves) with the same grad_scale.  USL evaluates the A action terms with a zero action where this path evaluates none:
    fmaf(0, w, acc) == acc for finite w unless acc is -0, which random networks do not produce."""
    import torch
    from guardx_amd import Engine
    from guardx_amd.usl import correction_probe
    D, n = 43 + A, 300
    qm = make_q(D, A, hc, 7 + hc)
    qp = Engine.pack_q_critic(qm, device='cuda')
    rng = np.random.default_rng(hc)
    obs, act = rng.normal(size=(n, D)).astype(F), (rng.normal(size=(n, A)) * 0.6).astype(F)
    dev = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
    for gs in (1.0, 1.0 / 2000):
        r = _probe(qp, obs, act, np.zeros(n, F), delta=0.0, grad_scale=gs)
        u = correction_probe(qp, dev(obs), dev(act), delta=-1.0, niter=1, grad_scale=gs)
        u0 = correction_probe(qp, dev(obs), dev(np.zeros_like(act)), delta=-1.0, niter=1, grad_scale=gs)
        np.testing.assert_array_equal(bits(r['q']), bits(u['q0'].cpu().numpy()))
        assert (u0['iters'].cpu().numpy() == 1).all()
        np.testing.assert_array_equal(bits(r['G']), bits(u0['grad0'].cpu().numpy()))
        assert (r['G'] != 0).any()


# ---------------------------------------------------------------------------------------------------------------------
# 4. the projection is its float32 transcription
# ---------------------------------------------------------------------------------------------------------------------
def _assert_project32(r, act, q_init, delta, sign, msg):
    a_safe, lam, branch = lpg64.project32(act, r['G'], r['q'], q_init, delta, sign)
    _assert_bits_or_nan(r['a_safe'], a_safe, msg + " a_safe")
    _assert_bits_or_nan(r['lam'], lam, msg + " lam")
    np.testing.assert_array_equal(r['branch'], branch, err_msg=msg + " branch")
    keep = r['branch'] == 0
    np.testing.assert_array_equal(bits(r['a_safe'][keep]), bits(act[keep]), err_msg=msg + " kept rows")


@pytest.mark.parametrize("name", sorted(PROBE_CASES))
def test_projection_is_project32_bit_for_bit(name):
    """a_safe, lam and branch from the probe's own G, q and q_init, for both signs and both gradient scales"""
    from guardx_amd import Engine
    qm, obs, act, q_init, delta = probe_inputs(name)
    qp = Engine.pack_q_critic(qm, device='cuda')
    for gs, sign in ((1.0, 1.0), (1.0, -1.0), (1.0 / 2000, 1.0)):
        r = _probe(qp, obs, act, q_init, delta=delta, grad_scale=gs, step_sign=sign)
        _assert_project32(r, act, q_init, delta, sign, f"{name} gs={gs} sign={sign}")
        if gs == 1.0:
            assert (r['branch'] == 1).any() and (r['a_safe'][r['branch'] == 1] != act[r['branch'] == 1]).any()


def test_projection_on_adversarial_rows():
    """G = 0 with eps > 0 (a_safe == act exactly), 0 / 0 (a NaN action, as the reference's division gives), top exactly
    0, q == delta exactly (the row keeps its action), and a gradient so large that G . G overflows"""
    from guardx_amd import Engine
    D, A, n = 43, 2, 64
    rng = np.random.default_rng(8)
    obs, act = rng.normal(size=(n, D)).astype(F), (rng.normal(size=(n, A)) * 0.6).astype(F)
    # a zero action block: G is exactly 0
    qz = Engine.pack_q_critic(make_q(D, A, 64, 5, zero_action=True), device='cuda')
    q_init = np.full(n, 0.25, F)
    q_init[::2] = F(-1.0)                                       # eps = 0 on the even rows (delta = -1), 1.25 on the odd
    r = _probe(qz, obs, act, q_init, delta=-1.0)
    assert (r['G'] == 0).all() and (r['branch'] == 2).all()
    np.testing.assert_array_equal(bits(r['a_safe'][1::2]), bits(act[1::2]))        # -eps / 0 = -inf -> lam = 0
    assert (r['lam'][1::2] == 0).all()
    assert np.isnan(r['a_safe'][::2]).all() and np.isnan(r['lam'][::2]).all()       # 0 / 0
    _assert_project32(r, act, q_init, -1.0, 1.0, "zero gradient")
    # top exactly 0: a zero action and eps = 0, on a plain network
    qm = make_q(D, A, 64, 6)
    qp = Engine.pack_q_critic(qm, device='cuda')
    zero = np.zeros_like(act)
    r = _probe(qp, obs, zero, np.full(n, -1.0, F), delta=-1.0)
    assert (r['branch'] == 2).all() and (r['lam'] == 0).all() and (r['a_safe'] == 0).all()
    _assert_project32(r, zero, np.full(n, -1.0, F), -1.0, 1.0, "top == 0")
    # q == delta exactly on row 0
    q0 = float(_probe(qp, obs, act, q_init, delta=0.0)['q'][0])
    r = _probe(qp, obs, act, q_init, delta=q0)
    assert r['branch'][0] == 0 and r['lam'][0] == 0
    _assert_project32(r, act, q_init, q0, 1.0, "q == delta")
    # a huge gradient: G . G overflows to inf, lam = top / inf is 0 or NaN
    r = _probe(qp, obs, act, q_init, delta=0.0, grad_scale=1e30, step_sign=-1.0)
    assert np.abs(r['G']).max() > 1e20
    _assert_project32(r, act, q_init, 0.0, -1.0, "huge G")


# ---------------------------------------------------------------------------------------------------------------------
# 5. the probe against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(PROBE_CASES))
def test_probe_against_float64(name):
    """q, G, lam and a_safe within the bounds derived in tests/lpg64.py (and tests/usl64.py) on the rows that are not
    edge rows, branch equal there; edge rows at most 2 %"""
    from guardx_amd import Engine
    qm, obs, act, q_init, delta = probe_inputs(name)
    qp = Engine.pack_q_critic(qm, device='cuda')
    r = _probe(qp, obs, act, q_init, delta=delta, grad_scale=1.0)
    w = lpg64.probe64(usl64.QCritic(qm), obs, act, q_init, delta, 1.0)
    ok = ~w['edge']
    share = float(w['edge'].mean())

    def ratio(got, want, bound, rows):
        err = np.abs(got - want)[rows]
        with np.errstate(divide='ignore', invalid='ignore'):          # an exact value with a zero bound counts as 0
            return float(np.where(err == 0, 0.0, err / bound[rows]).max()) if rows.any() else 0.0

    every = np.ones(PROBE_N, bool)
    ratios = dict(q=ratio(r['q'], w['q'], w['dq'], every), G=ratio(r['G'], w['G'], w['dG'], every),
                  lam=ratio(r['lam'], w['lam'], w['dlam'], ok), a_safe=ratio(r['a_safe'], w['a_safe'], w['da_safe'], ok))
    corr = ok & (w['branch'] == 1)
    print(f"lpg probe {name}: edge rows {share:.4f}  " + "  ".join(f"{k} {v:.3f}" for k, v in ratios.items())
          + f"  median bounds q {np.median(w['dq']):.2e} G {np.median(w['dG']):.2e} lam {np.median(w['dlam'][corr]):.2e}"
          f" a_safe {np.median(w['da_safe'][corr]):.2e}")
    assert share <= EDGE_CAP, share
    assert np.isfinite(r['q']).all() and np.isfinite(r['a_safe'][ok]).all()
    np.testing.assert_array_equal(r['branch'][ok], w['branch'][ok])
    np.testing.assert_array_equal(bits(r['a_safe'][ok & (w['branch'] != 1)]), bits(act[ok & (w['branch'] != 1)]))
    for k, v in ratios.items():
        assert v <= 1.0, (k, v)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the rollout against the probe and against a second engine
# ---------------------------------------------------------------------------------------------------------------------
# grad_scale = 8: eps = |delta - q_init| does not scale with the gradient, G . a does, so the corrected rows fall on both
# sides of lam = 0 (with the reference's 1 / env_num almost every lam is clipped to 0)
@pytest.mark.parametrize("robot,h,hc,delta", [("point", 64, 64, 0.6), ("ant", 256, 128, 0.3), ("swimmer", 128, 256, 0.0)])
def test_rollout_equals_the_probe_and_steps_the_env_on_act_safe(robot, h, hc, delta):
    from guardx_amd import Engine
    N, T, gs = 17, 5, 8.0
    cfg = _cfg(robot, N, seed=7, **dict(COSTLY, num_steps=2))   # the time-out falls on step 3 of the 5
    E, Et = _engine(cfg), _engine(cfg)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = rollout_nets(D, A, h, hc)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    out = E.rollout_lpg(p, T, q_critic=qp, noise_seed=SEED, delta=delta, grad_scale=gs)
    g = _np(out)
    np.testing.assert_array_equal(bits(g['q_init']), bits(g['qc'][0]))
    branches = set()
    for t in range(T):
        r = _probe(qp, g['obs'][t], g['act'][t], g['q_init'], delta=delta, grad_scale=gs)
        np.testing.assert_array_equal(bits(g['act_safe'][t]), bits(r['a_safe']), err_msg=f"t={t}")
        np.testing.assert_array_equal(bits(g['qc'][t]), bits(r['q']), err_msg=f"t={t}")
        np.testing.assert_array_equal(bits(g['lam'][t]), bits(r['lam']), err_msg=f"t={t}")
        branches |= set(np.unique(r['branch']).tolist())
    assert len(branches) >= 2 and (g['lam'] > 0).any() and (g['act_safe'] != g['act']).any()
    obs, rew, cost, done = (x.cpu().numpy() for x in Et.rollout(out['act_safe']))
    np.testing.assert_array_equal(bits(obs[:-1]), bits(g['obs'][1:]))
    np.testing.assert_array_equal(bits(obs[-1]), bits(g['obs_last']))
    for k, w in (('rew', rew), ('cost', cost), ('done', done)):
        np.testing.assert_array_equal(bits(g[k]), bits(w), err_msg=k)
    assert g['done'][:-1].sum() > 0
    E.close()
    Et.close()


# ---------------------------------------------------------------------------------------------------------------------
# 7. q_init and the noise counter
# ---------------------------------------------------------------------------------------------------------------------
def test_q_init_and_noise_counter_across_calls_reset_and_other_paths():
    """store_init=True captures qc[0]; a second call with store_init=False projects with the first call's values and
    returns them, although reset(), step(), rollout_policy and rollout_usl ran in between; its noise continues at
    step0 = T of the first call; rollout_usl's own counter is not advanced by this path"""
    import torch
    from guardx_amd import Engine
    from oracle import policy64
    N, T1, T2, delta, gs = 33, 3, 2, 0.6, 8.0
    E = _engine(_cfg("point", N, seed=5, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = rollout_nets(D, A, 64, 64)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    A64 = policy64.ActorCritic(ac)
    g1 = _np(E.rollout_lpg(p, T1, q_critic=qp, noise_seed=SEED, delta=delta, grad_scale=gs))
    np.testing.assert_array_equal(bits(g1['q_init']), bits(g1['qc'][0]))
    policy64.compare(g1, policy64.rollout(A64, g1, SEED, t0=0), keys=('mu', 'act', 'logp', 'val'), what="call 1")
    E.reset()
    E.step(torch.zeros(N, A, device='cuda'))
    E.reset_done()
    E.rollout_policy(p, 3, noise_seed=SEED)
    E.rollout_usl(p, 2, q_critic=qp, noise_seed=SEED)
    assert E._lpg.steps == T1 and E._usl.steps == 2
    np.testing.assert_array_equal(bits(E._lpg.q_init.cpu().numpy()), bits(g1['q_init']))
    g2 = _np(E.rollout_lpg(p, T2, q_critic=qp, noise_seed=SEED, delta=delta, grad_scale=gs, store_init=False))
    np.testing.assert_array_equal(bits(g2['q_init']), bits(g1['q_init']))
    assert (g2['q_init'] != g2['qc'][0]).any()
    for t in range(T2):
        r = _probe(qp, g2['obs'][t], g2['act'][t], g1['q_init'], delta=delta, grad_scale=gs)
        np.testing.assert_array_equal(bits(g2['act_safe'][t]), bits(r['a_safe']), err_msg=f"t={t}")
        np.testing.assert_array_equal(bits(g2['lam'][t]), bits(r['lam']), err_msg=f"t={t}")
    policy64.compare(g2, policy64.rollout(A64, g2, SEED, t0=T1), keys=('mu', 'act', 'logp', 'val'), what="call 2")
    wrong = policy64.rollout(A64, g2, SEED, t0=0)
    assert (np.abs(g2['act'] - wrong['act']) > wrong['act_b']).any()
    assert E._lpg.steps == T1 + T2 and E._usl.steps == 2
    # the next call with store_init=True replaces the values
    g3 = _np(E.rollout_lpg(p, 1, q_critic=qp, noise_seed=SEED, delta=delta))
    np.testing.assert_array_equal(bits(g3['q_init']), bits(g3['qc'][0]))
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. errors
# ---------------------------------------------------------------------------------------------------------------------
def test_errors():
    import ctypes as C
    import torch
    from guardx_amd import Engine, _lpg_native as n
    from guardx_amd.lpg import projection_probe
    N = 32
    E = _engine(_cfg("point", N))
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = make_ac(D, A, 64, seed=1), make_q(D, A, 64, 2)
    p, qp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_q_critic(qm, device='cuda')
    with pytest.raises(RuntimeError, match="before reset"):
        E.rollout_lpg(p, 3, q_critic=qp)
    E.reset()
    state = E.get_state()
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_lpg(p, 3, q_critic=qp.clone())                    # a copy carries no declaration
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_lpg(p, 3, q_critic=None)
    with pytest.raises(ValueError, match="pack_q_critic"):
        E.rollout_lpg(p, 3, q_critic=Engine.pack_critic(make_ac(D, 1, 64).v, device='cuda'))
    with pytest.raises(ValueError, match=r"q_critic has \d+ floats"):
        E.rollout_lpg(p, 3, q_critic=Engine.pack_q_critic(make_q(D + 1, A, 64, 2), device='cuda'))   # a wrong input width
    with pytest.raises(ValueError, match="T must be >= 1"):
        E.rollout_lpg(p, 0, q_critic=qp)
    with pytest.raises(ValueError, match=r"params has \d+ floats"):
        E.rollout_lpg(p[:-1], 3, q_critic=qp)
    assert E._lpg is None                                           # no call got as far as the path's state
    obs, act, qi = torch.zeros(4, D, device='cuda'), torch.zeros(4, A, device='cuda'), torch.zeros(4, device='cuda')
    with pytest.raises(ValueError, match=r"floats"):
        projection_probe(qp[:-1].clone(), obs, act, qi)
    with pytest.raises(ValueError, match=r"q_init"):
        projection_probe(qp, obs, act, qi[:3])
    lib = n.load()
    out = [torch.zeros(4 * 3, device='cuda') for _ in range(5)]
    work = torch.zeros(int(lib.gxp_probe_work_floats(D, A, 64)), device='cuda')

    def raw(D_, A_, hc, n_=4):
        return lib.gxp_projection_probe(n_, D_, A_, hc, qp.data_ptr(), work.data_ptr(), obs.data_ptr(), act.data_ptr(),
                                        qi.data_ptr(), 0.0, 1.0, 1.0, *(o.data_ptr() for o in out), None)
    assert raw(D, A, 64, n_=-1) == n.GXP_ERR_ARG
    assert raw(D, A, 96) == n.GXP_ERR_UNSUPPORTED                   # a width outside the four
    assert raw(D, 3, 64) == n.GXP_ERR_UNSUPPORTED                   # an odd A
    a = n.GxpStepArgs()
    a.struct_size = C.sizeof(n.GxpStepArgs) - 8
    assert lib.gxp_policy_step(C.byref(a), None) == n.GXP_ERR_ARG and b"struct_size" in lib.gxp_last_error()
    torch.cuda.synchronize()
    assert all((o == 0).all() for o in out)                         # nothing was launched
    assert_state_equal(E.get_state(), state)
    E.close()


# ---------------------------------------------------------------------------------------------------------------------
# 9. the batch helper
# ---------------------------------------------------------------------------------------------------------------------
def test_lpg_rollout_batch_on_device():
    """the batch helper's device path on a real rollout against its host form and the numpy restatement of the buffer
    (tests/test_usl_host.py:USLBufferNP: LPGBufferX is USLBufferX under another name)"""
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import lpg_rollout_batch
    from test_usl_host import usl_batch_np
    N, T = 67, 24
    E = _engine(_cfg("point", N, seed=9, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, qm = rollout_nets(D, A, 64, 64)
    out = E.rollout_lpg(Engine.pack_actor_critic(ac).cuda(), T, q_critic=Engine.pack_q_critic(qm, device='cuda'),
                        noise_seed=SEED, delta=0.5, grad_scale=8.0)
    g = _np(out)
    assert g['done'][:-1].sum() > 0 and (g['act_safe'] != g['act']).any()
    got, want = _np(lpg_rollout_batch(out)), usl_batch_np(g)
    host = _np(lpg_rollout_batch({k: v.cpu() for k, v in out.items()}))
    assert set(got) == set(want) == set(host)
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=tol, err_msg=k)
        np.testing.assert_allclose(got[k], host[k], rtol=tol, atol=tol, err_msg=k)
    E.close()
