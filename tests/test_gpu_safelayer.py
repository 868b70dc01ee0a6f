"""Engine.rollout_safelayer (the safety-layer learner's collection loop on the device, guardx_amd/safelayer.py,
libguardx_safelayer.so): bit equality with rollout_policy in the warm-up branch, the prev_cost channel against the numpy
recurrence, the correction against its numpy float32 transcription bit for bit (in the rollout and on adversarial rows
through gxl_correction_probe), the three networks and the correction against the float64 restatement
(tests/safelayer64.py on oracle/policy64.py), errors, and that the engine is left as rollout_policy leaves it.

Bounds.  g: policy64.mlp's bound for an A-wide head.  act_safe: the per-element bound derived at the top of
tests/safelayer64.py from policy64's constants: the bounds on g and act carried through the two dot products, numer /
denom and a - mult g in the kernel's fixed operation order, one rounding of U per operation, times MARGIN; capped at 2
(both evaluations end in [-1, 1]), so no element is set aside.  A row whose |pred - delta| lies within pred's own bound may
take either branch; such rows may be at most 1 % of all rows (sized on the CPU checker's engine in
tests/test_safelayer_host.py::test_chosen_inputs_exercise_both_branches_and_few_edges)."""
import numpy as np
import pytest

from oracle import policy64
from helpers import assert_state_equal
from test_policy64 import make_ac, report_line, Stub
from test_gpu_statewise import _cfg, _engine, _np, COSTLY, SEED
import safelayer64

pytestmark = pytest.mark.gpu

# (robot, actor width, g_net width): A = 2 and A = 8
CORR_CASES = [("point", 64, 64), ("ant", 256, 128)]
CORR_N, CORR_T, CORR_T2, CORR_CFG_SEED = 203, 12, 5, 7
EDGE_CAP = 0.01


def make_g(D, A, h, seed):
    """a C_Critic-shaped module (.g_net = mlp([D, h, h, A], tanh)) whose outputs are O(1) with either sign"""
    return Stub(g_net=make_ac(D, A, h, seed=seed).pi.mu_net)


def corr_nets(D, A, h, hg):
    return make_ac(D, A, h, seed=h + A, shift=h // 64), make_g(D, A, hg, seed=100 + hg + A)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def prev_cost_recurrence(cost, done, prev0):
    """prev_cost (T, N) and the carried prev_c from the returned cost / done (safelayer.py:546, 576-581)"""
    T, N = cost.shape
    pc, out = prev0.astype(np.float32).copy(), np.empty((T, N), np.float32)
    for t in range(T):
        out[t] = pc
        pc = np.where(done[t] > 0, np.float32(0), cost[t]).astype(np.float32)
    return out, pc


TWIN_KEYS = ('obs', 'act', 'mu', 'logp', 'val', 'rew', 'cost', 'done', 'obs_last', 'val_last', 'logstd')


def _warmup_runs(cfg, h, hg, T, T2, seed, **ekw):
    from guardx_amd import Engine
    E, Et = _engine(cfg, **ekw), _engine(cfg, **ekw)
    Et.set_policy_impl(3)
    E.reset()
    Et.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = make_ac(D, A, h, seed=seed, shift=h // 64), make_g(D, A, hg, seed + 1)
    p, gp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_g_net(gm, device='cuda', act_dim=A)
    runs = []
    for steps in (T, T2):
        g = _np(E.rollout_safelayer(p, steps, g_net=gp, noise_seed=SEED, correct=False))
        w = _np(Et.rollout_policy(p, steps, noise_seed=SEED))
        runs.append((g, w))
    return E, Et, runs


def _assert_warmup_equal(g, w, what):
    for k in TWIN_KEYS:
        np.testing.assert_array_equal(bits(g[k]), bits(w[k]), err_msg=f"{what} {k}")
    np.testing.assert_array_equal(bits(g['act_safe']), bits(g['act']), err_msg=f"{what} act_safe")


# every robot at both width pairs with a ragged last workgroup and many workgroups; the lone row and the exactly full
# workgroup once
WARMUP_CASES = [(robot, h, hg, N) for robot in ("point", "swimmer", "ant") for h, hg in ((64, 64), (256, 128))
                for N in (17, 2000)] + [("point", 64, 64, 1), ("point", 64, 64, 16)]


@pytest.mark.parametrize("robot,h,hg,N", WARMUP_CASES)
def test_warmup_is_bit_equal_to_rollout_policy(robot, h, hg, N):
    """correct=False: the actor, v, the noise and the env give rollout_policy's bits (step-wise form on a twin engine),
    over resets inside the call (num_steps 5 < T) and a second call that continues the noise counter; and the engine is
    left as rollout_policy leaves it"""
    import torch
    T, T2 = (12, 5) if N < 2000 else (8, 3)
    E, Et, runs = _warmup_runs(_cfg(robot, N), h, hg, T, T2, seed=h + N)
    for i, (g, w) in enumerate(runs):
        _assert_warmup_equal(g, w, f"{robot} h={h} N={N} call {i}")
    assert runs[0][0]['done'][:-1].sum() > 0
    np.testing.assert_array_equal(runs[1][0]['obs'][0], runs[0][0]['obs_last'])
    torch.cuda.synchronize()
    assert_state_equal(E.get_state(), Et.get_state())
    for a, b in ((E._obs, Et._obs), (E._reward, Et._reward), (E._done, Et._done), (E._info['cost'], Et._info['cost'])):
        np.testing.assert_array_equal(a.cpu().numpy(), b.cpu().numpy())
    E.close()
    Et.close()


def test_warmup_bit_equal_on_the_thread_per_env_path():
    """env_num = 20000: the step launch does not speculate reset_done, gx_reset_done runs as a launch of its own"""
    wide = dict(placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)       # enough valid layouts for 20000 envs
    E, Et, runs = _warmup_runs(_cfg("point", 20000, seed=4, **wide), 64, 64, 9, 2, seed=9, n_candidates=400000)
    assert E._spec.value == 0                                                   # the launch did not speculate
    for i, (g, w) in enumerate(runs):
        _assert_warmup_equal(g, w, f"N=20000 call {i}")
    assert runs[0][0]['done'][:-1].sum() > 0
    E.close()
    Et.close()


def test_prev_cost_recurrence_across_calls_reset_and_other_paths():
    import torch
    from guardx_amd import Engine
    N = CORR_N
    E = _engine(_cfg("point", N, seed=5, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = corr_nets(D, A, 64, 64)
    p, gp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_g_net(gm, device='cuda')
    pc = np.zeros(N, np.float32)
    seen = dict(after_done=False, positive=False)
    for call, (T, correct) in enumerate(((6, True), (9, True), (4, False))):
        g = _np(E.rollout_safelayer(p, T, g_net=gp, noise_seed=SEED, correct=correct))
        want, pc = prev_cost_recurrence(g['cost'], g['done'], pc)
        np.testing.assert_array_equal(bits(g['prev_cost']), bits(want), err_msg=f"call {call}")
        after = g['done'][:-1] > 0
        seen['after_done'] |= bool(after.any())
        assert (g['prev_cost'][1:][after] == 0).all()                 # zero on the step after a done
        seen['positive'] |= bool((g['prev_cost'] > 0).any())
        if call == 0:
            # an intervening step() + reset_done() and a rollout_policy neither read nor write prev_c
            act = torch.zeros(N, A, device='cuda')
            E.step(act)
            E.reset_done()
            E.rollout_policy(p, 3, noise_seed=SEED)
    assert seen['after_done'] and seen['positive']
    assert pc.any()
    o = E.reset()
    g = _np(E.rollout_safelayer(p, 4, g_net=gp, noise_seed=SEED))
    np.testing.assert_array_equal(g['obs'][0], o.cpu().numpy())
    np.testing.assert_array_equal(bits(g['prev_cost'][0]), bits(np.zeros(N, np.float32)))   # zero after reset()
    want, _ = prev_cost_recurrence(g['cost'], g['done'], np.zeros(N, np.float32))
    np.testing.assert_array_equal(bits(g['prev_cost']), bits(want))
    E.close()


@pytest.mark.parametrize("delta", [0.0, 0.05])
@pytest.mark.parametrize("robot,h,hg", CORR_CASES)
def test_correction_is_the_float32_transcription_bit_for_bit(robot, h, hg, delta):
    """correction32 on the kernel's own g, act, prev_cost gives act_safe's bits on every row, and both branches are
    exercised: corrected and uncorrected rows are each at least a tenth of all rows"""
    from guardx_amd import Engine
    E = _engine(_cfg(robot, CORR_N, seed=CORR_CFG_SEED, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = corr_nets(D, A, h, hg)
    p, gp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_g_net(gm, device='cuda')
    rows = corrected = 0
    for steps in (CORR_T, CORR_T2):
        g = _np(E.rollout_safelayer(p, steps, g_net=gp, noise_seed=SEED, delta=delta))
        want, pred = safelayer64.correction32(g['g'], g['act'], g['prev_cost'], delta)
        np.testing.assert_array_equal(bits(g['act_safe']), bits(want))
        unc = pred <= np.float32(delta)
        np.testing.assert_array_equal(bits(g['act_safe'][unc]), bits(g['act'][unc]))     # unclamped, untouched
        assert (np.abs(g['act_safe'][~unc]) <= 1).all()
        rows += pred.size
        corrected += int((~unc).sum())
        assert (g['prev_cost'] > 0).any() and g['done'][:-1].sum() > 0
    share = corrected / rows
    print(f"safelayer correction {robot} A={A} delta={delta}: {rows} rows, corrected {share:.3f}")
    assert 0.1 <= share <= 0.9, share
    E.close()


def test_correction_probe_on_adversarial_rows():
    """gxl_correction_probe against correction32, bit for bit: pred one ulp either side of delta, g = 0, |a| > 1 on an
    uncorrected row, a non-zero delta, random rows of every width"""
    import torch
    from guardx_amd.safelayer import correction_probe
    f = np.float32

    def run(g, a, pc, delta):
        got = correction_probe(torch.from_numpy(g).cuda(), torch.from_numpy(a).cuda(), torch.from_numpy(pc).cuda(),
                               delta).cpu().numpy()
        want, pred = safelayer64.correction32(g, a, pc, delta)
        np.testing.assert_array_equal(bits(got), bits(want))
        return got, pred

    for delta in (f(0.0), f(0.25), f(-0.1)):
        lo, hi = np.nextafter(delta, f(-10)), np.nextafter(delta, f(10))
        # g = (1, 0), a = (x, 0.5), prev_c = 0: pred = x exactly
        x = np.array([lo, delta, hi], f)
        g = np.tile(np.array([1, 0], f), (3, 1))
        a = np.stack([x, np.full(3, 0.5, f)], 1)
        got, pred = run(g, a, np.zeros(3, f), delta)
        np.testing.assert_array_equal(bits(pred), bits(x))
        np.testing.assert_array_equal(bits(got[:2]), bits(a[:2]))             # pred <= delta: untouched
        assert got[2, 0] != a[2, 0] or hi - delta == 0                          # one ulp above: corrected
        # g = 0: pred = prev_c; where prev_c > delta the result is clamp(a), elsewhere a itself, |a| > 1 included
        a = np.array([[1.5, -2.0], [0.3, -0.4], [1.5, -2.0], [-3.0, 0.2]], f)
        pc = np.array([1.0, 1.0, -1.0, delta], f)
        got, _ = run(np.zeros((4, 2), f), a, pc, delta)
        np.testing.assert_array_equal(got[0], np.array([1.0, -1.0], f))
        np.testing.assert_array_equal(got[1], a[1])
        np.testing.assert_array_equal(got[2], a[2])                             # uncorrected: stays unclamped
        np.testing.assert_array_equal(got[3], a[3])
    rng = np.random.default_rng(2)
    for A in (1, 2, 3, 8, 10, 16):
        n = 20000
        g = rng.normal(size=(n, A)).astype(f) * rng.choice([1e-4, 1.0, 30.0], size=(n, 1)).astype(f)
        a = (rng.normal(size=(n, A)) * 1.5).astype(f)
        pc = (rng.random(n) * (rng.random(n) < 0.5)).astype(f)
        _, pred = run(g, a, pc, f(0.05))
        assert 0.2 < (pred > f(0.05)).mean() < 0.95


@pytest.mark.parametrize("robot,h,hg", CORR_CASES)
def test_networks_and_correction_match_the_float64_restatement(robot, h, hg):
    """teacher-forced on the recorded obs and prev_cost: mu, act, logp, val, val_last and g within policy64's bounds,
    act_safe within the bound of tests/safelayer64.py; rows on the branch's edge (either value accepted) at most 1 %.
    The report line prints, per output, the largest err / bound and the median bound, and the share of edge rows."""
    from guardx_amd import Engine
    E = _engine(_cfg(robot, CORR_N, seed=CORR_CFG_SEED, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = corr_nets(D, A, h, hg)
    p, gp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_g_net(gm, device='cuda')
    t0, edges, rows = 0, 0, 0
    for steps in (CORR_T, CORR_T2):
        g = _np(E.rollout_safelayer(p, steps, g_net=gp, noise_seed=SEED))
        what = f"safelayer {robot} h={h} g={hg} t0={t0}"
        want = safelayer64.rollout(ac, gm, g, SEED, t0=t0)
        res = policy64.compare(g, want, keys=policy64.OUTPUTS + ('g',), what=what)
        worst, med, edge = safelayer64.compare_act_safe(g, want, what)
        res['act_safe'] = (worst, med)
        report_line(what + f" edge rows {edge:.4f}", res)
        c = want['corr']
        edges += int(c['edge'].sum())
        rows += c['edge'].size
        assert c['corrected'].any() and (~c['corrected']).any()
        assert np.isfinite(c['a_safe_b']).all()
        t0 += steps
    assert edges <= EDGE_CAP * rows, (edges, rows)
    E.close()


def test_errors():
    import torch
    from guardx_amd import Engine
    N = 32
    E = _engine(_cfg("point", N))
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = corr_nets(D, A, 64, 64)
    p, gp = Engine.pack_actor_critic(ac).cuda(), Engine.pack_g_net(gm, device='cuda')
    with pytest.raises(RuntimeError, match="before reset"):
        E.rollout_safelayer(p, 3, g_net=gp)
    E.reset()
    state = E.get_state()
    with pytest.raises(ValueError, match=r"g_net has \d+ floats"):
        E.rollout_safelayer(p, 3, g_net=Engine.pack_g_net(make_g(D + 1, A, 64, 1), device='cuda'))    # another input width
    with pytest.raises(ValueError, match=r"g_net has \d+ floats"):
        E.rollout_safelayer(p, 3, g_net=Engine.pack_g_net(make_g(D, 4, 64, 1), device='cuda'))        # another action width
    with pytest.raises(ValueError, match="pack_g_net"):
        E.rollout_safelayer(p, 3, g_net=gp.clone())                   # a copy carries no declaration
    with pytest.raises(ValueError, match="pack_g_net"):
        E.rollout_safelayer(p, 3, g_net=Engine.pack_critic(make_ac(D, 1, 64).v, device='cuda'))
    with pytest.raises(ValueError, match="pack_g_net"):
        E.rollout_safelayer(p, 3, g_net=None)
    with pytest.raises(ValueError, match="T must be >= 1"):
        E.rollout_safelayer(p, 0, g_net=gp)
    with pytest.raises(ValueError, match=r"params has \d+ floats"):
        E.rollout_safelayer(p[:-1], 3, g_net=gp)
    torch.cuda.synchronize()
    assert_state_equal(E.get_state(), state)                          # nothing ran
    E.close()


def test_safelayer_rollout_batch_on_device():
    """the batch helper's device path on a real rollout against the numpy restatement of SafeLayerBufferX"""
    from guardx_amd import Engine
    from guardx_amd.rollout_buffer import safelayer_rollout_batch
    from test_safelayer_host import safelayer_batch_np
    N, T = 67, 24
    E = _engine(_cfg("point", N, seed=9, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac, gm = corr_nets(D, A, 64, 64)
    out = E.rollout_safelayer(Engine.pack_actor_critic(ac).cuda(), T, g_net=Engine.pack_g_net(gm, device='cuda'),
                              noise_seed=SEED)
    g = _np(out)
    assert g['done'][:-1].sum() > 0 and (g['act_safe'] != g['act']).any()
    got, want = _np(safelayer_rollout_batch(out)), safelayer_batch_np(g)
    assert set(got) == set(want)
    for k in want:
        tol = 2e-4 if k == 'adv' else 2e-5
        np.testing.assert_allclose(got[k], want[k], rtol=tol, atol=tol, err_msg=k)
    E.close()
