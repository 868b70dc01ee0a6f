"""The C checker's dynamics on the engine path (OracleEngine.set_state -> step -> get_state) against the float64
robot models of tests/dyn64.py, on the state sets that tests/test_gpu_dyn64.py runs through the HIP kernels:
random states of helpers.random_state, config variants, a three-step chain, and directed states.  Shows that
inputs and bounds hold for the checker alone, and widens its float64 coverage from the single-state probes
(120-150 states, |th| <= 1, velocities N(0, 2)) to the engine path and the parity tests' distribution.

Worst error of the C checker per env, max|d| / (1 + max|ref|), one step, as these tests print it (pose0 stays
below 3e-7 absolute at one physics step; "of bound": the largest fraction of any bound of dyn64.py reached):
    robot     random N = 192                   directed, 16 states     active rows of the random set
              qpos      qvel      of bound     qpos      qvel          limit   contact
    point     5.2e-08   9.7e-07   0.80         3.2e-08   6.0e-07
    swimmer   4.7e-08   4.0e-07   0.15         3.0e-08   3.9e-07
    ant       2.4e-05   1.05e-04  0.12         1.4e-06   3.0e-06       706     792
    walker    5.1e-06   1.66e-04  0.12         5.1e-07   7.1e-06       421     172
Every directed state passes for the checker alone: none is excluded or expected to fail.
"""
import functools

import numpy as np
import pytest

import dyn64
from helpers import task_config, random_state, SWIMMER, ANT, WALKER, ANT_SIGMA, WALKER_LO, WALKER_HI
from oracle import ref64

f32 = np.float32
ROBOTS = ["point", "swimmer", "ant", "walker"]
EXTRA = {"point": {}, "swimmer": SWIMMER, "ant": ANT, "walker": WALKER}
ADIM = {"point": 2, "swimmer": 2, "ant": 8, "walker": 10}
N_RANDOM = 192
N_VARIANT = 32
VARIANTS = {"k2": dict(physics_steps_per_control_step=2), "vel": dict(observe_vel=True),
            "rot": dict(robot_rot=0.9)}


def config(robot, N, **over):
    """num_steps above any step count of the state sets: no timeout"""
    return task_config(N, seed=5, num_steps=1000, **EXTRA[robot], **over)


def _pose_of(robot, qpos):
    return ref64.robot_pose(ref64.Config(config(robot, 1)), qpos).astype(f32)


def _far(s, robot):
    """the dynamics read no object and no earlier position: goal and hazards go out of reach, the step counters
    to zero and the last positions onto the robot (pose0 keeps its heading, which the Point's ctrl reads), so
    that no env is done and a rollout row carries the step's own qpos / qvel for every env"""
    s['objs'][:] = f32(50.0)
    s['steps'][:] = 0
    s['hist'] = 2
    s['pose0'][:, :2] = _pose_of(robot, s['qpos'])[:, :2]
    s['pose1'] = s['pose0'][:, :2].copy()
    return s


def settle(cfg, s):
    """a copy of s whose last positions are the robot's under `cfg` (robot_rot turns the world pose), see _far"""
    s = dict(s, pose0=s['pose0'].copy())
    s['pose0'][:, :2] = ref64.robot_pose(ref64.Config(cfg), s['qpos'])[:, :2].astype(f32)
    s['pose1'] = s['pose0'][:, :2].copy()
    return s


PER_ENV = ('qpos', 'qvel', 'pose0', 'pose1', 'objs', 'done0', 'done1', 'steps')     # the rest (key, hist) is per engine


def take(s, idx):
    """rows idx of a state dict"""
    return {k: (v[idx] if k in PER_ENV else v) for k, v in s.items()}


@functools.lru_cache(maxsize=None)
def random_set(robot):
    """(state, actions) of N_RANDOM envs: random_state as the parity tests draw it (qvel up to +-6, legs 15 %
    beyond their ranges), actions beyond the ctrl range (clipped for the force only); a third of the Point's envs
    slow and gently driven so that its velocity servo is not saturated.  Batch sizes and variants take prefixes."""
    rng = np.random.default_rng(0)
    s = _far(random_state(N_RANDOM, 8, rng, done_frac=0.0, robot=robot), robot)
    act = rng.uniform(-1.4, 1.4, (N_RANDOM, ADIM[robot])).astype(f32)
    if robot == 'point':
        s['qvel'][::3] *= f32(0.03)
        act[::3] *= f32(0.03)
    return s, act


def _directed_qv(robot):
    """[(name, qpos, qvel, action or None)]; None: a drawn action beyond the ctrl range"""
    out = []
    nq = ref64.NQ[robot]
    Z = lambda: np.zeros(nq)

    def add(name, q, v=None, act=None):
        out.append((name, np.asarray(q, float), Z() if v is None else np.asarray(v, float), act))
    zero = np.zeros(ADIM[robot])
    if robot == 'ant':
        S = ANT_SIGMA.astype(float)
        hip, ank = [3, 5, 7, 9], [4, 6, 8, 10]

        def pose(x=0.7, th=0.0, y=-0.4, hips=0.0, ankles=0.0):
            q = Z(); q[0], q[1], q[2] = x, th, y
            q[hip] = hips; q[ank] = S * ankles
            return q

        def vel(base=(0, 0, 0), hips=0.0, ankles=0.0):
            v = Z(); v[:3] = base; v[hip] = hips; v[ank] = S * ankles
            return v
        alt = np.array([1.0, -1.0, 1.0, -1.0])
        add("rest", pose(), act=zero)                           # ankles 30 deg outside their range
        add("rest th=+1", pose(th=1.0), act=zero)
        add("rest th=-1", pose(th=-1.0), act=zero)
        add("feet pressed 1.15 lateral", pose(ankles=1.15), vel(base=(1, 0, -1)))
        add("feet pressed 1.3 lateral", pose(th=0.5, ankles=1.3), vel(base=(-1, 0, 1)))
        add("feet pressed 1.5 lateral th=+1", pose(th=1.0, ankles=1.5), vel(base=(1, 0, 1)))
        add("feet pressed 1.2 v=0", pose(ankles=1.2), act=zero)
        add("all beyond high", pose(hips=0.6, ankles=1.3))
        add("all beyond low outward", pose(hips=-0.6, ankles=0.4), vel(hips=-3.0, ankles=-3.0))
        add("beyond alternating", pose(hips=0.6 * alt, ankles=np.where(alt > 0, 0.4, 1.3)))
        add("beyond alternating other", pose(hips=-0.6 * alt, ankles=np.where(alt > 0, 1.3, 0.4)))
        add("|v|=6 all +", pose(ankles=0.8), np.full(nq, 6.0))
        add("|v|=6 alternating th=-1", pose(th=-1.0, ankles=0.8), 6.0 * np.where(np.arange(nq) % 2, -1.0, 1.0))
        add("|v|=6 feet pressed", pose(ankles=1.25), 6.0 * np.where(np.arange(nq) % 2, 1.0, -1.0))
        add("th=-1 feet pressed 1.4 lateral", pose(th=-1.0, ankles=1.4), vel(base=(1, 2, -1), hips=2.0))
        add("ankles at the range edge", pose(ankles=float(f32(np.pi / 6))), act=zero)
    elif robot == 'walker':
        lo, hi = WALKER_LO.astype(float), WALKER_HI.astype(float)
        w = hi - lo
        alt = np.where(np.arange(10) % 2, -1.0, 1.0)

        def pose(x=0.7, th=0.0, y=-0.4, legs=0.0, foot=None):
            q = Z(); q[0], q[1], q[2] = x, th, y
            q[3:] = legs
            if foot is not None:
                q[7] = q[12] = foot
            return q

        def vel(base=(0, 0, 0), legs=0.0):
            v = Z(); v[:3] = base; v[3:] = legs
            return v
        add("rest", pose(), act=zero)
        add("rest th=+1", pose(th=1.0), act=zero)
        add("rest th=-1", pose(th=-1.0), act=zero)
        add("feet down v=0", pose(foot=-0.6), act=zero)          # as test_foot_contact_rows
        add("feet down lateral", pose(foot=-0.6), vel(base=(1, 0, -1)))
        add("feet down th=+1 moving", pose(th=1.0, foot=-0.75), vel(base=(-1, 1, 1), legs=2.0 * alt))
        add("all beyond high", pose(legs=hi + 0.1 * w))
        add("all beyond low outward", pose(legs=lo - 0.1 * w), vel(legs=-3.0))
        add("beyond alternating", pose(legs=np.where(alt > 0, hi + 0.1 * w, lo - 0.1 * w)))
        add("beyond alternating other", pose(legs=np.where(alt > 0, lo - 0.1 * w, hi + 0.1 * w)))
        add("|v|=6 all + mid-range", pose(legs=0.5 * (lo + hi)), np.full(nq, 6.0))
        add("|v|=6 alternating th=-1 feet down", pose(th=-1.0, foot=-0.4), 6.0 * np.where(np.arange(nq) % 2, -1.0, 1.0))
        add("|v|=6 beyond alternating", pose(legs=np.where(alt > 0, hi + 0.05 * w, lo - 0.05 * w)),
            6.0 * np.where(np.arange(nq) % 2, 1.0, -1.0))
        add("th=+1 mid-range", pose(th=1.0, legs=lo + 0.3 * w), vel(base=(0.5, -2, 0.5), legs=3.0 * alt))
        add("th=-1 feet down hips beyond", pose(th=-1.0, legs=np.tile(np.r_[hi[:3] + 0.1 * w[:3], 0, 0], 2), foot=-0.6))
        add("feet beyond their limit v=0", pose(foot=-0.9), act=zero)
    elif robot == 'swimmer':
        L = 1.7453293

        def qv(j1, j2, w1=0.0, w2=0.0, th=0.3, base=(0.0, 0.0, 0.0)):
            return [0.5, -0.3, th, j1, j2], [base[0], base[1], base[2], w1, w2]
        add("rest", Z(), act=zero)
        add("both beyond ++ outward", *qv(L + 0.05, L + 0.05, 5, 5))
        add("both beyond -- outward", *qv(-L - 0.05, -L - 0.05, -5, -5))
        add("both beyond +- outward", *qv(L + 0.05, -L - 0.05, 5, -5))
        add("both beyond -+ outward", *qv(-L - 0.05, L + 0.05, -5, 5))
        add("both beyond by 0.3 outward 8", *qv(L + 0.3, -L - 0.3, 8, -8, base=(1, -1, 8)))
        add("both beyond inward", *qv(L + 0.1, L + 0.1, -5, -5))
        add("both just beyond v=0", *qv(L + 1e-6, -L - 1e-6), act=zero)
        add("|v|=6 all +", *qv(0.5, -0.5, 6, 6, base=(6, 6, 6)))
        add("|v|=6 alternating", *qv(-1.0, 1.0, -6, 6, base=(6, -6, 6)))
        add("|v|=6 both beyond", *qv(L + 0.2, L + 0.2, 6, 6, base=(-6, 6, -6)))
        add("th=+1", *qv(1.2, -0.7, 2, -3, th=1.0, base=(0.5, 0.5, 2)))
        add("th=-1", *qv(-1.2, 0.7, -2, 3, th=-1.0, base=(-0.5, 0.5, -2)))
        add("th=8 spinning", *qv(0.3, 1.5, 4, 4, th=8.0, base=(1, 1, 8)))
        add("both beyond v=0", *qv(L + 0.2, -L - 0.2), act=zero)
        add("one beyond saturated ctrl", *qv(L + 0.1, 0.2), act=np.array([1.4, -1.4]))
    else:
        add("rest", Z(), act=zero)
        add("rest saturated", Z(), act=np.array([1.0, 1.0]))            # |ctrl| > .05: the force limit
        add("rest not saturated", Z(), act=np.array([0.04, 0.04]))
        add("servo off", [0.5, -0.5, 0.3], [0.1, 0, 0], act=np.array([0.03, 0.0]))
        add("servo brakes not saturated", [0.5, -0.5, 0.3], [0.1, -0.1, 0.1], act=zero)
        add("fast saturated", [2.0, -2.0, 3.0], [3, -3, 30], act=np.array([1.4, -1.4]))
        add("|v|=6 all +", [1.0, 1.0, 0.5], [6, 6, 6])
        add("|v|=6 alternating", [-1.0, 1.0, -0.5], [6, -6, 6])
        add("th=+1", [0.2, 0.3, 1.0], [1, -1, 3])
        add("th=-1", [0.2, 0.3, -1.0], [-1, 1, -3])
        add("th=+40 spinning", [2.5, -2.5, 40.0], [1, 1, 30])
        add("th=-40 spinning", [-2.5, 2.5, -40.0], [-1, -1, -30])
        add("stale heading a quarter turn off", [0.0, 0.0, 0.0], [0.02, 0.01, 0.05], act=np.array([0.03, 0.02]))
        add("slow gentle", [1.0, -1.0, 2.0], [0.05, -0.03, 0.4], act=np.array([0.02, -0.03]))
        add("at the force limit", Z(), act=np.array([0.05, -0.05]))
        add("ctrl far beyond its range", [0.3, 0.3, 0.3], [0.5, 0.5, 5], act=np.array([7.0, -9.0]))
    return out


@functools.lru_cache(maxsize=None)
def directed_set(robot):
    """(state, actions, names) of the directed states of _directed_qv"""
    rows = _directed_qv(robot)
    n = len(rows)
    rng = np.random.default_rng(1)
    s = random_state(n, 8, rng, done_frac=0.0, robot=robot)
    s['qpos'] = np.array([r[1] for r in rows], f32)
    s['qvel'] = np.array([r[2] for r in rows], f32)
    s['pose0'] = _pose_of(robot, s['qpos'])
    s = _far(s, robot)
    act = rng.uniform(-1.4, 1.4, (n, ADIM[robot])).astype(f32)
    names = []
    for i, (name, _, _, a) in enumerate(rows):
        names.append(name)
        if a is not None:
            act[i] = a
        if name.startswith("stale heading"):
            s['pose0'][i, 2:] = (0.0, 1.0)
    return s, act, names


def checker_step(oracle, cfg, s, act):
    """the C checker's post-step state from s under act; no env of these sets is done"""
    E = oracle.OracleEngine(cfg, n_candidates=3000)
    E.reset(check=False)
    E.set_state(s)
    _, _, done, _ = E.step(act)
    assert not done.any()
    return E.get_state()


# ---- random states ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_random_states(oracle, robot):
    s, act = random_set(robot)
    cfg = config(robot, N_RANDOM)
    want = dyn64.expect(cfg, s, act)
    st = checker_step(oracle, cfg, s, act)
    worst = dyn64.check(cfg, want, st['qpos'], st['qvel'], st['pose0'], what="random")
    rows = dyn64.rows_count(robot, s) if robot in dyn64.TREE_BOUND else None
    print(f"checker {robot} random: {worst}; (limit, contact) rows {rows}")
    if rows is not None:
        assert rows[0] > 100 and rows[1] > 100, rows          # the set exercises both kinds of rows


# ---- variants -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_variants(oracle, robot, variant):
    s, act = random_set(robot)
    s, act = take(s, slice(0, N_VARIANT)), act[:N_VARIANT]
    cfg = config(robot, N_VARIANT, **VARIANTS[variant])
    s = settle(cfg, s)
    want = dyn64.expect(cfg, s, act)
    st = checker_step(oracle, cfg, s, act)
    worst = dyn64.check(cfg, want, st['qpos'], st['qvel'], st['pose0'], what=variant)
    print(f"checker {robot} {variant}: {worst}")
    if variant != "k2":
        # neither the observation's contents nor the root body's turn reaches the joint dynamics
        base = checker_step(oracle, config(robot, N_VARIANT), settle(config(robot, N_VARIANT), s), act)
        np.testing.assert_array_equal(st['qpos'], base['qpos'])
        np.testing.assert_array_equal(st['qvel'], base['qvel'])
        assert (variant == "rot") == (not np.allclose(st['pose0'], base['pose0'], atol=1e-3))


def test_point_two_substeps(oracle):
    """the measurement behind dyn64.POINT_HINGE_VEL_BOUND_K2: the checker at two physics steps per control step on
    the Point's random set, its directed states and three chained steps of the random set.  Worst hinge velocity
    error 9.46e-6 max(1, max|ref|) (random set, first step), half the bound; every other component stays within
    the single-step 2e-6 (worst 1.4e-7)"""
    worst, hinge = dyn64.Worst(), 0.0
    for s, act in (random_set("point"), directed_set("point")[:2]):
        cfg = config("point", len(act), **VARIANTS["k2"])
        E = oracle.OracleEngine(cfg, n_candidates=3000)
        E.reset(check=False)
        E.set_state(settle(cfg, s))
        for t in range(3):
            pre = E.get_state()
            a = np.roll(act, t, axis=0)
            _, _, done, _ = E.step(a)
            assert not done.any()
            st = E.get_state()
            want = dyn64.expect(cfg, pre, a)
            dyn64.check(cfg, want, st['qpos'], st['qvel'], st['pose0'], worst=worst, what=f"k2 t={t}")
            scale = np.maximum(1.0, np.abs(want['qvel2']).max(axis=1))
            hinge = max(hinge, (np.abs(st['qvel'][:, 2] - want['qvel2'][:, 2]) / scale).max())
    print(f"checker point k2: {worst}; hinge velocity {hinge:.3g} max(1, max|ref|)")


# ---- three steps, each from the checker's own state ---------------------------------------------------------
@pytest.mark.parametrize("robot", ROBOTS)
def test_chain_of_three(oracle, robot):
    """the states a rollout passes through after the first step (large accelerations out of the limits and the
    floor) stay inside the bounds too; each step is compared from the fp32 state before it"""
    N = N_VARIANT
    s, act = random_set(robot)
    s = take(s, slice(0, N))
    cfg = config(robot, N)
    E = oracle.OracleEngine(cfg, n_candidates=3000)
    E.reset(check=False)
    E.set_state(s)
    worst = dyn64.Worst()
    for t in range(3):
        pre = E.get_state()
        a = act[t * N:(t + 1) * N]
        _, _, done, _ = E.step(a)
        assert not done.any()
        st = E.get_state()
        dyn64.check(cfg, dyn64.expect(cfg, pre, a), st['qpos'], st['qvel'], st['pose0'], worst=worst, what=f"t={t}")
    print(f"checker {robot} chain: {worst}")


# ---- directed states ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _directed_checker(robot):
    s, act, names = directed_set(robot)
    cfg = config(robot, len(names))
    return dyn64.expect(cfg, s, act), checker_step(_directed_checker.oracle, cfg, s, act)


def _directed_params():
    return [pytest.param(r, i, id=f"{r}-{i}") for r in ROBOTS for i in range(16)]


@pytest.mark.parametrize("robot,i", _directed_params())
def test_directed_state(oracle, robot, i):
    s, act, names = directed_set(robot)
    assert len(names) == 16
    _directed_checker.oracle = oracle
    want, st = _directed_checker(robot)
    worst = dyn64.check(config(robot, 16), want, st['qpos'], st['qvel'], st['pose0'], rows=[i], what=names[i])
    print(f"checker {robot} directed {i} ({names[i]}): {worst}")


def test_directed_states_reach_what_they_name():
    """the float64 models see the rows the names promise"""
    for robot, need in (("ant", {"rest": (4, 0), "feet pressed 1.15 lateral": (0, 16), "feet pressed 1.2 v=0": (0, 16),
                                 "all beyond high": (8, 16), "all beyond low outward": (8, 0)}),
                        ("walker", {"rest": (0, 8), "feet down v=0": (0, 8), "all beyond high": (10, 0),
                                    "all beyond low outward": (10, None), "feet beyond their limit v=0": (2, 8)})):
        s, act, names = directed_set(robot)
        for name, (nlim, ncon) in need.items():
            i = names.index(name)
            got = dyn64.rows_count(robot, take(s, slice(i, i + 1)))
            assert got[0] == nlim and ncon in (None, got[1]), (robot, name, got)
    s, act, names = directed_set("point")
    u = act[:, 0].astype(float) * s['pose0'][:, 2] - 0.3 * s['qvel'][:, 0]
    assert abs(u[names.index("fast saturated")]) > 0.05 > abs(u[names.index("slow gentle")])
