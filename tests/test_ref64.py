"""oracle/ref64.py, the float64 restatement of the output layer: hand-worked cases, and the C checker against it
for every robot over the variant configs and the capacity shapes (multi-step, with reset_done)."""
import ast
import math
import os

import numpy as np
import pytest

from helpers import task_config, SWIMMER, ANT, WALKER
from oracle import ref64

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTRA = {"point": {}, "swimmer": SWIMMER, "ant": ANT, "walker": WALKER}
ADIM = {"point": 2, "swimmer": 2, "ant": 8, "walker": 10}

# the variant list of test_gpu_parity.test_variant_configs
VARIANTS = [
    dict(hazards_num=3, lidar_num_bins=8),
    dict(hazards_num=12, lidar_num_bins=24, lidar_alias=False, hazards_keepout=0.25),
    dict(observe_vel=True, observe_acc=True),
    dict(observe_qpos=False, observe_ctrl=False, observe_goal_lidar=False),
    dict(lidar_max_dist=3.0, physics_steps_per_control_step=2, lidar_exp_gain=0.5),
    dict(hazards_num=20, goal_size=0.3, hazards_size=0.2, reward_distance=2.0,
         hazards_keepout=0.18, placements_extents=[-3, -3, 3, 3]),
    dict(robot_rot=0.7),
    dict(robot_rot=-2.4, observe_vel=True, hazards_num=5, goal_size=1.5),
]

# capacity shapes: bin counts 3..64 (3: bin +- 1 wrap onto each other; 17, 33, 63: not a multiple of 4), object
# counts up to 65 (goal + 64 hazards, or goal + 40 hazards + 24 observed pillars), and the widest row of a robot
_WIDE = dict(placements_extents=[-6, -6, 6, 6], hazards_size=0.3, hazards_keepout=0.1)
CAPACITY = [
    dict(lidar_num_bins=3, hazards_num=4, observe_vel=True, observe_acc=True),
    dict(lidar_num_bins=17, hazards_num=15, lidar_exp_gain=2.5, **_WIDE),
    dict(lidar_num_bins=33, hazards_num=16, lidar_alias=False, **_WIDE),
    dict(lidar_num_bins=63, hazards_num=31, lidar_max_dist=2.0, **_WIDE),
    dict(lidar_num_bins=64, hazards_num=32, **_WIDE),
    dict(lidar_num_bins=64, hazards_num=64, observe_vel=True, observe_acc=True, **_WIDE),
    dict(lidar_num_bins=64, hazards_num=40, pillars_num=24, observe_pillars=True, pillars_size=0.1,
         pillars_keepout=0.1, observe_vel=True, observe_acc=True, **_WIDE),
]


def run_checker_vs_ref64(oracle, robot, v, N=96, T=40, seed=9, n_candidates=30000):
    """T steps of the C checker, reset_done every 7th, each compared with ref64; returns the exclusion tally"""
    cfg = task_config(N, seed=seed, num_steps=25, **v, **EXTRA[robot])
    O = oracle.OracleEngine(cfg, n_candidates=n_candidates)
    O.reset()
    C = ref64.Config(cfg)
    assert C.D == O.D
    rng = np.random.default_rng(seed)
    tally = ref64.Tally()
    for t in range(T):
        pre = O.get_state()
        act = rng.uniform(-1, 1, (N, ADIM[robot])).astype(np.float32)
        o, r, d, info = O.step(act)
        post = O.get_state()
        want = ref64.step(C, pre, act, post['qpos'], post['qvel'])
        ref64.check(C, dict(obs=o, reward=r, done=d, cost=info['cost'], steps=post['steps']), want, tally,
                    what=f"{robot} {v} t={t}")
        if t % 7 == 6:
            ro = O.reset_done()
            check_reset_done(C, o, d, ro, O.get_state(), tally)
    assert tally.frac() < 0.01, tally
    return tally


def check_reset_done(C, obs_step, done, obs_rd, post, tally, what="reset_done"):
    obs_step, obs_rd = np.asarray(obs_step), np.asarray(obs_rd)
    keep = np.asarray(done) == 0
    np.testing.assert_array_equal(obs_rd[keep], obs_step[keep])
    qs = obs_rd[:, C.slices['qpos']] if 'qpos' in C.slices else None
    qv = obs_rd[:, C.slices['qvel']] if 'qvel' in C.slices else None
    want, aux, rows = ref64.reset_obs(C, obs_step, done, post, qs, qv)
    rows = np.nonzero(rows)[0]
    ref64.check_obs(C, obs_rd, want, aux, tally, rows, what=what)
    tally.entries += int((~keep).sum() - rows.size) * C.D
    tally.excluded += int((~keep).sum() - rows.size) * C.D


# ---- hand-worked cases --------------------------------------------------------------------------------------
def _cfg(**kw):
    return ref64.Config(dict(kw))


def _pose(x=0.0, y=0.0, th=0.0):
    return np.array([[x, y, math.cos(th), math.sin(th)]])


def _read(C, pose, pts):
    pts = np.asarray(pts, float).reshape(1, -1, 2)
    pos, s, _, _ = ref64.lidar_parts(C, pose, pts, (np.zeros(1), np.zeros(1)))
    return ref64.lidar(C, pos, s)[0], pos[0]


def test_lidar_dead_ahead():
    """an object on the robot's x axis at distance 2: angle 0, bin 0, alias 0 -> bin 0 and bin B-1 read
    exp(-2), bin 1 reads 0 (engine.py:843-869)"""
    C = _cfg(lidar_num_bins=16)
    obs, pos = _read(C, _pose(1.0, -1.0, 0.0), [(3.0, -1.0)])
    want = np.zeros(16)
    want[0] = want[15] = math.exp(-2.0)
    np.testing.assert_allclose(obs, want, rtol=0, atol=1e-15)
    assert pos[0] == 0.0
    # the same object seen by a robot turned by +90 degrees is at -90 degrees = 270: bin 12, alias 0
    obs, pos = _read(C, _pose(1.0, -1.0, math.pi / 2), [(3.0, -1.0)])
    assert abs(pos[0] - 12.0) < 1e-12
    assert abs(obs[11] - math.exp(-2.0)) < 1e-12 and abs(obs[12] - math.exp(-2.0)) < 1e-12


def test_lidar_object_on_robot():
    """dist 0: atan2(0, 0) = 0, reading exp(0) = 1 in bin 0 and (alias 0) in bin B-1"""
    C = _cfg(lidar_num_bins=8)
    obs, _ = _read(C, _pose(0.5, 0.5, 1.0), [(0.5, 0.5)])
    np.testing.assert_array_equal(obs, [1, 0, 0, 0, 0, 0, 0, 1])


def test_lidar_three_bins_wrap():
    """3 bins: bin +- 1 are the two other bins.  An object at 300 deg: bin 2, alias (300-240)/120 = .5 ->
    bin 0 (= bin + 1 mod 3) and bin 1 (= bin - 1) both read .5 s"""
    C = _cfg(lidar_num_bins=3)
    a = math.radians(300)
    obs, pos = _read(C, _pose(), [(math.cos(a), math.sin(a))])
    s = math.exp(-1.0)
    np.testing.assert_allclose(obs, [0.5 * s, 0.5 * s, s], rtol=0, atol=1e-12)
    # no alias: only bin 2
    obs, _ = _read(_cfg(lidar_num_bins=3, lidar_alias=False), _pose(), [(math.cos(a), math.sin(a))])
    np.testing.assert_allclose(obs, [0, 0, s], rtol=0, atol=1e-12)


def test_lidar_max_dist_and_gain():
    """lidar_max_dist: max(0, md - d) / md; beyond md the reading is 0, never negative; exp gain"""
    C = _cfg(lidar_num_bins=4, lidar_max_dist=2.0, lidar_alias=False)
    obs, _ = _read(C, _pose(), [(0.0, 0.5), (-3.0, 0.0)])         # 90 deg at .5 -> bin 1; 180 deg at 3 -> bin 2
    np.testing.assert_allclose(obs, [0, 0.75, 0, 0], rtol=0, atol=1e-15)
    C = _cfg(lidar_num_bins=4, lidar_exp_gain=3.0, lidar_alias=False)
    obs, _ = _read(C, _pose(), [(0.0, -0.5)])                      # 270 deg -> bin 3
    np.testing.assert_allclose(obs, [0, 0, 0, math.exp(-1.5)], rtol=0, atol=1e-15)


def test_lidar_dropped_scatter_at_2pi():
    """choice 2, an angle that rounded to 2 pi: the write to bin B is dropped, the aliases land in bin 1 (x 0)
    and bin B-1 (x 1) -- bin 0 stays empty"""
    C = _cfg(lidar_num_bins=16)
    pos = np.array([[15.999999999]])
    s = np.array([[0.5]])
    np.testing.assert_allclose(ref64.lidar(C, pos, s, np.array([[2]]))[0],
                               np.eye(16)[15] * 0.5, rtol=0, atol=0)
    # the float64 reading of the same angle: bin 15 at alias ~1 -> bins 15 and 0
    got = ref64.lidar(C, pos, s)[0]
    assert got[15] == 0.5 and abs(got[0] - 0.5) < 1e-9 and got[14] < 1e-9


@pytest.mark.parametrize("hist", [0, 1, 2])
@pytest.mark.parametrize("d0,d1", [(0, 0), (1, 0), (0, 1), (1, 1)])
def test_vel_acc_history_rule(hist, d0, d1):
    """engine.py:902-929 with p = (.3, 0), last = (.1, 0), last_last = (0, 0), dt = .02, heading 0.
    hist 0 (last_done None): no history, vel = acc = 0.  hist 1 (last_last_done None): last_last is the
    CURRENT position, not the last one.  hist 2: last_last falls back to last where last_done + last_last_done"""
    C = _cfg()
    p, R = np.array([[0.3, 0.0]]), np.array([[1.0, 0.0]])
    pl, pll = np.array([[0.1, 0.0]]), np.array([[0.0, 0.0]])
    ld = None if hist < 1 else np.array([float(d0)])
    lld = None if hist < 2 else np.array([float(d1)])
    v, a = ref64.vel_acc(C, p, R, pl, pll, ld, lld)
    dt = 0.02
    if hist == 0 or d0:
        last = 0.3
    else:
        last = 0.1
    if hist == 0:
        lastlast = 0.3
    elif hist == 1:
        lastlast = 0.3
    else:
        lastlast = last if (d0 + d1) else 0.0
    vel = (0.3 - last) / dt
    acc = (vel - (last - lastlast) / dt) / dt
    np.testing.assert_allclose(v[0], [vel, 0], rtol=1e-12, atol=1e-9)
    np.testing.assert_allclose(a[0], [acc, 0], rtol=1e-12, atol=1e-9)


def test_reward_done_cost_by_hand():
    """reward = (last dist - dist) * reward_distance; done inside goal_size or |d_dist| > 1 (reward 0 there);
    timeout when steps > num_steps; cost = sum(size - min(d, size))"""
    C = ref64.Config(dict(hazards_num=2, goal_size=0.5, reward_distance=2.0, num_steps=10))
    N = 4
    qpos = np.array([[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]], np.float32)
    objs = np.zeros((N, 3, 2), np.float32)
    objs[:, 0] = [(0.4, 0.0), (2.0, 0.0), (2.0, 0.0), (2.0, 0.0)]        # goal: inside, outside x3
    objs[:, 1] = [(0.1, 0.0), (5, 5), (5, 5), (5, 5)]
    objs[:, 2] = [(0.0, -0.3), (5, 5), (5, 5), (5, 5)]
    pose0 = np.array([[0.0, 0.0, 1, 0], [0.5, 0.0, 1, 0], [-1.5, 0.0, 1, 0], [0.0, 0.0, 1, 0]], np.float32)
    pre = dict(qpos=qpos, qvel=np.zeros_like(qpos), pose0=pose0, pose1=pose0[:, :2], objs=objs,
               done0=np.zeros(N, np.float32), done1=np.zeros(N, np.float32),
               steps=np.array([3, 3, 3, 11], np.float32), hist=2)
    w = ref64.step(C, pre, np.zeros((N, 2), np.float32), qpos, np.zeros_like(qpos))
    np.testing.assert_allclose(w['reward'], [2 * (0.4 - 0.4), 2 * (1.5 - 2.0), 0.0, 0.0], atol=1e-7)
    np.testing.assert_array_equal(w['done'], [1, 0, 1, 1])      # in goal; no; |d_dist| = 1.5 > 1; timeout
    np.testing.assert_array_equal(w['steps'], [0, 4, 0, 0])
    np.testing.assert_allclose(w['cost'], [0.2 + 0.0, 0, 0, 0], atol=1e-7)


def test_robot_pose_matches_tree_kinematics():
    """the vectorised robot-body rule against TreeModel.kinematics of ant_np / walker_np, robot_rot included"""
    from oracle.ant_np import AntModel
    from oracle.walker_np import WalkerModel
    rng = np.random.default_rng(0)
    for robot, model in (("ant", AntModel()), ("walker", WalkerModel())):
        for rot in (None, 0.7):
            C = ref64.Config(dict(robot_base=EXTRA[robot]['robot_base'], robot_rot=rot))
            q = rng.uniform(-3, 3, (5, C.nq))
            got = ref64.robot_pose(C, q)
            for i in range(5):
                kin = model.kinematics(q[i])
                p, R = kin['xpos'][1], kin['R'][1]
                phi = rot or 0.0
                Rz = np.array([[math.cos(phi), -math.sin(phi)], [math.sin(phi), math.cos(phi)]])
                np.testing.assert_allclose(got[i, :2], Rz @ p[:2], atol=1e-12)
                np.testing.assert_allclose(got[i, 2:], Rz @ R[:2, 0], atol=1e-12)


@pytest.mark.parametrize("v", VARIANTS + CAPACITY[-1:])
def test_column_order_matches_engine(v):
    """the sorted-key column order (engine.py:773-777) derived here equals the engine's _obs_slices"""
    from guardx_amd.engine import Engine, _ROBOTS
    for robot in EXTRA:
        cfg = dict(v, **EXTRA[robot])
        E = Engine.__new__(Engine)
        E.parse(cfg)
        _, nq, nv, nu = _ROBOTS[E.robot_base][:4]
        E.robot = type('Robot', (), dict(nq=nq, nv=nv, nu=nu))()
        E.build_observation_space()
        C = ref64.Config(cfg)
        assert list(C.slices.items()) == list(E._obs_slices.items())
        assert C.D == E.obs_flat_size


def test_ref64_is_independent_of_the_checker():
    tree = ast.parse(open(os.path.join(ROOT, "oracle", "ref64.py")).read())
    names = set()
    for node in ast.walk(tree):
        if isinstance(node, ast.Import):
            names.update(a.name for a in node.names)
        elif isinstance(node, ast.ImportFrom):
            names.add(node.module or '')
            names.update(a.name for a in node.names)
    assert not any('gx_oracle_np' in n or n.split('.')[-1] == 'gxo' for n in names), names
    assert names <= {'math', 'os', 're', 'numpy', 'ant_np', 'walker_np', 'build_tables'}, names


# ---- the C checker against ref64 ---------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["point", "swimmer", "ant", "walker"])
@pytest.mark.parametrize("vi", range(len(VARIANTS)))
def test_checker_vs_ref64_variants(oracle, robot, vi):
    v = dict(VARIANTS[vi])
    if vi == 4:
        v.update(observe_vel=True, observe_acc=True)      # vel / acc with dt = 2 h as well
    run_checker_vs_ref64(oracle, robot, v)


@pytest.mark.parametrize("robot", ["point", "swimmer", "ant", "walker"])
@pytest.mark.parametrize("ci", range(len(CAPACITY)))
def test_checker_vs_ref64_capacity(oracle, robot, ci):
    run_checker_vs_ref64(oracle, robot, CAPACITY[ci], N=64, T=22, n_candidates=40000)


@pytest.mark.parametrize("hist", [0, 1, 2])
def test_checker_vs_ref64_history_states(oracle, hist):
    """set_state with every (done0, done1) mix at hist 0 / 1 / 2, vel and acc observed"""
    from helpers import random_state
    N = 256
    cfg = task_config(N, seed=5, observe_vel=True, observe_acc=True)
    O = oracle.OracleEngine(cfg, n_candidates=4000)
    O.reset(check=False)
    rng = np.random.default_rng(hist)
    s = random_state(N, 8, rng, done_frac=0.5)
    s['hist'] = hist
    O.set_state(s)
    act = rng.uniform(-1, 1, (N, 2)).astype(np.float32)
    o, r, d, info = O.step(act)
    post = O.get_state()
    C = ref64.Config(cfg)
    want = ref64.step(C, s, act, post['qpos'], post['qvel'])
    tally = ref64.check(C, dict(obs=o, reward=r, done=d, cost=info['cost'], steps=post['steps']), want)
    assert tally.frac() < 0.01
    assert post['hist'] == want['hist']
