"""The HIP dynamics pass (what a step does to qpos / qvel, and the pose it leaves in pose0) against the float64
robot models of tests/dyn64.py, which share nothing with the kernels or with the C checker: every robot on the
thread, lane-group and split paths, batch sizes at the lane-group kernels' edges, the config variants that change
which kernel runs (the persistent lane-group rollout among them), and directed states.  The state sets are those
of tests/test_dyn64.py, where the C checker alone is held to the same bounds.  The bit-for-bit comparison with the checker is kept beside it, so that a
failure says at once whether the kernel moved or both twins did; the float64 verdict does not depend on it.

Each step is compared from the engine's own fp32 state before it, so fp32 error never compounds.  thread / group:
set_state, step, get_state.  split / split-alone: a rollout of T = 3, chained through the rows' qpos / qvel columns
(no env of these sets is ever done, so every row is the step's own).

Worst error per env, max|d| / (1 + max|ref|), on the random states (N = 192), and the largest fraction of a
bound of dyn64.py reached ("of bound"; with pose0 on the step paths, which a rollout row does not carry), as
these tests print them.  The HIP figures equal the C checker's digit for digit, as bit equality implies:
              C checker (CPU) and HIP (MI355X),       HIP, split = split-alone,
              thread = group, one step                3 chained steps (576 env-steps)
    robot     qpos      qvel      of bound            qpos      qvel      of bound
    point     5.2e-08   9.7e-07   0.80                5.4e-08   9.7e-07   0.80
    swimmer   4.7e-08   4.0e-07   0.15                4.8e-08   1.0e-06   0.017
    ant       2.4e-05   1.05e-04  0.12                2.9e-05   1.22e-04  0.061
    walker    5.1e-06   1.66e-04  0.12                5.6e-06   2.45e-04  0.082
Directed states (16 per robot), worst over the paths: point 4.6e-08 / 6.0e-07, swimmer 4.0e-08 / 3.9e-07,
ant 1.4e-04 / 2.8e-04 (in the rollout's second and third step), walker 1.6e-06 / 2.1e-05.
"""
import numpy as np
import pytest

import dyn64
from oracle import ref64
from test_dyn64 import (ROBOTS, N_RANDOM, N_VARIANT, VARIANTS, config, random_set, directed_set, take, settle)

pytestmark = pytest.mark.gpu

PATHS = {"thread": 1, "group": 2, "split": 3, "split-alone": 3}
T_ROLLOUT = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _engine(cfg, path=None, n_candidates=20000):
    from guardx_amd import Engine
    E = Engine(cfg, n_candidates=n_candidates)
    if path is not None:
        E.set_path(PATHS[path])
        if path == "split-alone":
            E.set_prefetch(-1)
    E.reset(check=False)                    # the layouts are never used: set_state replaces every env
    return E


def _checker(oracle, cfg, E, n_candidates=20000):
    O = oracle.OracleEngine(cfg, n_candidates=n_candidates, env_total=E._cfg.env_total, env_offset=E._cfg.env_offset)
    O.reset(check=False)
    return O


def step_vs_dyn64(torch, oracle, cfg, path, s, act, worst, what):
    """set_state, step, get_state on `path` (None: the engine's own choice) against dyn64 and the checker"""
    E = _engine(cfg, path)
    O = _checker(oracle, cfg, E)
    E.set_state(s)
    _, _, done, _ = E.step(torch.from_numpy(act).cuda())
    st = E.get_state()
    E.close()
    assert not done.any().item()
    dyn64.check(cfg, dyn64.expect(cfg, s, act), st['qpos'], st['qvel'], st['pose0'], worst=worst, what=what)
    O.set_state(s)
    O.step(act)
    so = O.get_state()
    for k in ('qpos', 'qvel', 'pose0'):
        np.testing.assert_array_equal(st[k], so[k], err_msg=f"{what}: {k} against the checker")


def rollout_vs_dyn64(torch, oracle, cfg, path, s, acts, worst, what):
    """rollout of acts (T, n, A) from s on `path`: row t against dyn64 from row t - 1's qpos / qvel"""
    C = ref64.Config(cfg)
    qs, qv = C.slices['qpos'], C.slices['qvel']
    E = _engine(cfg, path)
    O = _checker(oracle, cfg, E)
    E.set_state(s)
    obs, rew, cost, done = (x.cpu().numpy() for x in E.rollout(torch.from_numpy(acts).cuda()))
    E.close()
    assert not done.any()                   # every row carries its step's qpos / qvel, no env is left out
    O.set_state(s)
    pre = s
    for t in range(acts.shape[0]):
        want = dyn64.expect(cfg, pre, acts[t])
        dyn64.check(cfg, want, obs[t][:, qs], obs[t][:, qv], worst=worst, what=f"{what} t={t}")
        O.step(acts[t])
        so = O.get_state()
        np.testing.assert_array_equal(obs[t][:, qs], so['qpos'], err_msg=f"{what} t={t}: qpos against the checker")
        np.testing.assert_array_equal(obs[t][:, qv], so['qvel'], err_msg=f"{what} t={t}: qvel against the checker")
        # the Point's next ctrl reads the heading this step left in pose0, which a row does not carry
        pre = dict(qpos=obs[t][:, qs], qvel=obs[t][:, qv],
                   pose0=dyn64.expected_pose0(C, want, obs[t][:, qs], obs[t][:, qv])[0])


def _run(torch, oracle, cfg, path, s, act, worst, what):
    """one step on the step paths; on the split paths T_ROLLOUT steps, the actions rotated env-wise step by step"""
    if path in ("split", "split-alone"):
        acts = np.stack([np.roll(act, t, axis=0) for t in range(T_ROLLOUT)])
        rollout_vs_dyn64(torch, oracle, cfg, path, s, acts, worst, what)
    else:
        step_vs_dyn64(torch, oracle, cfg, path, s, act, worst, what)


# ---- random states: robots x paths --------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_random_states_vs_dyn64(torch_cuda, oracle, robot, path):
    s, act = random_set(robot)
    if robot in dyn64.TREE_BOUND:
        nlim, ncon = dyn64.rows_count(robot, s)
        assert nlim > 100 and ncon > 100, (nlim, ncon)       # the set exercises limit rows and contact rows
    worst = dyn64.Worst()
    _run(torch_cuda, oracle, config(robot, N_RANDOM), path, s, act, worst, f"{robot} {path}")
    print(f"HIP {robot} {path} random: {worst}")
    assert worst.envs == N_RANDOM * (T_ROLLOUT if path.startswith("split") else 1)


# ---- batch sizes at the kernels' edges ----------------------------------------------------------------------
# lane-group: 4 envs of 16 lanes per wave -- a lone env, a wave short of one env, a full wave, one env over,
# a tail of one, and both sides of 64; thread: both sides of a wave of envs
SIZES = [("group", r, n) for r in ("ant", "walker") for n in (1, 3, 4, 5, 17, 63, 65)] + \
        [("thread", "walker", n) for n in (1, 63, 64, 65)]


@pytest.mark.parametrize("path,robot,N", SIZES)
def test_sizes_vs_dyn64(torch_cuda, oracle, path, robot, N):
    """the last N envs of the random set, so that the tail lanes hold other states at every size; every env,
    the tail included, is compared"""
    s, act = random_set(robot)
    s, act = take(s, slice(N_RANDOM - N, N_RANDOM)), act[N_RANDOM - N:]
    worst = dyn64.Worst()
    step_vs_dyn64(torch_cuda, oracle, config(robot, N), path, s, act, worst, f"{robot} {path} N={N}")
    print(f"HIP {robot} {path} N={N}: {worst}")
    assert worst.envs == N


# ---- variants that change which kernel runs -----------------------------------------------------------------
@pytest.mark.parametrize("path", ["thread", "group", "rollout"])
@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_variants_vs_dyn64(torch_cuda, oracle, robot, variant, path):
    """two physics steps per control step, an observation with vel, and a turned root body (which must move
    pose0 only), each on the thread and lane-group step kernels by explicit choice and through a rollout with the
    split path chosen.  The two-kernel rollout has no form for the first two variants, so their rollout runs the
    persistent lane-group kernel instead; which of the two ran is asserted through the engine's own statement of
    it: tape_floats() refuses exactly the configs that gx_rollout does not split."""
    from guardx_amd._native import GxError
    s, act = random_set(robot)
    s, act = take(s, slice(0, N_VARIANT)), act[:N_VARIANT]
    cfg = config(robot, N_VARIANT, **VARIANTS[variant])
    if path == "rollout":
        E = _engine(cfg, "split")
        try:
            E.tape_floats(T_ROLLOUT)
            splits = True
        except GxError:
            splits = False
        E.close()
        assert splits == (variant == "rot"), (robot, variant)
    worst = dyn64.Worst()
    _run(torch_cuda, oracle, cfg, "split" if path == "rollout" else path, settle(cfg, s), act, worst,
         f"{robot} {variant} {path}")
    print(f"HIP {robot} {variant} {path}: {worst}")


def test_robot_rot_moves_pose0_only(torch_cuda):
    """robot_rot = 0.9 against 0 on the same states: qpos / qvel bit for bit the same, pose0 turned"""
    torch = torch_cuda
    for robot in ROBOTS:
        s, act = random_set(robot)
        s, act = take(s, slice(0, N_VARIANT)), act[:N_VARIANT]
        out = []
        for rot in (None, 0.9):
            E = _engine(config(robot, N_VARIANT, robot_rot=rot))
            E.set_state(s)
            E.step(torch.from_numpy(act).cuda())
            out.append(E.get_state())
            E.close()
        np.testing.assert_array_equal(out[0]['qpos'], out[1]['qpos'])
        np.testing.assert_array_equal(out[0]['qvel'], out[1]['qvel'])
        c, sn = np.cos(0.9), np.sin(0.9)
        p0, p1 = out[0]['pose0'].astype(np.float64), out[1]['pose0']
        turned = np.stack([c * p0[:, 0] - sn * p0[:, 1], sn * p0[:, 0] + c * p0[:, 1],
                           c * p0[:, 2] - sn * p0[:, 3], sn * p0[:, 2] + c * p0[:, 3]], axis=1)
        # each pose is within its bound of the true one; turning the first spreads its error over two components
        np.testing.assert_allclose(p1, turned, rtol=0, atol=(1 + np.sqrt(2)) * dyn64.POSE_ATOL[robot])


# ---- directed states ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", list(PATHS))
@pytest.mark.parametrize("robot", ROBOTS)
def test_directed_states_vs_dyn64(torch_cuda, oracle, robot, path):
    """the sixteen directed states of test_dyn64.directed_set (each passes there for the checker alone, so none
    is excluded or expected to fail here); a failure names the first state beyond its bound"""
    s, act, names = directed_set(robot)
    worst = dyn64.Worst()
    try:
        _run(torch_cuda, oracle, config(robot, len(names)), path, s, act, worst, f"{robot} {path} directed")
    except AssertionError as e:
        raise AssertionError(f"{e}\nenvs: {list(enumerate(names))}") from None
    print(f"HIP {robot} {path} directed: {worst}")
    assert worst.envs == 16 * (T_ROLLOUT if path.startswith("split") else 1)
