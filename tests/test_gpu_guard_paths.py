"""The case sets of tests/guard_cases.py on Engine, every path, against the checker bit for bit (NaN equal to NaN): obs,
reward, cost, done, every reset_done observation and the final state.  The sets sit on both sides of every threshold of
the rollout kernels' fast / exact step switch and hold non-finite and huge values in every kind of state entry and
action (tests/test_guard_cases.py proves on the CPU which side each row landed on, and that the same checks catch three
planted mistakes of the switch).

  rollout(actions), rollout(actions, packed=True)   thread, group, split, split-alone (the last selects the Swimmer's
                                                     quad-per-env dynamics pass and the Ant's / Walker's one env per
                                                     wave; two per wave need more than 1024 envs:
                                                     test_rollout_two_envs_per_wave)
  step() + reset_done()                              thread, group: also the guard property and ref64 on the finite rows
                                                     from the engine's own get_state

Neighbour independence: every set runs once as built and once with every planted row replaced by its ordinary original;
the untouched envs' rows must be bit-identical between the two runs -- cross-lane leakage through the wave-uniform
branches shows without relying on the checker."""
import numpy as np
import pytest

import guard_cases as gc
from helpers import assert_state_equal
from oracle import ref64
from test_guard_cases import check_step, FarGoal

pytestmark = pytest.mark.gpu

PATHS = {"thread": 1, "group": 2, "split": 3, "split-alone": 3}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _engine(cfg, path, n_candidates=gc.N_CANDIDATES):
    from guardx_amd import Engine
    E = Engine(cfg, n_candidates=n_candidates)
    E.set_path(PATHS[path])
    if path == "split-alone":
        E.set_prefetch(-1)
    return E


def _np(x):
    return x.cpu().numpy()


def _rollout(torch, E, state, acts, packed):
    E.set_state(state)
    out = E.rollout(torch.from_numpy(acts).cuda(), packed=packed)
    res = [_np(x) for x in out[:4]]
    if packed:
        D = E.obs_flat_size
        np.testing.assert_array_equal(_np(out[4])[..., D:D + acts.shape[2]], acts)
    return res


@pytest.mark.parametrize("robot", gc.ROBOTS)
@pytest.mark.parametrize("path", list(PATHS))
def test_rollout_guard_paths(torch_cuda, robot, path):
    """every case set under every config through rollout(actions) and rollout(actions, packed=True): each step's obs
    (the reset_done observation), reward, cost and done and the final state equal the checker's; the untouched envs'
    rows equal those of the run without the planted rows"""
    torch = torch_cuda
    for cname in gc.CONFIGS:
        E = _engine(gc.config(robot, cname), path)
        E.reset()
        for cs, rows, final in gc.checker_runs(robot, cname):
            what = f"{robot} {path} {cname} {cs['label']}"
            for packed in (False, True):
                obs, rew, cost, done = _rollout(torch, E, cs['state'], cs['acts'], packed)
                for t, rec in enumerate(rows):
                    np.testing.assert_array_equal(obs[t], rec['rd'], err_msg=f"{what} packed={packed} t={t}: obs")
                    np.testing.assert_array_equal(rew[t], rec['rew'], err_msg=f"{what} packed={packed} t={t}: reward")
                    np.testing.assert_array_equal(cost[t], rec['cost'], err_msg=f"{what} packed={packed} t={t}: cost")
                    np.testing.assert_array_equal(done[t], rec['done'], err_msg=f"{what} packed={packed} t={t}: done")
                assert_state_equal(E.get_state(), final)
            # neighbour independence
            plain = _rollout(torch, E, cs['plain_state'], cs['plain_acts'], False)
            keep = ~cs['planted']
            for a, b, k in zip((obs, rew, cost, done), plain, ("obs", "reward", "cost", "done")):
                np.testing.assert_array_equal(a[:, keep], b[:, keep], err_msg=f"{what}: untouched envs' {k}")
        E.close()


@pytest.mark.parametrize("robot", ["ant", "walker"])
def test_rollout_two_envs_per_wave(torch_cuda, oracle, robot):
    """alone on the chip the Ant's / Walker's dynamics pass takes one env per wave up to 1024 envs (N = 67 above) and two
    up to 2048: two case sets, sixteen times side by side (1072 envs), on split-alone.  An odd N shifts every other copy
    by one lane group, so the planted pairs fall into one wave in some copies and into two in others."""
    torch = torch_cuda
    K, M = 16, 200000                                       # about 2 % of the candidates are valid layouts
    cfg = dict(gc.config(robot, "default"), env_num=K * gc.N)
    assert 1024 < cfg['env_num'] <= 2048
    E = _engine(cfg, "split-alone", n_candidates=M)
    O = oracle.OracleEngine(cfg, n_candidates=M)
    E.reset()
    O.reset()
    for cs in gc.case_sets(robot):
        if cs['label'] not in ("values0", "thresholds0"):
            continue
        cs = gc.tiled(cs, K)
        rows, final = gc.run_checker(O, cs['state'], cs['acts'])
        obs, rew, cost, done = _rollout(torch, E, cs['state'], cs['acts'], False)
        for t, rec in enumerate(rows):
            for a, k in ((obs[t], 'rd'), (rew[t], 'rew'), (cost[t], 'cost'), (done[t], 'done')):
                np.testing.assert_array_equal(a, rec[k], err_msg=f"{robot} {cs['label']} t={t}: {k}")
        assert_state_equal(E.get_state(), final)
        plain = _rollout(torch, E, cs['plain_state'], cs['plain_acts'], False)
        keep = ~cs['planted']
        for a, b, k in zip((obs, rew, cost, done), plain, ("obs", "reward", "cost", "done")):
            np.testing.assert_array_equal(a[:, keep], b[:, keep], err_msg=f"{robot} {cs['label']}: untouched envs' {k}")
    E.close()


def _steps(torch, E, state, acts):
    E.set_state(state)
    out = []
    for t in range(acts.shape[0]):
        pre = E.get_state()
        o, r, d, info = E.step(torch.from_numpy(acts[t]).cuda())
        post = E.get_state()
        o, r, d, c = _np(o), _np(r), _np(d), _np(info['cost'])
        rd = _np(E.reset_done())
        out.append(dict(pre=pre, act=acts[t], obs=o, rew=r, cost=c, done=d, post=post, rd=rd))
    return out, E.get_state()


@pytest.mark.parametrize("robot", gc.ROBOTS)
@pytest.mark.parametrize("path", ["thread", "group"])
def test_step_guard_paths(torch_cuda, robot, path):
    """the same through step() + reset_done(): equal to the checker, and -- from the engine's own get_state -- the
    guard property, ref64 on the finite rows and the derived reward bound, as tests/test_guard_cases.py applies them to
    the checker"""
    torch = torch_cuda
    for cname in gc.CONFIGS:
        cfg = gc.config(robot, cname)
        C = ref64.Config(cfg)
        E = _engine(cfg, path)
        E.reset()
        tally, far = ref64.Tally(), FarGoal()
        for cs, rows, final in gc.checker_runs(robot, cname):
            got, last = _steps(torch, E, cs['state'], cs['acts'])
            for t, (g, rec) in enumerate(zip(got, rows)):
                what = f"{robot} {path} {cname} {cs['label']} t={t}"
                for k in ('obs', 'rew', 'cost', 'done', 'rd'):
                    np.testing.assert_array_equal(g[k], rec[k], err_msg=f"{what}: {k}")
                # the guard property and ref64 from the engine's own states
                check_step(robot, C, g['pre'], g['act'], g['obs'], g['rew'], g['cost'], g['done'], g['post'], tally,
                           far, what)
            assert_state_equal(last, final)
            # neighbour independence
            plain, _ = _steps(torch, E, cs['plain_state'], cs['plain_acts'])
            keep = ~cs['planted']
            for t, (g, p) in enumerate(zip(got, plain)):
                for k in ('obs', 'rew', 'cost', 'done', 'rd'):
                    np.testing.assert_array_equal(g[k][keep], p[k][keep],
                                                  err_msg=f"{robot} {path} {cname} {cs['label']} t={t}: untouched envs' {k}")
        E.close()
        print(f"{robot} {path} {cname}: {tally}; reward error / derived bound: worst {far.worst:.3f}, "
              f"with the goal >= 1000 away {far.worst_far:.3f}")
        assert tally.frac() < 0.01, tally
