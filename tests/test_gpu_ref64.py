"""HIP outputs against the float64 restatement (oracle/ref64.py) directly: configs x paths, capacity shapes,
batch sizes at the kernels' thresholds, and directed edge states.  Where the checker is cheap the bit-exact
comparison is kept as well."""

import numpy as np
import pytest

from helpers import task_config, random_state
from oracle import ref64
from test_ref64 import VARIANTS, CAPACITY, EXTRA, check_reset_done

pytestmark = pytest.mark.gpu

PATHS = {"thread": 1, "group": 2, "split": 3, "split-alone": 3}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


def _engine(cfg, path=None, n_candidates=30000):
    from guardx_amd import Engine
    E = Engine(cfg, n_candidates=n_candidates)
    if path is not None:
        E.set_path(PATHS[path])
        if path == "split-alone":
            E.set_prefetch(-1)
    return E


def _np(x):
    return x.cpu().numpy()


def steps_vs_ref64(torch, E, C, T, rng, tally, rd_every=5, oracle=None):
    """T x step (reset_done every rd_every-th) of the engine, each checked against ref64 from the engine's own
    pre-step state and post-step joint state; with `oracle` (same config) also bit for bit against the checker"""
    N, A = E.env_num, E.action_space.shape[0]
    for t in range(T):
        pre = E.get_state()
        act = rng.uniform(-1, 1, (N, A)).astype(np.float32)
        o, r, d, info = E.step(torch.from_numpy(act).cuda())
        post = E.get_state()
        o, r, d, c = _np(o), _np(r), _np(d), _np(info['cost'])
        want = ref64.step(C, pre, act, post['qpos'], post['qvel'])
        ref64.check(C, dict(obs=o, reward=r, done=d, cost=c, steps=post['steps']), want, tally,
                    what=f"step t={t}")
        if oracle is not None:
            oo, ro, do, io = oracle.step(act)
            np.testing.assert_array_equal(o, oo)
            np.testing.assert_array_equal(r, ro)
            np.testing.assert_array_equal(d, do)
        if t % rd_every == rd_every - 1:
            rd = _np(E.reset_done())
            check_reset_done(C, o, d, rd, E.get_state(), tally)
            if oracle is not None:
                np.testing.assert_array_equal(rd, oracle.reset_done())


def rollout_vs_ref64(torch, E, C, T, rng, tally, packed=False):
    """fused rollout: each env's rows up to its first done against ref64 chained through the obs rows' qpos /
    qvel columns; the done row on reward, cost and done (its obs is the next episode's)"""
    N, A = E.env_num, E.action_space.shape[0]
    s = E.get_state()
    acts = rng.uniform(-1, 1, (T, N, A)).astype(np.float32)
    out = E.rollout(torch.from_numpy(acts).cuda(), packed=packed)
    obs, rew, cost, done = (_np(x) for x in out[:4])
    if packed:
        pk = _np(out[4])
        np.testing.assert_array_equal(pk[..., C.D:C.D + A], acts)
    return rows_vs_ref64(C, s, acts, obs, rew, cost, done, tally)


def rows_vs_ref64(C, s, acts, obs, rew, cost, done, tally):
    """the rollout rows (T, n, ...) of n envs that started from state s, against ref64 up to each env's first
    done.  With physics_steps_per_control_step > 1 the done row's pose would need the step's own qpos / qvel,
    which the row does not carry (it holds the next episode's): those rows are counted as excluded."""
    T, N = done.shape
    alive = np.ones(N, bool)
    qs, qv = C.slices['qpos'], C.slices['qvel']
    for t in range(T):
        want = ref64.step(C, s, acts[t], obs[t][:, qs], obs[t][:, qv])
        got = dict(obs=obs[t], reward=rew[t], done=done[t], cost=cost[t])
        cont = alive & (done[t] == 0)
        ref64.check(C, got, want, tally, rows=np.nonzero(cont)[0], what=f"rollout t={t}")
        last = alive & (done[t] > 0)
        if C.k == 1:
            ref64.check(C, got, want, tally, rows=np.nonzero(last)[0], compare_obs=False, what=f"rollout t={t}")
        else:
            tally.entries += 3 * int(last.sum())
            tally.excluded += 3 * int(last.sum())
        alive = cont
        s = dict(qpos=obs[t][:, qs], qvel=obs[t][:, qv], pose0=want['pose0'], pose1=want['pose1'],
                 objs=s['objs'], done0=done[t], done1=s['done0'], steps=want['steps'], hist=want['hist'])
    return alive


# ---- configs x paths ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["point", "swimmer", "ant", "walker"])
@pytest.mark.parametrize("path", list(PATHS))
def test_variants_vs_ref64(torch_cuda, robot, path):
    torch = torch_cuda
    tally = ref64.Tally()
    for vi, v in enumerate(VARIANTS):
        N = 130
        cfg = task_config(N, seed=9, num_steps=12, **v, **EXTRA[robot])
        E = _engine(cfg, path)
        C = ref64.Config(cfg)
        assert list(C.slices.items()) == list(E._obs_slices.items())
        E.reset()
        rng = np.random.default_rng(vi)
        steps_vs_ref64(torch, E, C, 16, rng, tally)
        if 'qpos' in C.slices:
            rollout_vs_ref64(torch, E, C, 9, rng, tally)
        E.close()
    print(f"{robot} {path}: {tally}")
    assert tally.frac() < 0.01, tally


# ---- capacity shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("robot", ["point", "swimmer", "ant", "walker"])
@pytest.mark.parametrize("path", ["thread", "group", "split"])
def test_capacity_vs_ref64(torch_cuda, oracle, robot, path):
    """bins 3..64, up to 65 objects (64 hazards; 40 hazards + 24 observed pillars): the (5, 4) lane-group / split
    forms at full capacity and PMAX = 33; the last shape is each robot's widest row, also through
    rollout(packed=True).  The first shape is kept bit for bit against the checker too."""
    torch = torch_cuda
    tally = ref64.Tally()
    for ci, v in enumerate(CAPACITY):
        N = 96
        cfg = task_config(N, seed=4, num_steps=15, **v, **EXTRA[robot])
        E = _engine(cfg, path, n_candidates=40000)
        C = ref64.Config(cfg)
        O = None
        if ci in (0, len(CAPACITY) - 1):
            O = oracle.OracleEngine(cfg, n_candidates=40000, env_total=E._cfg.env_total, env_offset=E._cfg.env_offset)
            np.testing.assert_array_equal(_np(E.reset()), O.reset())
        else:
            E.reset()
        rng = np.random.default_rng(ci)
        steps_vs_ref64(torch, E, C, 8, rng, tally, rd_every=4, oracle=O)
        rollout_vs_ref64(torch, E, C, 6, rng, tally, packed=(ci == len(CAPACITY) - 1))
        E.close()
    print(f"{robot} {path}: {tally}")
    assert tally.frac() < 0.01, tally


# ---- batch sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path,N", [(p, n) for p in ("thread", "group") for n in (1, 63, 64, 65, 255, 257)]
                         + [("split-alone", n) for n in (1024, 1025, 2048, 2049)])
def test_sizes_vs_ref64(torch_cuda, path, N):
    torch = torch_cuda
    cfg = task_config(N, seed=N, num_steps=10, goal_size=0.9, observe_vel=True, observe_acc=True, **EXTRA["ant"]) \
        if path == "split-alone" else task_config(N, seed=N, num_steps=10, goal_size=0.9)
    E = _engine(cfg, path, n_candidates=200000)           # about 2 % of the candidates are valid layouts
    C = ref64.Config(cfg)
    E.reset()
    tally = ref64.Tally()
    rng = np.random.default_rng(1)
    steps_vs_ref64(torch, E, C, 6, rng, tally, rd_every=3)
    rollout_vs_ref64(torch, E, C, 12, rng, tally)
    E.close()
    assert tally.frac() < 0.01, tally


# ---- directed edges -----------------------------------------------------------------------------------------
EDGE_N = 7 * 64          # seven waves of 64 envs, each with its own kind of edge


def _edge_state(rng, bins, H=8):
    """set_state input: robots at rest at the origin, heading 0, so the robot-frame vector of an object is its
    own fp32 coordinates (k = 1: the pose of the step is the pre-step qpos).  Wave by wave:
      0-2  every object on a bin edge k * 2 pi / B with k >= 1 and dist >= .6: no angle below 2^-100 anywhere in
           the wave, so 16 bins take the div_bin16 fast path; even envs at steps = num_steps + 1 (timeout),
           odd ones at num_steps (not a timeout)
      3    the same, plus one env with a positive angle below 2^-100 (1, 2^-110): the wave's true division
      4    objects at (1, -1e-30) (atan2 -> -tiny, the remainder rounds to 2 pi), hazards on the robot (dist 0)
           and at exactly hazards_size
      5    the goal at dist = goal_size and +- 1 ulp
      6    |d_dist| at 1 and 1 +- 1 ulp (both signs): the goal at .75 (or 1.75) on the x axis, the last pose on
           the x axis so that the last distance is 1.75 (or .75) and its fp32 neighbours"""
    N = EDGE_N
    f = np.float32
    s = random_state(N, H, rng, done_frac=0.0)
    s['qpos'][:] = 0.0
    s['qvel'][:] = 0.0
    s['pose0'][:] = (0.0, 0.0, 1.0, 0.0)
    s['pose1'][:] = 0.0
    s['hist'] = 2
    s['steps'][:] = 3
    s['steps'][0:192:2] = 4
    k = 1 + rng.integers(0, bins - 1, (N, 1 + H))
    ang = (2 * np.pi / bins) * k
    r = rng.uniform(0.6, 2.0, ang.shape)
    s['objs'] = np.stack([r * np.cos(ang), r * np.sin(ang)], -1).astype(f)
    s['objs'][3 * 64 + 5, 1] = (1.0, f(2.0 ** -110))
    w = slice(4 * 64, 5 * 64)
    s['objs'][w, 2] = (1.0, f(-1e-30))
    s['objs'][w, 3] = (f(0.7), f(-1e-30))
    s['objs'][w][0::2, 1] = 0.0
    s['objs'][w][1::2, 1] = (f(0.3), 0.0)
    g = f(0.5)
    for j, x in enumerate((g, np.nextafter(g, f(1)), np.nextafter(g, f(0)))):
        s['objs'][5 * 64 + j:6 * 64:3, 0] = (x, 0.0)
    rows = np.arange(6 * 64, 7 * 64)
    for j, (gx, L) in enumerate(((0.75, 1.75), (1.75, 0.75))):
        for i, Lx in enumerate((f(L), np.nextafter(f(L), f(4)), np.nextafter(f(L), f(0)))):
            sel = rows[(2 * i + j)::6]
            s['objs'][sel, 0] = (gx, 0.0)
            s['pose0'][sel, 0] = f(gx) - Lx              # exact: the last distance is Lx
    return s


EDGE_CASES = [(16, 1.0, True), (17, 1.0, True), (64, 1.0, True), (16, 200.0, True), (16, 1.0, False),
              (17, 1.0, False), (64, 1.0, False)]


@pytest.mark.parametrize("bins,gain,alias", EDGE_CASES)
@pytest.mark.parametrize("path", ["thread", "group"])
def test_directed_edges_vs_ref64(torch_cuda, oracle, bins, gain, alias, path):
    """the edge states of _edge_state (16 bins: the div_bin16 fast path in waves 0-2, the true division in wave 3;
    gain 200: readings below exp(-87)) against ref64 edge-aware and against the checker bit for bit.  With the
    alias on, a reading is continuous across a bin edge; with it off the bin assignment shows, and the
    either-assignment search of ref64 must find the kernel's"""
    torch = torch_cuda
    N = EDGE_N
    cfg = task_config(N, seed=3, num_steps=3, lidar_num_bins=bins, lidar_exp_gain=gain, lidar_alias=alias)
    E = _engine(cfg, path)
    O = oracle.OracleEngine(cfg, n_candidates=30000, env_total=E._cfg.env_total, env_offset=E._cfg.env_offset)
    E.reset()
    O.reset()
    C = ref64.Config(cfg)
    s = _edge_state(np.random.default_rng(bins), bins)
    E.set_state(s)
    O.set_state(s)
    act = np.zeros((N, 2), np.float32)
    o, r, d, info = E.step(torch.from_numpy(act).cuda())
    post = E.get_state()
    o, r, d, c = _np(o), _np(r), _np(d), _np(info['cost'])
    want = ref64.step(C, s, act, post['qpos'], post['qvel'])
    tally = ref64.check(C, dict(obs=o, reward=r, done=d, cost=c, steps=post['steps']), want, what="edges")
    print(f"edges bins={bins} gain={gain} alias={alias} {path}: {tally}")
    assert tally.frac() < 0.01, tally
    assert tally.either_rows >= 100                     # waves 5 and 6
    if not alias:
        assert tally.edge_rows > 0
    oo, ro, do, io = O.step(act)
    np.testing.assert_array_equal(o, oo)
    np.testing.assert_array_equal(r, ro)
    np.testing.assert_array_equal(d, do)
    np.testing.assert_array_equal(c, io['cost'])
    E.close()
    # timeouts: steps = num_steps + 1 is done whatever else, num_steps is not a timeout
    assert (d[0:192:2] == 1).all()
    np.testing.assert_array_equal(d[1:192:2], want['done'][1:192:2])


# ---- 2^22 + 37 envs ----------------------------------------------------------------------------------------
def _state_rows(s, idx):
    return {k: (v[idx] if isinstance(v, np.ndarray) and v.ndim and v.shape[0] > 2 else v) for k, v in s.items()}


def test_large_batch_vs_oracle_slices_and_ref64(torch_cuda, oracle):
    """N = 2^22 + 37 (the README's bandwidth regime; Npad rounds it up to a 256-multiple, the last block is
    partial): step() and rollout() with K = 4, bit for bit against checker engines on three contiguous slices
    (the first 256 envs, 256 across a 256-boundary in the middle, the last 300), and against ref64 on a seeded
    sample of 64 k envs.  For the rollout, whose resets happen in the kernel, a slice's checker is built with the
    engine's seed and candidate count and env_total = N, env_offset = the slice start, and is reset -- so that it
    draws the same pool and layout rows -- before set_state loads the slice."""
    torch = torch_cuda
    N, K, M = (1 << 22) + 37, 4, 20000
    cfg = task_config(N, seed=21, num_steps=6, goal_size=0.9)
    E = _engine(cfg, n_candidates=M)
    E.reset(check=False)                      # fewer valid layouts than envs: rows repeat (check deferred)
    C = ref64.Config(cfg)
    mid = (1 << 21) - 100
    slices = [(0, 256), (mid, mid + 256), (N - 300, N)]
    sample = np.sort(np.random.default_rng(0).choice(N, 65536, replace=False))
    gen = torch.Generator(device='cuda').manual_seed(5)
    tally = ref64.Tally()
    # step()
    pre = E.get_state()
    act_d = torch.rand(N, 2, device='cuda', generator=gen) * 2 - 1
    o, r, d, info = E.step(act_d)
    post = E.get_state()
    act = act_d.cpu().numpy()
    o, r, d, c = _np(o), _np(r), _np(d), _np(info['cost'])
    for a, b in slices:
        sl = {**_state_rows(pre, slice(a, b))}
        cs = dict(cfg, env_num=b - a)
        O = oracle.OracleEngine(cs, n_candidates=M, env_total=N, env_offset=a)
        O.reset(check=False)
        O.set_state(sl)
        oo, ro, do, io = O.step(act[a:b])
        np.testing.assert_array_equal(o[a:b], oo)
        np.testing.assert_array_equal(r[a:b], ro)
        np.testing.assert_array_equal(d[a:b], do)
        np.testing.assert_array_equal(c[a:b], io['cost'])
    want = ref64.step(C, _state_rows(pre, sample), act[sample], post['qpos'][sample], post['qvel'][sample])
    ref64.check(C, dict(obs=o[sample], reward=r[sample], done=d[sample], cost=c[sample],
                        steps=post['steps'][sample]), want, tally, what="2^22+37 step")
    del o, r, d, c
    # rollout(), K = 4, from the state after reset_done
    E.reset_done()
    s0 = E.get_state()
    acts_d = torch.rand(K, N, 2, device='cuda', generator=gen) * 2 - 1
    obs_d, rew_d, cost_d, done_d = E.rollout(acts_d)
    acts = acts_d.cpu().numpy()
    for a, b in slices:
        cs = dict(cfg, env_num=b - a)
        O = oracle.OracleEngine(cs, n_candidates=M, env_total=N, env_offset=a)
        O.reset(check=False)
        O.set_state(_state_rows(s0, slice(a, b)))
        for t in range(K):
            oo, ro, do, io = O.step(acts[t, a:b])
            np.testing.assert_array_equal(_np(obs_d[t, a:b]), O.reset_done())
            np.testing.assert_array_equal(_np(rew_d[t, a:b]), ro)
            np.testing.assert_array_equal(_np(done_d[t, a:b]), do)
            np.testing.assert_array_equal(_np(cost_d[t, a:b]), io['cost'])
    idx = torch.from_numpy(sample).cuda()
    rows_vs_ref64(C, _state_rows(s0, sample), acts[:, sample], _np(obs_d[:, idx]), _np(rew_d[:, idx]),
                  _np(cost_d[:, idx]), _np(done_d[:, idx]), tally)
    print(f"2^22+37: {tally}")
    assert tally.frac() < 0.01, tally
    del obs_d, rew_d, cost_d, done_d
    E.close()


# ---- rollout_policy limits ---------------------------------------------------------------------------------
def test_rollout_policy_limits(torch_cuda, oracle):
    """gx_rollout_policy accepts hazards_num 15, 16 bins and N = 65536 and matches the checker on obs, reward,
    cost and done; N = 65537 is refused"""
    torch = torch_cuda
    from guardx_amd import Engine
    from guardx_amd._native import GxError
    from test_policy_rollout import _torch_ac
    N, T = 65536, 3
    over = dict(hazards_num=15, lidar_num_bins=16, placements_extents=[-4, -4, 4, 4], hazards_keepout=0.2)
    cfg = task_config(N, seed=8, num_steps=30, goal_size=0.9, **over)
    E = _engine(cfg, n_candidates=60000)
    O = oracle.OracleEngine(cfg, n_candidates=60000)
    og, oo = _np(E.reset(check=False)), O.reset(check=False)
    np.testing.assert_array_equal(og, oo)
    mu_net, v_net, log_std = _torch_ac(E.obs_flat_size, 2, seed=5)
    params = Engine.pack_actor_critic(mu_net=mu_net, v_net=v_net, log_std=log_std)
    g = E.rollout_policy(params.cuda(), T, noise_seed=(3, 4))
    o = O.rollout_policy(params.numpy(), T, oo, noise_seed=(3, 4))
    for k in ('obs', 'rew', 'cost', 'done', 'obs_last'):
        np.testing.assert_array_equal(g[k].cpu().numpy(), o[k], err_msg=k)
    E.close()
    F = _engine(dict(cfg, env_num=N + 1), n_candidates=60000)
    F.reset(check=False)
    with pytest.raises(GxError, match="65536"):
        F.rollout_policy(params.cuda(), T, noise_seed=(3, 4))
    F.close()
