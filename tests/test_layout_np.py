"""tests/layout_np.py (the layout sampler's whole pool in numpy float32) against the scalar numpy transcription and
against the C checker, on the arenas tests/test_gpu_layout_sampler.py runs on the device: sizes around a wave, a block
and a compaction tile, pools of zero / one / two rows, nearly every candidate valid, dense arenas, margins, thresholds
that are no exact floats, 3 to 24 objects, pillars, fixed locations, per-object rectangles and the phase-0 pruning edge.
Everything is compared bit for bit.  Each case's stated condition is asserted on the numpy pool alone, so a changed
seed or size that empties a case fails here; two planted mistakes show that the comparison can fail."""
import functools

import numpy as np
import pytest

import layout_np as ln
from layout_np import CASE, CASES, SHARDED
from oracle import gx_oracle_np as onp

f32 = np.float32


@functools.lru_cache(maxsize=None)
def _pool(name, reset=0, mistake=None):
    c = CASE[name]
    rows, ok = ln.sample_pool(c.cfg, c.key(reset), c.M, mistake=mistake, rows_of_failed=False)
    rows.setflags(write=False); ok.setflags(write=False)
    return rows, ok


# ---- the vectorised statement against the scalar one ---------------------------------------------------------------
SCALAR = [
    ("default", 7, {}),
    ("pillars", 9, dict(hazards_num=4, pillars_num=5, placements_extents=[-3, -3, 3, 3])),
    ("margin", 11, dict(placements_margin=0.15, hazards_keepout=0.37)),
]


@pytest.mark.parametrize("name,seed,over", SCALAR, ids=[s[0] for s in SCALAR])
def test_sample_pool_equals_the_scalar_transcription(name, seed, over):
    """rows and success of every one of the first 150 candidates, the failed ones (their -inf rows) included"""
    M = 150
    cfg = ln.task_config(ln.ENV_NUM, seed=seed, **over)
    key = np.array([0, seed], np.uint32)
    rows, ok = ln.sample_pool(cfg, key, M)
    keys = onp.split(key, M)
    d = {**ln.DEFAULTS, **over}
    for j in range(M):
        lay, s = onp.sample_layout(keys[j], hazards_num=d['hazards_num'], extents=d['placements_extents'],
                                   keepouts=(d['goal_keepout'], d['hazards_keepout'], d['robot_keepout']),
                                   margin=d['placements_margin'], pillars_num=d['pillars_num'],
                                   pillars_keepout=d['pillars_keepout'])
        np.testing.assert_array_equal(rows[j], lay, err_msg=f"candidate {j}")
        assert bool(s) == bool(ok[j]), j
    assert ln.failed_all_tries(rows).any() or name == "default"     # failed candidates were among those compared
    assert not ok.all()


def test_key_of_the_second_reset(oracle):
    """the key the later resets sample with: one split per step()"""
    c = CASE['sizes-63']
    O = oracle.OracleEngine(c.cfg, n_candidates=c.M)
    O.reset(check=False)
    np.testing.assert_array_equal(O.get_state()['key'], c.key(0))
    for _ in range(ln.NUM_STEPS):
        O.step(np.zeros((ln.ENV_NUM, 2), f32))
        O.reset_done()
    np.testing.assert_array_equal(O.get_state()['key'], c.key(1))


# ---- the checker's pool ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES + [ln.SHARD_CASE], ids=repr)
def test_checker_pool_equals_sample_pool(oracle, case):
    """size, rows and order of the checker's pool after reset(); the layouts the reset hands the envs are
    pool[randint(key, env_num, L)]"""
    rows, ok = _pool(case.name)
    want = rows[ok]
    O = oracle.OracleEngine(case.cfg, n_candidates=case.M)
    O.reset(check=False)
    assert O.layout_size == len(want)
    got = O.get_pool()
    np.testing.assert_array_equal(got, want)
    if len(want):
        pick = want[onp.randint(case.key(0), ln.ENV_NUM, len(want))]
        st = O.get_state()
        np.testing.assert_array_equal(st['objs'], pick[:, :-1])
        np.testing.assert_array_equal(st['qpos'][:, :2], pick[:, -1])


def _steps(O, redrawn, key, pool):
    """num_steps zero-action steps with reset_done.  'redrawn': every step ends every episode, and reset_done hands
    every env pool[randint(key, env_num, L)] with the key of that step"""
    picks = set()
    for t in range(ln.NUM_STEPS):
        done = O.step(np.zeros((ln.ENV_NUM, 2), f32))[2]
        O.reset_done()
        assert done.all() == redrawn
        if redrawn:
            idx = onp.randint(ln.advance(key, t + 1), ln.ENV_NUM, len(pool))
            picks.update(idx.tolist())
            st = O.get_state()
            np.testing.assert_array_equal(st['objs'], pool[idx][:, :-1])
            np.testing.assert_array_equal(st['qpos'][:, :2], pool[idx][:, -1])
    return picks


@pytest.mark.parametrize("name", [c.name for c in CASES if c.name.startswith('sizes-')] + ['redrawn'])
def test_checker_pool_of_the_second_reset(oracle, name):
    """the same after num_steps steps: the pool of the second reset (the prefetched one on the device).  'redrawn':
    the reset_done draws after the first reset come from its one row, those after the second from both of its two"""
    c = CASE[name]
    rows, ok = _pool(name, 1)
    O = oracle.OracleEngine(c.cfg, n_candidates=c.M)
    O.reset(check=False)
    rows0, ok0 = _pool(name, 0)
    assert _steps(O, name == 'redrawn', c.key(0), rows0[ok0]) <= {0}
    O.reset(check=False)
    assert O.layout_size == int(ok.sum())
    np.testing.assert_array_equal(O.get_pool(), rows[ok])
    if name == 'redrawn':
        assert _steps(O, True, c.key(1), rows[ok]) == {0, 1}


# ---- what each case is there for ---------------------------------------------------------------------------------
def _far_corner_sq(case, goal):
    """squared distance from a goal to the farthest corner of the robot's rectangle (float64)"""
    rect, k = ln.placements(case.cfg)[-1]
    xmin, ymin, xmax, ymax = (float(v) for v in ln.bounds(rect, k))
    g = goal.astype(np.float64)
    fx = np.maximum(np.abs(xmin - g[:, 0]), np.abs(xmax - g[:, 0]))
    fy = np.maximum(np.abs(ymin - g[:, 1]), np.abs(ymax - g[:, 1]))
    return fx * fx + fy * fy


@pytest.mark.parametrize("case", CASES, ids=repr)
def test_case_condition(case):
    rows, ok = _pool(case.name)
    L, M, name = int(ok.sum()), case.M, case.name
    pool = rows[ok]
    print(f"{name}: M {M} L {L}, share failing all ten tries {ln.failed_all_tries(rows).mean():.4f}")
    if name.startswith('sizes-'):
        assert L >= 1 and int(_pool(name, 1)[1].sum()) >= 1
    elif name in ('span-1', 'one-candidate'):
        assert L == 1
    elif name == 'redrawn':
        assert L == 1 and int(_pool(name, 1)[1].sum()) == 2
    elif name == 'empty':
        assert L == 0
    elif name == 'easy':
        assert L >= 0.8 * M
    else:
        assert L >= case.min_L
    if name == 'dense':
        assert ln.failed_all_tries(rows).mean() >= 0.20
    if name == 'fixed':
        place = ln.placements(case.cfg)
        for o in (0, 1, 2):                    # the goal and the first two hazards
            xmin, ymin, xmax, ymax = ln.bounds(*place[o])
            if o in (0, 2):                    # (1.2, 1.1) and (-1, 0.5): the constrained rectangle is ONE float32 point
                assert xmin == xmax and ymin == ymax
                assert (pool[:, o] == np.array([xmin, ymin], f32)).all()
            else:                              # (0, 0): NOT constant.  x - (k + 1e-9) + k = -1e-9 survives the rounding to
                                               # float32 next to 0.0 (next to 1.2 it does not), so the rows move within it
                assert 0 < xmax == -xmin == ymax == -ymin < 1.1e-9
                assert (np.abs(pool[:, o]) <= xmax).all() and len(np.unique(pool[:, o], axis=0)) > 1
        assert len(np.unique(pool[:, 3], axis=0)) > 1
    if name == 'prune-corner':
        d = np.sqrt(((pool[:, -1].astype(np.float64) - pool[:, 0]) ** 2).sum(1))
        assert (d >= 3.0 - 1e-6).all() and (d < 3.001).all()
        assert (_far_corner_sq(case, rows[:, 0]) < 9.0 * 1.001).all()     # every candidate sits at the pruning edge
    if name == 'prune-strips':
        far = _far_corner_sq(case, rows[:, 0])          # every candidate's goal (all ten goal tries are valid)
        reject = far * 1.0001 < 9.0 * (1 - 1e-6)        # phase 0 may drop these: no robot position is 3.0 away
        keep = far >= 9.0                               # ... and must keep these
        assert reject.sum() >= 100 and keep.sum() >= 100
        assert keep[ok].all()


@pytest.mark.parametrize("case,n", SHARDED, ids=lambda v: repr(v))
def test_shard_split(case, n):
    """the candidate ranges of the shards: whole, in order -- and at M = 257 / 8 some shard holds no valid layout"""
    _, ok = _pool(case.name)
    ranges = ln.shard_ranges(case.M, n)
    assert ranges[0][0] == 0 and ranges[-1][1] == case.M and all(a[1] == b[0] for a, b in zip(ranges, ranges[1:]))
    counts = [int(ok[a:b].sum()) for a, b in ranges]
    print(case.name, n, "shards:", counts)
    assert sum(counts) == int(ok.sum()) >= 1
    if case.M == 257:
        assert min(counts) == 0 and case.M % n != 0
    else:
        assert min(counts) > 0 and case.M % n != 0


# ---- the comparison can fail ---------------------------------------------------------------------------------------
MISTAKES = [
    ('first_valid', ['sizes-4097', 'easy', 'hazards-2', 'fixed']),
    ('no_margin', ['margin', 'odd-thresholds']),
]


@pytest.mark.parametrize("mistake,name", [(m, n) for m, names in MISTAKES for n in names])
def test_planted_mistakes_change_the_pool(mistake, name):
    """the first valid try wins instead of the last / the margin is dropped: another pool"""
    rows, ok = _pool(name)
    bad_rows, bad_ok = _pool(name, 0, mistake)
    same = int(ok.sum()) == int(bad_ok.sum()) and np.array_equal(rows[ok], bad_rows[bad_ok])
    assert not same
    if mistake == 'no_margin':
        assert int(bad_ok.sum()) > int(ok.sum())      # smaller thresholds reject less
    else:
        changed = (rows[ok & bad_ok] != bad_rows[ok & bad_ok]).any(axis=(1, 2)).mean()
        print(f"{name}: {changed:.2%} of the rows valid either way differ")
        assert changed > 0.5
