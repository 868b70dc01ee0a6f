"""The layout sampler's WHOLE pool in numpy float32: a third statement of sample_layout / draw_placement
(oracle/gx_oracle_np.py:sample_layout is the scalar one), written for all M candidates at
once the way `jit(vmap(sample_layout))(split(key, M))` runs them.  TEST INFRASTRUCTURE ONLY; it imports neither the C
checker nor the HIP engine, so a pool it reproduces has been stated three times independently.

Per candidate j: key = split(PRNGKey(seed), M)[j]; the objects are placed in the order goal, hazards, pillars, robot;
each object gets ten tries `rng, rng1 = split(rng)`, `r1, r2 = split(rng1)`, x = uniform(r1, xmin, xmax),
y = uniform(r2, ymin, ymax) in its rectangle shrunk by its keepout; a try is valid when sqrt(sum(square(d))) to every
object placed so far is not below float32(keepout_other + margin + keepout); the LAST valid try wins, an object without
one fails the candidate (its row stays -inf), and so does robot-goal < 3.0.  The pool is rows[success], in candidate order.

`mistake=` builds a deliberately WRONG pool (tests/test_layout_np.py shows that the comparison can fail):
'first_valid' keeps the first valid try instead of the last, 'no_margin' drops placements_margin from the thresholds."""
import numpy as np

from helpers import task_config
from oracle import gx_oracle_np as onp

f32, U32 = np.float32, np.uint32

DEFAULTS = {
    'placements_extents': [-2, -2, 2, 2], 'placements_margin': 0.0, 'hazards_num': 8, 'pillars_num': 0,
    'goal_keepout': 0.5, 'hazards_keepout': 0.4, 'pillars_keepout': 0.3, 'robot_keepout': 0.4,
    'goal_placements': None, 'hazards_placements': None, 'pillars_placements': None, 'robot_placements': None,
    'goal_locations': [], 'hazards_locations': [], 'pillars_locations': [], 'robot_locations': [],
}
MIN_ROBOT_GOAL = 3.0
TRIES = 10


def placements(cfg):
    """[(rectangle (xmin, ymin, xmax, ymax) in Python floats, keepout)] in placement order: the i-th fixed location of a
    family is the square of half-width keepout + 1e-9 around it, otherwise the family's one *_placements rectangle,
    otherwise the arena"""
    c = {**DEFAULTS, **{k: v for k, v in cfg.items() if k in DEFAULTS}}
    out = []
    for stem, count in (('goal', 1), ('hazards', c['hazards_num']), ('pillars', c['pillars_num']), ('robot', 1)):
        keepout, fixed, rects = c[stem + '_keepout'], c[stem + '_locations'], c[stem + '_placements']
        for i in range(int(count)):
            if i < len(fixed):
                x, y = fixed[i]
                pad = keepout + 1e-9
                rect = (x - pad, y - pad, x + pad, y + pad)
            elif rects is not None:
                assert len(rects) == 1, "several rectangles per object are drawn with a host RNG the reference lacks"
                rect = tuple(rects[0])
            else:
                rect = tuple(c['placements_extents'])
            out.append((tuple(float(v) for v in rect), float(keepout)))
    return out


def bounds(rect, keepout):
    """constrain_placement: the rectangle shrunk by the keepout in Python floats, then what uniform() makes of it"""
    return f32(rect[0] + keepout), f32(rect[1] + keepout), f32(rect[2] - keepout), f32(rect[3] - keepout)


def margin(cfg):
    return float(cfg.get('placements_margin', DEFAULTS['placements_margin']))


def _split(k):
    """jax.random.split(k, 2) for a column of keys k (M, 2): threefry over the counters (0, 1 | 2, 3)"""
    z = np.zeros(k.shape[0], U32)
    a0, b0 = onp.threefry2x32(k[:, 0], k[:, 1], z, z + U32(2))
    a1, b1 = onp.threefry2x32(k[:, 0], k[:, 1], z + U32(1), z + U32(3))
    return np.stack([a0, a1], 1), np.stack([b0, b1], 1)


def _uniform(k, lo, hi):
    """jax.random.uniform(k, minval=lo, maxval=hi) per key: 23 mantissa bits -> [1, 2) - 1, scaled, clamped below"""
    z = np.zeros(k.shape[0], U32)
    bits, _ = onp.threefry2x32(k[:, 0], k[:, 1], z, z)
    u = ((bits >> U32(9)) | U32(0x3F800000)).view(f32) - f32(1.0)
    return np.maximum(lo, u * f32(hi - lo) + lo)


def advance(key, steps):
    """the engine's key after `steps` step() calls: key, _ = split(key) each"""
    key = np.asarray(key, U32)
    for _ in range(steps):
        key = onp.split(key, 2)[0]
    return key


def sample_pool(cfg, key, M, mistake=None, rows_of_failed=True):
    """(rows (M, K, 2) float32, success (M,) bool) of the M candidates of reset_layout(key).  A failed candidate is
    carried through every later object, as vmap does; rows_of_failed=False stops drawing for it once an object has
    failed all ten tries (its later rows stay -inf too), which changes neither `success` nor a successful row."""
    assert mistake in (None, 'first_valid', 'no_margin')
    place = placements(cfg)
    K = len(place)
    ko = [k for _, k in place]
    mg = 0.0 if mistake == 'no_margin' else margin(cfg)
    rng = onp.split(np.asarray(key, U32), M).astype(U32)
    rows = np.full((M, K, 2), -np.inf, f32)
    success = np.ones(M, bool)
    idx = np.arange(M)                      # the candidates still drawn for
    with np.errstate(invalid='ignore'):     # (-inf) - (-inf) of a failed candidate's robot and goal
        for o, (rect, k) in enumerate(place):
            xmin, ymin, xmax, ymax = bounds(rect, k)
            thr = np.array([f32(ko[q] + mg + k) for q in range(o)], f32)
            before = rows[idx, :o]
            xy = np.full((len(idx), 2), -np.inf, f32)
            placed = np.zeros(len(idx), bool)
            for _ in range(TRIES):
                rng, rng1 = _split(rng)
                r1, r2 = _split(rng1)
                cur = np.stack([_uniform(r1, xmin, xmax), _uniform(r2, ymin, ymax)], 1)
                dist = np.sqrt(np.sum(np.square(cur[:, None, :] - before), axis=2, dtype=f32), dtype=f32)
                ok = ~(dist < thr).any(axis=1)
                if mistake == 'first_valid':
                    ok &= ~placed
                xy[ok] = cur[ok]
                placed |= ok
            rows[idx, o] = xy
            success[idx] &= placed
            if not rows_of_failed:
                idx, rng = idx[placed], rng[placed]
        d = rows[:, K - 1] - rows[:, 0]
        dist = np.sqrt(np.sum(np.square(d), axis=1, dtype=f32), dtype=f32)
        success &= ~(dist < f32(MIN_ROBOT_GOAL))
    return rows, success


def failed_all_tries(rows):
    """candidates with an object none of whose ten tries was valid"""
    return np.isinf(rows[:, :, 0]).any(axis=1)


def shard_ranges(M, n_shards):
    """candidates [M s / n, M (s + 1) / n) of shard s, as Engine.sample_shard documents"""
    return [(M * s // n_shards, M * (s + 1) // n_shards) for s in range(n_shards)]


# ---------------------------------------------------------------------------------------------------------------
# the arenas shared by tests/test_layout_np.py (CPU: this file against the checker) and tests/test_gpu_layout_sampler.py
# (HIP against the checker).  L = the pool size measured with sample_pool on the first / second reset (the second
# reset's key is the first advanced by num_steps = 3 steps); they are records, the tests assert the conditions.
# ---------------------------------------------------------------------------------------------------------------
ENV_NUM, NUM_STEPS = 5, 3
EASY = dict(hazards_num=1, hazards_keepout=0.1, goal_keepout=0.1, robot_keepout=0.1, placements_extents=[-8, -8, 8, 8])


class Case:
    def __init__(self, name, M, seed, over, min_L=10, resets=2):
        self.name, self.M, self.seed, self.over, self.min_L, self.resets = name, M, seed, over, min_L, resets

    @property
    def cfg(self):
        return task_config(ENV_NUM, seed=self.seed, num_steps=NUM_STEPS, **self.over)

    @property
    def n_tape_objects(self):
        """hazards + pillars: 8 is the object count with a key tape"""
        return self.cfg['hazards_num'] + self.cfg.get('pillars_num', 0)

    def key(self, reset):
        return advance([0, self.seed], NUM_STEPS * reset)

    def __repr__(self):
        return self.name


CASES = [Case(f'sizes-{M}', M, 0, {}, min_L=1) for M in (63, 64, 65, 255, 256, 257, 4095, 4096, 4097)]
# L: 3 / 3, 3 / 2, 3 / 1, 5 / 4, 4 / 2, 4 / 3, 83 / 97, 78 / 83, 73 / 63              (first / second reset)
CASES += [
    Case('span-1', 2, 5, {}, min_L=1),                                                           # L 1 / 0
    Case('one-candidate', 1, 0, EASY, min_L=1),                                                  # L 1 / 0
    Case('empty', 1, 0, {}, min_L=0, resets=1),                                                  # L 0
    # goal_size 6 ends every episode at every step: the reset_done calls after the first reset draw every env's layout
    # from its pool of one row, those after the second reset from its pool of two (both rows are drawn)
    Case('redrawn', 40, 4, dict(goal_size=6.0), min_L=1),                                        # L 1 / 2
    Case('easy', 8193, 3, EASY),                                                                 # L 7414 / 7435
    Case('dense', 150_000, 3, dict(hazards_keepout=0.47)),                                       # L 146 / 118; 99 % of the candidates have an object failing all ten tries
    Case('margin', 60_000, 3, dict(placements_margin=0.15)),                                     # L 44 / 35
    Case('odd-thresholds', 40_000, 3, dict(hazards_keepout=0.37, goal_keepout=0.61, robot_keepout=0.23,
                                           placements_margin=0.013)),                            # L 1754 / 1834
    Case('asymmetric', 40_000, 3, dict(placements_extents=[-3.5, -1.25, 2.0, 2.75])),            # L 7726 / 7624
    Case('objects-7', 60_000, 3, dict(hazards_num=7)),                                           # L 2056 / 2107
    Case('objects-9', 60_000, 3, dict(hazards_num=9)),                                           # L 486 / 495
    Case('hazards-1', 20_000, 3, dict(hazards_num=1)),                                           # L 960 / 893
    Case('hazards-2', 20_000, 3, dict(hazards_num=2)),                                           # L 956 / 961
    Case('hazards-16', 60_000, 3, dict(hazards_num=16, hazards_keepout=0.3)),                    # L 122 / 125
    # L 13043 / 13136 and 12985 / 13054
    Case('lds-23-objects', 20_000, 3, dict(hazards_num=21, hazards_keepout=0.2, placements_extents=[-4, -4, 4, 4])),
    Case('lds-24-objects', 20_000, 3, dict(hazards_num=22, hazards_keepout=0.2, placements_extents=[-4, -4, 4, 4])),
    Case('pillars', 30_000, 3, dict(hazards_num=6, pillars_num=5, pillars_keepout=0.3, observe_pillars=True,
                                    placements_extents=[-3, -3, 3, 3])),                          # L 13040 / 13064
    Case('fixed', 20_000, 3, dict(goal_locations=[(1.2, 1.1)], hazards_locations=[(0.0, 0.0), (-1.0, 0.5)])),   # L 721 / 676
    # ('fixed': the rows of the goal and of the hazard at (-1, 0.5) are constant across the pool; the hazard at (0, 0) keeps
    # a rectangle of +-1e-9 in float32 and moves within it -- tests/test_layout_np.py asserts exactly that)
    Case('rectangles', 20_000, 3, dict(robot_placements=[(-2, -2, -1, -1)], goal_placements=[(0.5, 0.5, 2, 2)])),   # L 4185 / 4138
    Case('prune-corner', 60_000, 3, dict(goal_locations=[(-1.5, 0.0)], robot_placements=[(1.0, -0.45, 1.9, 0.45)],
                                         hazards_num=2)),                                        # L 62 / 64
    Case('prune-strips', 60_000, 3, dict(goal_placements=[(-2.0, -0.6, -0.9, 0.6)],
                                         robot_placements=[(1.0, -0.5, 1.9, 0.5)], hazards_num=2), min_L=3),          # L 6 / 3
]
# the sharded form: (arena, shards).  The first must hold a shard that exports nothing.
SHARD_CASE = Case('shards-20011', 20_011, 3, {})                                                 # L 367
CASE = {c.name: c for c in CASES + [SHARD_CASE]}
SHARDED = [(CASE['sizes-257'], 8), (SHARD_CASE, 7)]
