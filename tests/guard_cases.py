"""Case sets and predicates for the rollout kernels' fast / exact step switch (tests/test_guard_cases.py on the CPU,
tests/test_gpu_guard_paths.py on the device).

Every rollout kernel has two forms of a step and picks one by a magnitude test:

  dyn_tape_kernel (Point, Swimmer)  steps with the unguarded forms first and checks AFTERWARDS whether the step was
      "ordinary"; if not it redoes the step exactly from the saved q, v and evaluates the NaN / Inf guard of the
      reference (engine.py:696-699) on a real observation row.  The terms, as the kernel writes them:
        cfg      the closeness cannot overflow: lidar_max_dist > 0, or lidar_exp_gain >= 0
        phys1    physics_steps_per_control_step == 1 (the two-kernel rollout is not used otherwise: constant here)
        objects  every object coordinate of the layout in effect is moderate, |x| < 1e18
        pose0    the stale pose's |cos| + |sin| is moderate
        start    the sum of |qpos|, |qvel| the step starts from is below 2^24 (sequential sum)
        stepped  the sum of |qpos|, |qvel| after the step and |action| is below 2^24 (summed as a tree)
        disp     displacement^2 of the returned pose against the stale one < 0.9
        goal     goal distance^2 < 1e8
      `goal reached` (distance < goal_size) and `timeout` (steps > num_steps) make a lane rare as well.  One rare lane
      sends its whole wave through the general branch.
  group_dyn_tape_kernel (Ant, Walker)  always steps exactly and evaluates the guard only when, for some lane of the
      wave, cfg / objects / start / stepped fails -- here with `moderate` (1e18) for both sums, both sequential.
  group_observe  switches the whole workgroup (four envs) from the integer scatter-max to the NaN-propagating
      sequential maxima when `lidar_bad` holds for any lane.

The predicates below restate those tests in numpy float32 from what the checker reports around a step.  They are NOT
a reference for values -- the checker and oracle/ref64.py are -- they exist so that a test can prove which side of
which test each planted row landed on.  `start` is evaluated on the state the step starts from; the kernel carries it
as a flag from the previous step's `stepped` (same sum without the action, in another order), which can differ only
where rounding decides, and the planted thresholds are made of one large term and zeros, where no order matters.
For a lane whose `start` fails the kernel's first, unguarded attempt is discarded, so `stepped` of the exact step is
what the predicate reports there too.

A start sum at or above its bound cannot fall below it in one step (moving a slide down by d costs a velocity of
d / h, fifty times d), so `start` is never the ONLY false term: the coverage conditions take it with `stepped`.

The case builder plants, per robot, non-finite and huge values in every kind of state entry and action, both sides of
every threshold (the nearest representable floats included, found by scanning the checker), rows that turn rare at a
later step and rows that turn ordinary again, into N = 67 envs x T = 19 steps: one full wave plus three lanes for the
thread-per-env kernels, a partial last wave at 4, 2 and 1 envs per wave for the lane-group ones; one whole block of
16 actions plus a block of three (the two-steps-per-trip loop's pairs, its odd tail, the LDS action buffer swap)."""
import functools

import numpy as np

from helpers import task_config, random_state, SWIMMER, ANT, WALKER
from test_ref64 import VARIANTS

f32 = np.float32
N, T, H = 67, 19, 8
N_CANDIDATES = 20000
NUM_STEPS = 1000
ROBOTS = ("point", "swimmer", "ant", "walker")
TAPE_ROBOTS = ("point", "swimmer")              # dyn_tape_kernel; the others: group_dyn_tape_kernel
EXTRA = {"point": {}, "swimmer": SWIMMER, "ant": ANT, "walker": WALKER}
ADIM = {"point": 2, "swimmer": 2, "ant": 8, "walker": 10}
# qpos index of the first slide, of the heading, and of the first / last joint
QIDX = {"point": dict(slide=0, heading=2, joints=()), "swimmer": dict(slide=0, heading=2, joints=(3, 4)),
        "ant": dict(slide=0, heading=1, joints=(3, 10)), "walker": dict(slide=0, heading=1, joints=(3, 12))}
# envs per wave of the kernels that take these robots (thread per env: 64, the Swimmer's quad form: 16; lane
# groups: 4, or 2 / 1 alone on the chip)
WAVES = {"point": (64,), "swimmer": (64, 16), "ant": (4, 2), "walker": (4, 2)}

TWO24 = f32(2.0 ** 24)
MOD = f32(1e18)
DISP = f32(0.9)
FAR = f32(1e8)

CONFIGS = {
    "default": {},
    "max_dist": dict(lidar_max_dist=3.0),
    "neg_gain": dict(lidar_exp_gain=-0.5),          # cfg false: every step of dyn_tape_kernel is the exact one
    "no_alias": dict(lidar_alias=False),
    "no_qpos": dict(VARIANTS[3]),                   # observe_qpos, observe_ctrl, observe_goal_lidar off
    "no_qpos_qvel": dict(VARIANTS[3], observe_qvel=False),
}
assert VARIANTS[3].get('observe_qpos') is False


def config(robot, name):
    return task_config(N, seed=7, num_steps=NUM_STEPS, **CONFIGS[name], **EXTRA[robot])


def below(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(0))
    return x


def above(x, k=1):
    x = f32(x)
    for _ in range(k):
        x = np.nextafter(x, f32(np.inf))
    return x


# ---- the predicates ------------------------------------------------------------------------------------------
def _seq_abs(*arrs):
    """sequential fp32 sum of the magnitudes of the columns, in order"""
    m = np.zeros(arrs[0].shape[0], f32)
    for a in arrs:
        for k in range(a.shape[1]):
            m = (m + np.abs(a[:, k])).astype(f32)
    return m


def _tree_abs(*arrs):
    """the same terms summed as dyn_tape_kernel's tree: term[k] += term[k + w] for w = 1, 2, 4, ..."""
    term = np.abs(np.concatenate(arrs, axis=1)).astype(f32)
    n = term.shape[1]
    w = 1
    while w < n:
        for k in range(0, n - w, 2 * w):
            term[:, k] = term[:, k] + term[:, k + w]
        w *= 2
    return term[:, 0].copy()


def cfg_ok(cfg):
    md = cfg.get('lidar_max_dist')
    return bool(md > 0) if md is not None else bool(-float(cfg.get('lidar_exp_gain', 1.0)) <= 0)


def step_terms(robot, cfg, pre, act, post):
    """(terms, values, extra): one boolean array per term of "was this step ordinary" for the robot's tape kernel --
    True: the term holds --, the fp32 value each threshold was compared with, and `goal_reached` and `timeout`.
    pre / post: the checker's state before and after the step (post['pose0'] is the pose the step returned)."""
    with np.errstate(all='ignore'):
        n = pre['qpos'].shape[0]
        q0, v0 = pre['qpos'].astype(f32), pre['qvel'].astype(f32)
        q1, v1, a = post['qpos'].astype(f32), post['qvel'].astype(f32), np.asarray(act, f32)
        objs = pre['objs'].astype(f32).reshape(n, -1)
        val = {}
        val['objects'] = np.abs(objs).max(axis=1)           # NaN propagates: the term is false then
        val['objects'] = np.where(np.isnan(objs).any(axis=1), f32(np.nan), val['objects'])
        full = np.ones(n, bool)
        terms = dict(cfg=full & cfg_ok(cfg),
                     phys1=full & (int(cfg.get('physics_steps_per_control_step', 1)) == 1),
                     objects=(np.abs(objs) < MOD).all(axis=1))
        gx, gy = pre['objs'][:, 0, 0].astype(f32), pre['objs'][:, 0, 1].astype(f32)
        px, py = post['pose0'][:, 0].astype(f32), post['pose0'][:, 1].astype(f32)
        gdx, gdy = gx - px, gy - py
        d2 = (gdx * gdx).astype(f32) + (gdy * gdy).astype(f32)
        if robot in TAPE_ROBOTS:
            val['pose0'] = (np.abs(pre['pose0'][:, 2]) + np.abs(pre['pose0'][:, 3])).astype(f32)
            terms['pose0'] = val['pose0'] < MOD
            val['start'] = _seq_abs(q0, v0)
            terms['start'] = val['start'] < TWO24
            val['stepped'] = _tree_abs(q1, v1, a)
            terms['stepped'] = val['stepped'] < TWO24
            mx, my = px - pre['pose0'][:, 0].astype(f32), py - pre['pose0'][:, 1].astype(f32)
            val['disp'] = (mx * mx).astype(f32) + (my * my).astype(f32)
            terms['disp'] = val['disp'] < DISP
            val['goal'] = d2
            terms['goal'] = d2 < FAR
        else:
            val['start'] = _seq_abs(q0, v0)
            terms['start'] = val['start'] < MOD
            val['stepped'] = _seq_abs(q1, v1, a)
            terms['stepped'] = val['stepped'] < MOD
        extra = dict(goal_reached=np.sqrt(d2).astype(f32) < f32(cfg.get('goal_size', 0.5)),
                     timeout=pre['steps'] > f32(cfg['num_steps']))
    return terms, val, extra


THRESHOLD = {"objects": MOD, "pose0": MOD, "disp": DISP, "goal": FAR}


def threshold(robot, term):
    if term in ("start", "stepped"):
        return TWO24 if robot in TAPE_ROBOTS else MOD
    return THRESHOLD[term]


def ordinary(terms):
    out = np.ones_like(terms['cfg'])
    for v in terms.values():
        out = out & v
    return out


def rare(robot, terms, extra):
    """lanes that send their wave through the general branch (tape kernels: a finished env does too)"""
    r = ~ordinary(terms)
    if robot in TAPE_ROBOTS:
        r = r | extra['goal_reached'] | extra['timeout']
    return r


def lidar_bad(cfg, pose, objs):
    """group_observe's switch, per env: a value that would land in a lidar row is non-finite.  fp32, the kernel's
    operation order; only whether a value is finite matters here, not its last bit."""
    with np.errstate(all='ignore'):
        pose, objs = pose.astype(f32), objs.astype(f32)
        dx = objs[:, :, 0] - pose[:, None, 0]
        dy = objs[:, :, 1] - pose[:, None, 1]
        c, s = pose[:, None, 2], pose[:, None, 3]
        zx = (dx * c).astype(f32) + (dy * s).astype(f32)
        zy = (dx * (-s)).astype(f32) + (dy * c).astype(f32)
        dist = np.sqrt(((zx * zx).astype(f32) + (zy * zy).astype(f32)).astype(f32))
        ang = np.arctan2(zy, zx).astype(f32)
        ang = np.where(ang < 0, ang + f32(2 * np.pi), ang)
        md = cfg.get('lidar_max_dist')
        if md is None:
            x = (f32(-float(cfg.get('lidar_exp_gain', 1.0))) * dist).astype(f32)
            sensor = np.where(x > 88, f32(np.inf), np.exp(np.minimum(x, f32(88))).astype(f32))
            sensor = np.where(np.isnan(x), x, sensor)
        else:
            gap = f32(md) - dist
            sensor = (np.where((gap < 0) & ~np.isnan(gap), f32(0), gap) / f32(md)).astype(f32)
        bins = int(cfg.get('lidar_num_bins', 16))
        bs = f32(2 * np.pi / bins)
        qn = ang / bs
        b = np.where(qn >= 0, np.minimum(np.floor(qn), bins), 0)
        alias = ((ang - bs * b.astype(f32)) / bs).astype(f32)
        bad = (b < bins) & ~np.isfinite(sensor)
        if cfg.get('lidar_alias', True):
            bad = bad | ~np.isfinite(alias * sensor) | ~np.isfinite((f32(1) - alias) * sensor)
        on = np.zeros(objs.shape[1], bool)
        on[0] = bool(cfg.get('observe_goal_lidar', True))
        on[1:] = bool(cfg.get('observe_hazards', True))
        return (bad & on[None]).any(axis=1)


# ---- running a case set on the checker -----------------------------------------------------------------------
def copy_state(s):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in s.items()}


def run_checker(O, s, acts):
    """the case set on an OracleEngine that was reset(): step + reset_done each step.  Returns the per-step records
    (pre, act, obs, rew, cost, done, post = the state after the step, rd = the reset_done observation) and the
    final state."""
    O.set_state(s)
    rows = []
    for t in range(acts.shape[0]):
        pre = O.get_state()
        o, r, d, info = O.step(acts[t])
        post = O.get_state()
        rd = O.reset_done()
        rows.append(dict(pre=pre, act=acts[t], obs=o, rew=r, cost=info['cost'], done=d, post=post, rd=rd))
    return rows, O.get_state()


@functools.lru_cache(maxsize=None)
def _scan_engine(robot):
    from oracle import gxo
    O = gxo.OracleEngine(config(robot, "default"), n_candidates=N_CANDIDATES)
    O.reset()
    return O


# ---- the case builder ------------------------------------------------------------------------------------------
VALUES = (("nan", np.nan), ("+inf", np.inf), ("-inf", -np.inf), ("3e38", 3e38), ("1e30", 1e30))
ACT_STEPS = (0, 15, 16, 18)
# planted rows sit at lane 0, lane 63, the last env, two adjacent envs of one lane group, and every third env between
SLOTS = [0, 63, 66, 5, 6] + list(range(9, 62, 3))


def _rest(s, i, robot, x=0.0):
    """env i at rest on the x axis, heading 0, the stale pose on the robot: an ordinary row whose sums of magnitudes
    are |x| alone.  The goal sits 16 to the right: its lidar reading, exp(-16), is below ref64's tolerance, so a
    position known to one ulp of 2^24 only (an angle ref64 counts as unknown) excludes nothing"""
    x = f32(x)
    s['qpos'][i] = 0
    s['qvel'][i] = 0
    s['qpos'][i, 0] = x
    s['pose0'][i] = (x, 0, 1, 0)
    s['pose1'][i] = (x, 0)
    s['steps'][i] = 3
    s['objs'][i, 0] = (x + f32(16), 3)


class _Set:
    def __init__(self, robot, seed):
        rng = np.random.default_rng(seed)
        self.robot = robot
        self.plain = random_state(N, H, rng, done_frac=0.0, robot=robot)
        self.plain['steps'][:] = rng.integers(0, 250, N)
        self.plain_acts = rng.uniform(-1, 1, (T, N, ADIM[robot])).astype(f32)
        self.state = copy_state(self.plain)
        self.acts = self.plain_acts.copy()
        self.names = {}
        self.free = list(SLOTS)

    def plant(self, name, fn, env=None):
        i = self.free.pop(0) if env is None else env
        assert i not in self.names, (i, name)
        fn(self.state, self.acts, i)
        self.names[i] = name
        return i

    @property
    def full(self):
        return not self.free

    def result(self, label):
        planted = np.zeros(N, bool)
        planted[list(self.names)] = True
        return dict(label=label, state=self.state, acts=self.acts, names=dict(self.names), planted=planted,
                    plain_state=self.plain, plain_acts=self.plain_acts)


def _value_plants(robot):
    ix = QIDX[robot]
    A = ADIM[robot]
    out = []

    def setter(field, *idx):
        def make(v):
            def fn(s, acts, i):
                s[field][(i,) + idx] = v
            return fn
        return make

    where = [("slide", setter('qpos', ix['slide'])), ("heading", setter('qpos', ix['heading']))]
    for k, j in enumerate(ix['joints']):
        where.append((("first", "last")[k] + " joint", setter('qpos', j)))
    where += [("velocity", setter('qvel', 0)), ("pose0 cos", setter('pose0', 2)), ("pose0 sin", setter('pose0', 3)),
              ("goal", setter('objs', 0, 0)), ("first hazard", setter('objs', 1, 1)), ("last hazard", setter('objs', H, 0))]
    for t in ACT_STEPS:
        for nm, d in (("first", 0), ("last", A - 1)):
            def make(v, t=t, d=d):
                def fn(s, acts, i):
                    acts[t, i, d] = v
                return fn
            where.append((f"{nm} action entry at t={t}", make))
    # value-major order: the plants of one location and step spread over the sets
    for wn, make in where:
        for vn, v in VALUES:
            out.append((f"{vn} in {wn}", make(f32(v))))
    return out


def _scan(gxo, robot, values, plant, term, t=0, steps=1):
    """the predicate's value of `term` at step t for every candidate value, one env each (at most N)"""
    values = np.asarray(values, f32)
    assert values.size <= N
    st = _Set(robot, 99)
    for i, v in enumerate(values):
        plant(f32(v))(st.state, st.acts, i)
    rows, _ = run_checker(_scan_engine(robot), st.state, st.acts[:steps])
    _, val, _ = step_terms(robot, config(robot, "default"), rows[t]['pre'], rows[t]['act'], rows[t]['post'])
    return val[term][:values.size]


def _pick(values, got, thr):
    """the candidates whose value lies within 2 ulp below the threshold, and at or within 2 ulp above it"""
    lo = [v for v, g in zip(values, got) if below(thr, 2) <= g < thr]
    hi = [v for v, g in zip(values, got) if thr <= g <= above(thr, 2)]
    assert lo and hi, (values, got, thr)
    return f32(lo[-1]), f32(hi[0])


def _threshold_plants(gxo, robot):
    """(name, fn) rows on both sides of every threshold of the robot's kernel"""
    ix = QIDX[robot]
    A = ADIM[robot]
    out = []

    def add(name, fn):
        out.append((name, fn))

    def obj(field_idx, v):
        def fn(s, acts, i):
            _rest(s, i, robot)
            s['objs'][(i,) + field_idx] = f32(v)
        return fn
    for nm, v in (("0.999e18", 0.999e18), ("1e18 - 1 ulp", below(MOD)), ("1e18", MOD), ("1.001e18", 1.001e18),
                  ("2e19", 2e19), ("-2e19", -2e19)):
        add(f"first hazard x at {nm}", obj((1, 0), v))
        add(f"last hazard y at {nm}", obj((H, 1), v))
    add("goal x at 1e18 - 1 ulp", obj((0, 0), below(MOD)))
    add("goal x at 1e18", obj((0, 0), MOD))

    if robot in TAPE_ROBOTS:
        def pose_cos(v):
            def fn(s, acts, i):
                _rest(s, i, robot)
                s['pose0'][i, 2] = f32(v)
                s['pose0'][i, 3] = 0
            return fn
        for nm, v in (("9e17", 9e17), ("1e18 - 1 ulp", below(MOD)), ("1e18", MOD), ("1.1e18", 1.1e18)):
            add(f"pose0 cos at {nm}", pose_cos(v))

        def start_x(v):
            def fn(s, acts, i):
                _rest(s, i, robot, v)
                acts[:, i] = 0
            return fn

        def start_th(v):
            def fn(s, acts, i):
                _rest(s, i, robot)
                s['qpos'][i, ix['heading']] = f32(v)
                acts[:, i] = 0
            return fn
        for nm, v in (("2^24 - 2", 2.0 ** 24 - 2), ("2^24 - 1", 2.0 ** 24 - 1), ("2^24", 2.0 ** 24),
                      ("2^24 + 2", 2.0 ** 24 + 2), ("2^25", 2.0 ** 25)):
            add(f"start sum through x at {nm}", start_x(v))
            add(f"start sum through the heading at {nm}", start_th(v))

        # start below 2^24, stepped sum + |action| at / above: the redo from the saved q, v
        def stepped(through, a):
            def fn(s, acts, i):
                (start_x if through == 'x' else start_th)(2.0 ** 24 - 50)(s, acts, i)
                acts[0, i, 0] = f32(a)
            return fn
        for through in ('x', 'heading'):
            cand = 40 + 0.25 * np.arange(N)
            got = _scan(gxo, robot, cand, lambda a, th=through: stepped(th, a), 'stepped')
            lo, hi = _pick(cand, got, TWO24)
            add(f"stepped sum through {through}: action {lo} just below 2^24", stepped(through, lo))
            add(f"stepped sum through {through}: action {hi} at 2^24", stepped(through, hi))
            add(f"stepped sum through {through}: action 60 above 2^24", stepped(through, 60))

        # displacement^2 around 0.9, at t = 0 through the stale pose ...
        def disp0(d):
            def fn(s, acts, i):
                _rest(s, i, robot)
                s['pose0'][i, 0] = -f32(d)
            return fn
        root = f32(np.sqrt(0.9))
        cand = np.array([above(root, k) if k >= 0 else below(root, -k) for k in range(-20, 21)], f32)
        got = _scan(gxo, robot, cand, disp0, 'disp')
        lo, hi = _pick(cand, got, DISP)
        add(f"stale pose {lo} behind: displacement^2 just below 0.9", disp0(lo))
        add(f"stale pose {hi} behind: displacement^2 at 0.9", disp0(hi))

        # ... and at t = 1 through a slide velocity found by bisection on the checker (grid refinement, N at a time)
        def disp1(vx):
            def fn(s, acts, i):
                _rest(s, i, robot)
                s['qvel'][i, 0] = f32(vx)
                acts[:, i] = 0
            return fn
        a_, b_ = f32(20), f32(80)
        for _ in range(4):
            cand = np.unique(np.linspace(a_, b_, N).astype(f32))
            got = _scan(gxo, robot, cand, disp1, 'disp', t=1, steps=2)
            k = int(np.argmax(got >= DISP))
            assert k > 0 and got[k - 1] < DISP, got
            a_, b_ = cand[k - 1], cand[k]
        add(f"slide velocity {a_}: displacement^2 below 0.9 at t = 1", disp1(a_))
        add(f"slide velocity {b_}: displacement^2 above 0.9 at t = 1", disp1(b_))

        def far_goal(gx):
            def fn(s, acts, i):
                _rest(s, i, robot)
                s['objs'][i, 0] = (f32(gx), 0)
                s['qvel'][i, :2] = (1.5, -0.7)   # moving: `last - dist` cancels at ulp(1e4) from t = 1 on
                acts[:, i] = 0
            return fn
        for nm, v in (("9999.5", 9999.5), ("10000 - 1 ulp", below(1e4)), ("10000", 1e4), ("10000.5", 10000.5)):
            add(f"far goal at {nm}", far_goal(v))

        # a velocity that carries the state over 2^24 at a later step (0.6 per step: no teleport, no displacement)
        def carried(s, acts, i):
            _rest(s, i, robot, 2.0 ** 24 - 33)
            s['qvel'][i, 0] = 30
            acts[:, i] = 0
        add("slide velocity 30 from x = 2^24 - 33: rare from a later step on", carried)
    else:
        def big_action(v, t, d):
            def fn(s, acts, i):
                acts[t, i, d] = f32(v)
            return fn
        for nm, v in (("1e18 - 1 ulp", below(MOD)), ("1e18", MOD), ("2e18", 2e18), ("-2e18", -2e18)):
            add(f"first action entry at {nm}, t = 0", big_action(v, 0, 0))
            add(f"last action entry at {nm}, t = 16", big_action(v, 16, A - 1))

        def start_x(v):
            def fn(s, acts, i):
                s['qpos'][i, ix['slide']] = f32(v)
            return fn
        for nm, v in (("1e18 - 1 ulp", below(MOD)), ("1e18", MOD), ("1.001e18", 1.001e18)):
            add(f"slide at {nm}", start_x(v))

        def carried(s, acts, i):
            s['qpos'][i, ix['slide']] = f32(0.99e18)
            s['qvel'][i, 0] = f32(1e17)          # 2e15 (0.5e16 for the Walker) per step
        add("slide 0.99e18 with velocity 1e17: over 1e18 at a later step", carried)

    def timeout(at):
        def fn(s, acts, i):
            s['steps'][i] = NUM_STEPS + 1 - at
        return fn
    add("timeout at t = 0", timeout(0))
    add("timeout at t = 15", timeout(15))
    add("timeout at t = 16", timeout(16))
    return out


def _solo_set(robot):
    """one planted lane in wave 0 at t = 15, one in the last wave at t = 16; whole waves rare at t = 3 and 4"""
    st = _Set(robot, 1000)
    # no goal within reach: the ordinary rows stay ordinary
    for s in (st.plain, st.state):
        d = s['objs'][:, 0] - s['pose0'][:, :2]
        near = np.hypot(d[:, 0], d[:, 1]) < 1.5
        s['objs'][near, 0] = s['pose0'][near, :2] + np.array([1.5, 0.5], f32)

    def act(t, v):
        def fn(s, acts, i):
            acts[t, i, 0] = f32(v)
        return fn
    st.plant("NaN action at t = 15, alone in its wave", act(15, np.nan), env=5)
    st.plant("3e38 action at t = 16, alone in the last wave", act(16, 3e38), env=66)
    for i in (64, 65):
        st.plant("NaN action at t = 3: the last wave all rare", act(3, np.nan), env=i)
    st.acts[3, 66, 0] = np.nan
    for i in (8, 9, 10, 11):
        st.plant("+inf action at t = 4: a lane-group wave all rare", act(4, np.inf), env=i)
    return st.result("solo")


@functools.lru_cache(maxsize=None)
def case_sets(robot):
    """the robot's case sets: dicts of label, state, acts (T, N, A), names {env: what was planted}, planted (N,) and
    the unplanted originals plain_state / plain_acts"""
    from oracle import gxo
    sets = []
    plants = _value_plants(robot)
    nsets = -(-len(plants) // len(SLOTS))
    group = [_Set(robot, 10 + k) for k in range(nsets)]
    for j, (name, fn) in enumerate(plants):
        group[j % nsets].plant(name, fn)
    sets += [g.result(f"values{k}") for k, g in enumerate(group)]
    plants = _threshold_plants(gxo, robot)
    nsets = -(-len(plants) // len(SLOTS))
    group = [_Set(robot, 50 + k) for k in range(nsets)]
    for j, (name, fn) in enumerate(plants):
        group[j % nsets].plant(name, fn)
    sets += [g.result(f"thresholds{k}") for k, g in enumerate(group)]
    sets.append(_solo_set(robot))
    return tuple(sets)


def tiled(cs, k):
    """the case set k times side by side, env_num = k * N (the later copies draw other layouts at a reset_done: the draw
    depends on the env index): for the forms a launcher only picks at a larger batch"""
    out = dict(cs, label=f"{cs['label']} x {k}")
    for key in ('state', 'plain_state'):
        out[key] = {f: (np.concatenate([v] * k, axis=0) if isinstance(v, np.ndarray) and f != 'key' else v)
                    for f, v in cs[key].items()}
    for key in ('acts', 'plain_acts'):
        out[key] = np.concatenate([cs[key]] * k, axis=1)
    out['planted'] = np.concatenate([cs['planted']] * k)
    return out


@functools.lru_cache(maxsize=None)
def checker_runs(robot, cname):
    """every case set of the robot on the checker under config `cname`: [(set, rows, final state)], computed once
    and shared (read-only) by the CPU and the device tests"""
    from oracle import gxo
    O = gxo.OracleEngine(config(robot, cname), n_candidates=N_CANDIDATES)
    O.reset()
    out = []
    for cs in case_sets(robot):
        rows, final = run_checker(O, cs['state'], cs['acts'])
        out.append((cs, rows, final))
    return out
