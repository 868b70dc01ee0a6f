"""The case sets of tests/guard_cases.py on the CPU checker: the NaN / Inf guard as the reference writes it
(engine.py:696-699), oracle/ref64.py on every finite row, the far-goal reward against float64 with a derived bound,
the coverage conditions that prove which side of which threshold the planted rows landed on, and three planted
mistakes of the kind the fast / exact step switch could make, each of which the same checks must catch.
tests/test_gpu_guard_paths.py runs the same sets on Engine."""
import numpy as np
import pytest

import guard_cases as gc
from oracle import ref64

f32 = np.float32
U = 2.0 ** -24
STATE_ROWS = ('qpos', 'qvel', 'pose0', 'pose1', 'objs', 'done0', 'done1', 'steps')


def finite_rows(robot, pre, act, obs, rew, cost, post):
    """rows whose inputs and outputs are all finite, and whose angles have a float64 meaning: beyond 2^24 the
    kernels' and the checker's sin / cos are DEFINED as those of 0 (gx_device.h sincos_f: x * 0), which a float64
    restatement of the model does not follow; such rows are compared with the checker bit for bit on the device and
    take part in the guard property, but not in ref64"""
    n = obs.shape[0]
    ok = np.ones(n, bool)
    with np.errstate(invalid='ignore'):
        for q in (pre['qpos'], post['qpos']):
            ang = np.delete(np.abs(q), [0, 1] if robot in gc.TAPE_ROBOTS else [0, 2], axis=1)
            ok &= (ang <= 2.0 ** 24).all(axis=1)
    for a in (pre['qpos'], pre['qvel'], pre['pose0'], pre['pose1'], pre['objs'], act, obs, rew, cost,
              post['qpos'], post['qvel'], post['pose0']):
        ok &= np.isfinite(np.asarray(a).reshape(n, -1)).all(axis=1)
    return ok


class FarGoal:
    """worst observed fraction of reward_bound, over all rows and over the rows with the goal >= 1000 away"""

    def __init__(self):
        self.worst = 0.0
        self.worst_far = 0.0
        self.far_rows = 0


def reward_bound(L, D, rd):
    """|reward_fp32 - reward_64| for reward = (last - dist) * reward_distance, both distances evaluated in fp32 from
    fp32 operands (goal, pose) as sqrt(dx * dx + dy * dy), u = 2^-24:
      dx = fl(gx - px) = (gx - px)(1 + e1), |e1| <= u; fl(dx * dx) carries (1 + u)^3; the sum of the two non-negative
      squares one more rounding: the radicand is exact to (1 + u)^4, its root to (1 + u)^2, and the correctly rounded
      square root adds one rounding: dist_fp32 = D (1 + e), |e| <= 3 u + O(u^2).  The same for `last` = L.
      The subtraction of the two fp32 distances rounds once, u |last - dist| <= u (1 + 6 u max(L, D)) (beyond
      |d_dist| = 1 the reward is 0), and the product with reward_distance once more.
    Sum: reward_distance * u * (3 (L + D) + 2), second-order terms covered by 3 -> 3.5.  Since ulp(dist) >= u * dist
    this is at most 7 ulp(max(L, D)) + 2 u: a small multiple of ulp(dist), 7e-3 at dist = 1e4 -- where ref64.check's
    fixed 1e-5 does not apply (tests pass such rows' reward to this bound instead)."""
    return rd * U * (3.5 * (L + D) + 2.0)


def check_reward64(C, pre, post, rew, rows, far, what):
    f = np.float64
    goal = pre['objs'][:, 0].astype(f)
    D = np.hypot(*(goal - post['pose0'][:, :2].astype(f)).T)
    L = np.where(pre['done0'] > 0, D, np.hypot(*(goal - pre['pose0'][:, :2].astype(f)).T)) if pre['hist'] >= 1 else D
    rd = float(C.c['reward_distance'])
    dd = L - D
    B = reward_bound(L, D, rd)
    want = np.where(np.abs(dd) > 1.0, 0.0, dd * rd)
    err = np.abs(rew.astype(f) - want)
    edge = np.abs(np.abs(dd) - 1.0) * rd <= B                  # either side of the teleport test
    err = np.where(edge, np.minimum(err, np.minimum(np.abs(rew.astype(f)), np.abs(rew.astype(f) - dd * rd))), err)
    sel = np.nonzero(rows)[0]
    if sel.size == 0:
        return
    frac = err[sel] / B[sel]
    far.worst = max(far.worst, float(frac.max()))
    isfar = np.maximum(L, D)[sel] >= 1000.0
    if isfar.any():
        far.worst_far = max(far.worst_far, float(frac[isfar].max()))
        far.far_rows += int(isfar.sum())
    assert (frac < 1.0).all(), f"{what}: reward {rew[sel][frac >= 1]} want {want[sel][frac >= 1]} bound {B[sel][frac >= 1]}"


def check_step(robot, C, pre, act, obs, rew, cost, done, post, tally, far, what):
    """one step's outputs (of the checker, of a planted subject or of Engine) against the reference's guard, ref64
    on the finite rows and the float64 reward"""
    bad = ~np.isfinite(obs).all(axis=1)
    # the guard as the reference writes it: done and a zero reward on every row with a non-finite observation entry;
    # the cost is left as computed.  (That no other row is ended is ref64's done comparison below.)
    assert (done[bad] == 1).all(), f"{what}: done on the non-finite rows {np.nonzero(bad & (done != 1))[0]}"
    assert (rew[bad] == 0).all(), f"{what}: reward on the non-finite rows {np.nonzero(bad & (rew != 0))[0]}"
    assert np.isin(done, (0.0, 1.0)).all()
    fin = finite_rows(robot, pre, act, obs, rew, cost, post)
    with np.errstate(all='ignore'):
        want = ref64.step(C, pre, act, post['qpos'], post['qvel'])
        assert not want['bad'][fin].any(), what
        # ref64.check's reward bound has no term that grows with the distance: rows with the goal far away get the
        # reference's own reward here (check has no switch to leave it out) and the derived bound below
        farrow = np.maximum(want['dist'], np.abs(want['dist'] + want['d_dist'])) >= 100.0
        r = np.where(farrow & fin, want['reward'], rew)
        # the same for the copied columns at huge magnitudes: qpos and qvel are copies (exact), ctrl is the action or
        # (Point) one fp32 product of the action and the stale pose's cos / sin: one rounding, u |x|, which passes
        # ref64's absolute 1e-5 from |x| = 168 on.  Such entries are compared here, relative, and handed on as the
        # reference's own value
        obs = obs.astype(np.float64)
        for key in ('qpos', 'qvel', 'ctrl'):
            if key in C.slices:
                g, w = obs[:, C.slices[key]], want['obs'][:, C.slices[key]]
                big = fin[:, None] & (np.abs(w) >= 64.0)
                tol = (1.5 * U if key == 'ctrl' else 0.0) * np.abs(w)
                assert (np.abs(g - w)[big] <= tol[big]).all(), f"{what}: {key} {g[big]} want {w[big]}"
                g[big] = w[big]
        ref64.check(C, dict(obs=obs, reward=r, done=done, cost=cost, steps=post['steps']), want, tally,
                    rows=np.nonzero(fin)[0], what=what)
        check_reward64(C, pre, post, rew, fin, far, what)
    return bad, fin


def check_after_reset_done(done, obs, rd, after, what):
    d = done > 0
    np.testing.assert_array_equal(rd[~d], obs[~d], err_msg=what)
    assert np.isfinite(rd[d]).all(), what
    for k in ('qpos', 'qvel', 'objs'):
        assert np.isfinite(after[k][d]).all(), f"{what}: {k} after reset_done"


# ---- the checker on every case set ---------------------------------------------------------------------------
@pytest.mark.parametrize("cname", list(gc.CONFIGS))
@pytest.mark.parametrize("robot", gc.ROBOTS)
def test_checker_guard_and_ref64(robot, cname):
    """done == 1 and reward == 0 on exactly the rows whose observation has a non-finite entry, the state after
    reset_done finite, ref64 on every all-finite row with the existing tests' exclusion cap, and the reward of every
    finite row -- the far goals among them -- within reward_bound of float64 (the worst fraction is printed)."""
    cfg = gc.config(robot, cname)
    C = ref64.Config(cfg)
    tally, far = ref64.Tally(), FarGoal()
    nbad = 0
    for cs, rows, final in gc.checker_runs(robot, cname):
        for t, rec in enumerate(rows):
            what = f"{robot} {cname} {cs['label']} t={t}"
            bad, fin = check_step(robot, C, rec['pre'], rec['act'], rec['obs'], rec['rew'], rec['cost'], rec['done'],
                                  rec['post'], tally, far, what)
            nbad += int(bad.sum())
            after = rows[t + 1]['pre'] if t + 1 < len(rows) else final
            check_after_reset_done(rec['done'], rec['obs'], rec['rd'], after, what)
    print(f"{robot} {cname}: {tally}, guarded rows {nbad}, far-goal rows {far.far_rows}; reward error / derived bound: "
          f"worst {far.worst:.3f}, worst with the goal >= 1000 away {far.worst_far:.3f}")
    assert tally.frac() < 0.01, tally
    assert nbad > 0
    if robot in gc.TAPE_ROBOTS and cname != "neg_gain":       # (exp(+5000): those rows are the guard's there)
        assert far.far_rows > 0 and far.worst_far > 0


def test_qvel_reaches_the_guard_only_when_observed():
    """a NaN velocity: with observe_qpos / observe_qvel on the guard sees it at t = 0; with both off (and no other
    entry that depends on it yet) it does not"""
    for robot in gc.ROBOTS:
        seen = {}
        for cname in ("default", "no_qpos_qvel"):
            hit = []
            for cs, rows, _ in gc.checker_runs(robot, cname):
                for i, name in cs['names'].items():
                    if name == "nan in velocity":
                        hit.append(bool(rows[0]['done'][i] == 1 and not np.isfinite(rows[0]['obs'][i]).all()))
            assert hit
            seen[cname] = hit
        assert all(seen["default"]) and not any(seen["no_qpos_qvel"]), (robot, seen)


# ---- coverage ----------------------------------------------------------------------------------------------
def _coverage(robot):
    tape = robot in gc.TAPE_ROBOTS
    thr_terms = ("objects", "pose0", "start", "stepped", "disp", "goal") if tape else ("objects", "start", "stepped")
    cov = dict(only={}, below={}, at={}, one_rare=set(), all_rare=set(), parity=set(), at_t=set(), redo=0,
               back_install=0, back_plain=0, back_goal=0, lidar_solo=0, sides={})
    for cname in gc.CONFIGS:
        cfg = gc.config(robot, cname)
        for cs, rows, _ in gc.checker_runs(robot, cname):
            prev_rare = prev_goal = None
            for t, rec in enumerate(rows):
                terms, val, extra = gc.step_terms(robot, cfg, rec['pre'], rec['act'], rec['post'])
                r = gc.rare(robot, terms, extra)
                # what the kernels' shortcut rests on, on the checker: an ordinary step has a finite observation, and
                # (tape kernels) ends the env exactly when the goal is reached or the time is up -- no teleport
                o = gc.ordinary(terms)
                assert np.isfinite(rec['obs'][o]).all(), (robot, cname, cs['label'], t)
                if tape:
                    np.testing.assert_array_equal(rec['done'][o] > 0, (extra['goal_reached'] | extra['timeout'])[o])
                    cov['back_goal'] += int((prev_goal & ~r).sum()) if prev_goal is not None else 0
                    prev_goal = o & extra['goal_reached']
                nfalse = sum((~v).astype(int) for v in terms.values())
                for k, v in terms.items():
                    only = ~v & (nfalse == 1)
                    if k == "start":            # never alone: see guard_cases
                        only = ~v & ~terms['stepped'] & (nfalse == 2)
                    cov['only'][k] = cov['only'].get(k, 0) + int(only.sum())
                    if k in thr_terms:
                        thr = gc.threshold(robot, k)
                        with np.errstate(invalid='ignore'):
                            lo = v & (val[k] >= gc.below(thr, 2)) & (val[k] < thr)
                            hi = only & (val[k] >= thr) & (val[k] <= gc.above(thr, 2))
                        cov['below'][k] = cov['below'].get(k, 0) + int(lo.sum())
                        cov['at'][k] = cov['at'].get(k, 0) + int(hi.sum())
                        for i in np.nonzero(lo | hi)[0]:
                            if i in cs['names']:
                                cov['sides'][(cs['names'][i], k)] = "below" if lo[i] else "at or above"
                for W in gc.WAVES[robot]:
                    for a in range(0, gc.N, W):
                        w = r[a:a + W]
                        if w.size > 1 and w.sum() == 1:
                            cov['one_rare'].add(W)
                        if w.size > 1 and w.all():
                            cov['all_rare'].add(W)
                if r.any():
                    cov['parity'].add(t % 2)
                    cov['at_t'].add(t)
                cov['redo'] += int((terms['start'] & ~terms['stepped']).sum())
                if prev_rare is not None:
                    back = prev_rare & ~r
                    cov['back_install'] += int((back & (rows[t - 1]['done'] > 0)).sum())
                    cov['back_plain'] += int((back & (rows[t - 1]['done'] == 0)).sum())
                prev_rare = r
                lb = gc.lidar_bad(cfg, rec['post']['pose0'], rec['pre']['objs'])
                lidar_cols = [sl for k, sl in ref64.Config(cfg).slices.items() if k.endswith('_lidar')]
                seen = ~np.isfinite(np.concatenate([rec['obs'][:, sl] for sl in lidar_cols], axis=1)).all(axis=1)
                np.testing.assert_array_equal(lb, seen, err_msg=f"lidar_bad {robot} {cname} {cs['label']} t={t}")
                for a in range(0, gc.N, 4):
                    if lb[a:a + 4].size > 1 and lb[a:a + 4].sum() == 1:
                        cov['lidar_solo'] += 1
    return cov, thr_terms


@pytest.mark.parametrize("robot", gc.ROBOTS)
def test_coverage(robot):
    """computed from the checker's records and the predicate alone; fails when the inputs drift off a threshold"""
    cov, thr_terms = _coverage(robot)
    print(robot, {k: v for k, v in cov.items() if k != 'sides'})
    for (name, k), side in sorted(cov['sides'].items()):
        print(f"  {k}: {side}: {name}")
    tape = robot in gc.TAPE_ROBOTS
    # every term is the only false one on some step (phys1 is constant: the two-kernel rollout is not used with more
    # than one physics step; start: together with stepped)
    for k in (("cfg",) + thr_terms):
        assert cov['only'].get(k, 0) > 0, f"{robot}: {k} is never the only false term"
    for k in thr_terms:
        assert cov['below'][k] > 0, f"{robot}: no step within 2 ulp below the threshold of {k}"
        assert cov['at'][k] > 0, f"{robot}: no step at the threshold of {k}"
    # the planted threshold rows landed on the side their names say
    for (name, k), side in cov['sides'].items():
        if "just below" in name or "- 1 ulp" in name:
            assert side == "below", (name, k, side)
    for W in gc.WAVES[robot]:
        assert W in cov['one_rare'], f"{robot}: no wave of {W} envs with exactly one rare lane"
        assert W in cov['all_rare'], f"{robot}: no wave of {W} envs with every lane rare"
    assert cov['parity'] == {0, 1}
    assert {15, 16} <= cov['at_t']
    assert cov['redo'] > 0
    assert cov['back_install'] > 0 and cov['back_plain'] > 0
    assert cov['lidar_solo'] > 0
    if tape:
        assert cov['back_goal'] > 0          # a goal-reached step (rare, every term true) with an ordinary one behind it


# ---- planted mistakes --------------------------------------------------------------------------------------
BUGS = {
    "guard_skipped": "the guard is skipped when the start state was below the bound (the step taken for ordinary)",
    "flags_stuck": "the flags are not restored after a re-initialisation: the env is treated as non-finite once more",
    "redo_from_stepped": "the exact redo starts from the already stepped q, v",
}


class Subject:
    """the checker with one mistake of the fast / exact switch planted"""

    def __init__(self, O, robot, cfg, bug):
        self.O, self.robot, self.cfg, self.bug = O, robot, cfg, bug
        self.stuck = np.zeros(O.N, bool)

    def _commit(self, post, rows, done, pre):
        post['done0'][rows] = done[rows]
        post['steps'][rows] = np.where(done[rows] > 0, 0, pre['steps'][rows] + 1)
        self.O.set_state(post)

    def step(self, act):
        O = self.O
        pre = O.get_state()
        o, r, d, info = O.step(act)
        c = info['cost']
        post = O.get_state()
        terms, _, extra = gc.step_terms(self.robot, self.cfg, pre, act, post)
        bad = ~np.isfinite(o).all(axis=1)
        if self.bug == "guard_skipped":
            rows = bad & terms['start']
            with np.errstate(all='ignore'):
                g = pre['objs'][:, 0]
                dg = np.sqrt(((g - post['pose0'][:, :2]) ** 2).sum(axis=1, dtype=f32))
                last = np.where(pre['done0'] > 0, dg, np.sqrt(((g - pre['pose0'][:, :2]) ** 2).sum(axis=1, dtype=f32)))
                dd = last - dg
                dn = ((dg < f32(self.cfg['goal_size'])) | (np.abs(dd) > 1) | extra['timeout']).astype(f32)
                rw = np.where(np.abs(dd) > 1, f32(0), dd * f32(self.cfg.get('reward_distance', 1.0))).astype(f32)
            d, r = np.where(rows, dn, d), np.where(rows, rw, r)
            self._commit(post, rows, d, pre)
        elif self.bug == "flags_stuck":
            rows = self.stuck
            d, r = np.where(rows, f32(1), d), np.where(rows, f32(0), r)
            self._commit(post, rows, d, pre)
            self.last_bad = bad
        elif self.bug == "redo_from_stepped":
            rows = terms['start'] & ~terms['stepped']
            if rows.any():
                s2 = gc.copy_state(pre)
                s2['qpos'][rows], s2['qvel'][rows] = post['qpos'][rows], post['qvel'][rows]
                O.set_state(s2)
                o2, r2, d2, i2 = O.step(act)
                post2 = O.get_state()
                o, r, d, c = (np.where(rows.reshape((-1,) + (1,) * (a.ndim - 1)), b, a)
                              for a, b in ((o, o2), (r, r2), (d, d2), (c, i2['cost'])))
                for k in STATE_ROWS:
                    post[k][rows] = post2[k][rows]
                O.set_state(post)
        self.bad = bad
        return o, r, d, c

    def reset_done(self):
        done = self.O.get_state()['done0'] > 0
        self.stuck = done & self.bad                     # re-initialised after a guarded step
        return self.O.reset_done()


def run_subject(robot, cname, bug):
    from oracle import gxo
    cfg = gc.config(robot, cname)
    C = ref64.Config(cfg)
    O = gxo.OracleEngine(cfg, n_candidates=gc.N_CANDIDATES)
    O.reset()
    tally, far = ref64.Tally(), FarGoal()
    for cs in gc.case_sets(robot):
        S = Subject(O, robot, cfg, bug)
        O.set_state(cs['state'])
        for t in range(gc.T):
            pre = O.get_state()
            o, r, d, c = S.step(cs['acts'][t])
            post = O.get_state()
            check_step(robot, C, pre, cs['acts'][t], o, r, c, d, post, tally, far, f"{bug} {cs['label']} t={t}")
            S.reset_done()
    assert tally.frac() < 0.01, tally


@pytest.mark.parametrize("robot", gc.ROBOTS)
def test_unplanted_subject_is_clean(robot):
    run_subject(robot, "default", None)


@pytest.mark.parametrize("bug", list(BUGS))
@pytest.mark.parametrize("robot", gc.ROBOTS)
def test_planted_mistake_is_caught(robot, bug):
    with pytest.raises(AssertionError) as e:
        run_subject(robot, "default", bug)
    print(f"{bug} on {robot}: {' '.join(str(e.value).split())[:200]}")
