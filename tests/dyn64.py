"""dyn64.py -- the float64 expectation of what one control step does to qpos / qvel, env by env, from the
independent robot models: oracle/ant_np.py (TreeModel.step, Ant and Walker through oracle/walker_np.py),
oracle/gx_oracle_np.swimmer_step, and for the Point the few lines of gx_oracle_np.point_substep restated in
float64 (that function rounds its trigonometry and its results to fp32).  None of these is the C checker or
shares code with it or with the kernels, and this module does not import the checker's binding.

expect(cfg, state, actions) -> dict(qpos2, qvel2, pose0), float64, where `state` is the dict of get_state() /
helpers.random_state and pose0 is (x, y, cos, sin) of the robot body after the step:
  * physics_steps_per_control_step = k runs k model steps with the same ctrl; pose0 is the pose of the qpos
    before the last integration (oracle/ref64.py, module docstring), turned by robot_rot (the root body's quat);
    check() compares a k > 1 pose0 with the pose of that qpos as the step's own results give it (expected_pose0);
  * ctrl: the Point's action is rotated by the heading the state holds in pose0 (convert_action reads the data
    before the step); the other robots take the raw action.  Every model clips ctrl for the force only.

Single model steps are cached by content (robot, q, v, ctrl): a state set costs its ~10 ms per env once, whatever
the kernel path, batch-size prefix or dynamics-neutral config variant it is run through afterwards.
"""
import numpy as np

from oracle import ref64, gx_oracle_np as onp

f64 = np.float64

# ---- bounds: those the project applies between the C checker and these models ------------------------------
TREE_BOUND = {'ant': 2e-3, 'walker': 3e-3}     # max|d| < b (1 + max|ref|): test_oracle_ant.py:81-83, test_oracle_walker.py:67-69
SWIMMER_TOL = {'qpos': (2e-5, 2e-5), 'qvel': (2e-4, 1e-4)}      # (rtol, atol) of test_oracle_swimmer.py:65-66
# Point: test_point_solve_single_step_error_against_float64 bounds one step from a common state by
# 2e-6 max(1, max|ref|), taken over its batch; here it is applied env by env.  That test feeds the float64 solve
# the checker's own fp32 forces; here the forces are float64 too, and the bound still transfers to the full step:
# the C checker's worst error on the Point state sets of test_dyn64.py is 0.80 of it (random, N = 192) and 0.38
# (directed).
# Two physics steps per control step: the bound does not transfer to the hinge's velocity.  Inside its force limit
# the velocity servo gives d qvel' / d qvel = 1 - h gear^2 kv / (Ic + h d) = -13.2 at h = 0.02 (it is unstable
# there), so the second substep multiplies the first one's last-bit error; the slides
# contract, and qpos takes h times the velocity's error.  For that one component the bound is therefore measured:
# the C checker against this module on the Point's state sets at k = 2 (test_dyn64.py::test_point_two_substeps:
# random N = 192, the directed states, three chained steps) is off by 9.46e-6 max(1, max|ref|) at worst, and the
# bound is twice that; the margin of 2 covers another seed.  Every other component keeps 2e-6 at k = 2 (worst
# measured there 1.4e-7).  No other k has been measured: it is refused.
POINT_BOUND = 2e-6
POINT_HINGE_VEL_BOUND_K2 = 2 * 9.46e-6
POSE_ATOL = {'point': 2e-6, 'swimmer': 1e-6, 'ant': 2e-6, 'walker': 2e-6}   # test_oracle_{ant,walker}.py, test_oracle_swimmer.py:67

_MODELS = {}
_CACHE = {}


def model(robot):
    """the float64 tree model of 'ant' / 'walker' (built once)"""
    if robot not in _MODELS:
        if robot == 'ant':
            from oracle.ant_np import AntModel as M
        else:
            from oracle.walker_np import WalkerModel as M
        _MODELS[robot] = M()
    return _MODELS[robot]


# point.xml: timestep :3, joint damping :16-18, gear :37-39; mass, first moment and inertia about the joint
# origin of sphere + box at density 1 (:5,19-20), actuator defaults :7-8 -- the float64 constants of gx_oracle_np
_PT_H, _PT_DAMP, _PT_GEAR = 0.02, np.array([0.01, 0.01, 0.005]), 0.3


def point_step64(q, v, ctrl):
    """gx_oracle_np.point_substep for one env, float64 throughout: (pose at the start state, q', v')"""
    c, s = np.cos(q[2]), np.sin(q[2])
    M = np.array([[onp.M, 0.0, -onp.MXC * s], [0.0, onp.M, onp.MXC * c], [-onp.MXC * s, onp.MXC * c, onp.IO]])
    w2 = v[2] * v[2]
    bias = np.array([-onp.MXC * c * w2, -onp.MXC * s * w2, 0.0])
    u = np.clip(ctrl, -onp.CTRL_LIM, onp.CTRL_LIM)
    act = _PT_GEAR * np.clip(u - onp.KV * (_PT_GEAR * v), -onp.FORCE_LIM, onp.FORCE_LIM)
    f = -_PT_DAMP * v - bias + act
    qa = np.linalg.solve(M + np.diag(_PT_H * _PT_DAMP), f)
    v2 = v + _PT_H * qa
    q2 = q + _PT_H * v2
    return np.array([q[0], q[1], c, s]), q2, v2


def _one(robot, q, v, ctrl):
    """one model step of one env, cached by content: (pose (x, y, cos, sin) at the start state, q', v')"""
    key = (robot, q.tobytes(), v.tobytes(), ctrl.tobytes())
    out = _CACHE.get(key)
    if out is None:
        if robot == 'point':
            out = point_step64(q, v, ctrl)
        elif robot == 'swimmer':
            pose, _, q2, v2 = onp.swimmer_step(q, v, ctrl)
            out = (pose, q2, v2)
        else:
            pose, _, q2, v2 = model(robot).step(q, v, ctrl)
            out = (pose, q2, v2)
        _CACHE[key] = out
    return out


def expect(cfg, state, actions):
    """float64 expectation of one control step of config `cfg` from `state` under `actions` (n, act_dim)"""
    C = ref64.Config(cfg)
    q0 = np.asarray(state['qpos'], f64)
    v0 = np.asarray(state['qvel'], f64)
    act = np.asarray(actions, f64)
    n = q0.shape[0]
    assert q0.shape == (n, C.nq) and v0.shape == (n, C.nv) and act.shape[0] == n
    if C.robot == 'point':
        p0 = np.asarray(state['pose0'], f64)
        ctrl = np.stack([act[:, 0] * p0[:, 2], act[:, 0] * p0[:, 3], act[:, 1]], axis=1)
    else:
        ctrl = act
    qpos2, qvel2, pose = np.empty((n, C.nq)), np.empty((n, C.nv)), np.empty((n, 4))
    for i in range(n):
        q, v, u = q0[i].copy(), v0[i].copy(), np.ascontiguousarray(ctrl[i])
        for _ in range(C.k):
            pose[i], q, v = _one(C.robot, q, v, u)
        qpos2[i], qvel2[i] = q, v
    if C.rot:
        cr, sr = np.cos(C.rot), np.sin(C.rot)
        x, y, c, s = pose.T
        pose = np.stack([cr * x - sr * y, sr * x + cr * y, cr * c - sr * s, sr * c + cr * s], axis=1)
    return dict(qpos2=qpos2, qvel2=qvel2, pose0=pose)


def rows_count(robot, state):
    """(limit rows, contact rows) the float64 tree model finds active over the states of an Ant / Walker set"""
    m = model(robot)
    nlim = ncon = 0
    for q, v in zip(np.asarray(state['qpos'], f64), np.asarray(state['qvel'], f64)):
        for r in m.rows(q, v):
            if np.count_nonzero(r[0]) == 1:
                nlim += 1
            else:
                ncon += 1
    return nlim, ncon


# ---- comparison --------------------------------------------------------------------------------------------
class Worst:
    """worst error seen per quantity, normalised max|d| / (1 + max|ref|) per env (pose0: absolute)"""

    def __init__(self):
        self.qpos = self.qvel = self.pose0 = self.frac = 0.0
        self.envs = 0

    def __repr__(self):
        return (f"worst qpos {self.qpos:.2e} qvel {self.qvel:.2e} pose0 {self.pose0:.2e}, {self.frac:.3f} of the "
                f"bound at most, over {self.envs} env-steps")


def norm_err(got, want):
    """per env: max|got - want| / (1 + max|want|)"""
    got, want = np.asarray(got, f64), np.asarray(want, f64)
    return np.abs(got - want).max(axis=1) / (1.0 + np.abs(want).max(axis=1))


def tolerance(C, name, w):
    """allowed |got - want| of qpos / qvel (`name`) for expectations w (n, nq), broadcastable to w's shape"""
    wmax = np.abs(w).max(axis=1, initial=0.0)[:, None]
    if C.robot in TREE_BOUND:
        return TREE_BOUND[C.robot] * (1.0 + wmax)
    if C.robot == 'swimmer':
        rtol, atol = SWIMMER_TOL[name]
        return atol + rtol * np.abs(w)
    if C.k not in (1, 2):
        raise NotImplementedError("the Point's bound is known for one and two physics steps per control step")
    b = np.full(3, POINT_BOUND)
    if C.k == 2 and name == 'qvel':
        b[2] = POINT_HINGE_VEL_BOUND_K2
    return b * np.maximum(1.0, wmax)


U32 = 2.0 ** -24          # unit roundoff of fp32


def expected_pose0(C, want, qpos, qvel):
    """(pose0 (n, 4), allowed |got - pose0| (n,)) after a step whose fp32 results are qpos / qvel.
    One physics step: the pose of the fp32 qpos the step started from, which the model returns, under the files'
    atol.  More: the pose of the qpos q' before the last integration.  The model's q' differs from the kernel's by
    the dynamics error of the substeps before (measured against it: 4.6e-5 for the Ant, 1.8e-6 for the Point at
    k = 2), which would drown a pose taken from the wrong substep's qpos (h v ~ 1e-2).  The step's own results
    give q' without it: Euler integrates slides and hinges as q = fl(q' + fl(h v)), so q' = q - h v up to
    u (|q| + h |v|) per coordinate, u = 2^-24.  The pose (x - sin(th) y, cos(th) y, cos(th), sin(th)) of the Ant /
    Walker base (x, y, th for the other two) moves by at most (1 + |y|) times that, and by sqrt 2 more per component
    where robot_rot mixes x and y.  The atol is kept on top."""
    if C.k == 1:
        return want['pose0'], np.full(want['pose0'].shape[0], POSE_ATOL[C.robot])
    q, v = np.asarray(qpos, f64), np.asarray(qvel, f64)
    pose = ref64.robot_pose(C, q - C.h * v)
    e = U32 * (np.abs(q[:, :3]).max(axis=1) + C.h * np.abs(v[:, :3]).max(axis=1))
    if C.robot in TREE_BOUND:
        e = e * (1.0 + np.abs(q[:, 2]))
    if C.rot:
        e = e * np.sqrt(2.0)
    return pose, POSE_ATOL[C.robot] + e


def check(cfg, want, qpos=None, qvel=None, pose0=None, rows=None, worst=None, what=""):
    """fp32 results (n, ..) of a step of config `cfg` against expect()'s `want` under the robot's bounds, on `rows`
    (default: every env).  Raises AssertionError naming the worst env."""
    C = ref64.Config(cfg)
    robot = C.robot
    n = want['qpos2'].shape[0]
    rows = np.arange(n) if rows is None else np.asarray(rows)
    worst = worst if worst is not None else Worst()
    worst.envs += rows.size
    for name, got in (('qpos', qpos), ('qvel', qvel)):
        if got is None:
            continue
        g, w = np.asarray(got, f64)[rows], want[name + '2'][rows]
        assert np.isfinite(g).all() and np.isfinite(w).all(), f"{what}: {name} not finite"
        setattr(worst, name, max(getattr(worst, name), norm_err(g, w).max(initial=0.0)))
        ratio = (np.abs(g - w) / tolerance(C, name, w)).max(axis=1, initial=0.0)
        worst.frac = max(worst.frac, ratio.max(initial=0.0))
        if (ratio >= 1.0).any():
            i = int(np.argmax(ratio))
            raise AssertionError(f"{what}: {robot} {name} of env {rows[i]} is {ratio[i]:.3g} x its bound "
                                 f"({int((ratio >= 1).sum())} envs beyond it): got {g[i]}, want {w[i]}")
    if pose0 is not None:
        w, tol = expected_pose0(C, want, qpos, qvel)
        g, w = np.asarray(pose0, f64)[rows], w[rows]
        d = np.abs(g - w).max(axis=1, initial=0.0)
        worst.pose0 = max(worst.pose0, d.max(initial=0.0))
        ratio = d / tol[rows]
        worst.frac = max(worst.frac, ratio.max(initial=0.0))
        if (ratio >= 1.0).any():
            i = int(np.argmax(ratio))
            raise AssertionError(f"{what}: {robot} pose0 of env {rows[i]} off by {d[i]:.3g}, {ratio[i]:.3g} x its "
                                 f"bound: got {g[i]}, want {w[i]}")
    return worst
