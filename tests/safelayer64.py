"""safelayer64.py -- TEST INFRASTRUCTURE ONLY: the safety layer's action correction (Dalal et al. 2018) restated twice.

Restated from the reference learner (safe_rl_libX/safelayer/safelayer_core.py:169-190, C_Critic.safety_correction):
    pred = g.a + prev_c
    pred <= delta:  a_safe = a
    pred >  delta:  mult = relu((g.a + prev_c - delta) / (g.g + 1e-8));  a_safe = clamp(a - mult g, -1, 1)
with the per-component multiplier in the general form mult[:, None] * g (the reference's cat((mult, mult)) is this for
act_dim = 2).

  * correction32: numpy float32 in the operation order include/guardx_safelayer.h fixes -- the kernel must give these bits.
  * correction64: float64, with a bound on how far a correct fp32 evaluation in that order may lie from it, given
    bounds on its inputs g and a.  The networks (mu, val, logp, g) and their bounds come from oracle.policy64.

The bound of a_safe[k], from policy64's constants (U = 2^-24, gamma(n), MARGIN), for inputs g +- dg, a +- da (prev_c and
delta are fp32 values the kernel reads exactly):
    ga = sum g_k a_k:   d_ga = sum (|g_k| da_k + |a_k| dg_k + da_k dg_k) + gamma(A) sum (|g_k| + dg_k)(|a_k| + da_k)
                        (term k passes through one product and at most A - 1 sums: A roundings)
    gg = sum g_k^2:     d_gg = sum (2 |g_k| dg_k + dg_k^2) + gamma(A) sum (|g_k| + dg_k)^2
    pred = ga + prev_c: d_pred = d_ga + U (|pred| + d_ga)
  uncorrected branch:   a_safe = a, bound da_k
  corrected branch:
    numer = pred - delta:   d_numer = d_pred + U (|numer| + d_pred)
    denom = gg + 1e-8:      d_denom = d_gg + |1e-8 - fl32(1e-8)| + U (denom + d_gg)
    q = numer / denom:      d_q = (d_numer + |q| d_denom) / (denom - d_denom) + one rounding U (|q| + ...)
                            (denom <= d_denom: unbounded; see the cap below); relu is 1-Lipschitz
    p_k = mult g_k:         d_p = mult dg_k + |g_k| d_q + d_q dg_k + U (mult + d_q)(|g_k| + dg_k)
    x_k = a_k - p_k:        d_x = da_k + d_p + U (|x_k| + da_k + d_p); the clamp is 1-Lipschitz
    bound = MARGIN d_x, never above 2: both evaluations end in [-1, 1], so no element needs to be set aside for size.
A row whose |pred - delta| <= d_pred may take either branch in a correct fp32 evaluation: `edge` marks it and both
branches' values and bounds are returned.
"""
import numpy as np

from oracle import policy64

F32_EPS = float(np.float32(1e-8))


def correction32(g, a, prev_c, delta=0.0):
    """the kernel's correction in numpy float32, operation for operation (include/guardx_safelayer.h); g, a (..., A),
    prev_c (...)"""
    f = np.float32
    g, a, prev_c, delta = np.asarray(g, f), np.asarray(a, f), np.asarray(prev_c, f), f(delta)
    A = g.shape[-1]
    with np.errstate(all='ignore'):
        ga = g[..., 0] * a[..., 0]
        gg = g[..., 0] * g[..., 0]
        for k in range(1, A):
            ga = ga + g[..., k] * a[..., k]
            gg = gg + g[..., k] * g[..., k]
        pred = ga + prev_c
        numer = pred - delta
        denom = gg + f(1e-8)
        mult = numer / denom
        mult = np.where(mult > 0, mult, f(0))
        x = a - mult[..., None] * g
        x = np.where(x < -1, f(-1), x)
        x = np.where(x > 1, f(1), x)
    assert x.dtype == f and pred.dtype == f
    return np.where((pred <= delta)[..., None], a, x), pred


def correction64(g, dg, a, da, prev_c, delta=0.0):
    """float64 restatement and bounds (module docstring).  Returns a dict: a_safe, a_safe_b (the branch the float64 pred
    takes), pred, pred_b, corrected (bool rows), edge (bool rows), other, other_b (the other branch's value and bound)"""
    U, gm, MG = policy64.U, policy64.gamma, policy64.MARGIN
    g, dg, a, da = (np.asarray(x, np.float64) for x in (g, dg, a, da))
    prev_c = np.asarray(prev_c, np.float64)
    delta = float(np.float32(delta))
    A = g.shape[-1]
    ag, aa = np.abs(g), np.abs(a)
    ga, gg = (g * a).sum(-1), (g * g).sum(-1)
    d_ga = (ag * da + aa * dg + da * dg).sum(-1) + gm(A) * ((ag + dg) * (aa + da)).sum(-1)
    d_gg = (2 * ag * dg + dg * dg).sum(-1) + gm(A) * ((ag + dg) ** 2).sum(-1)
    pred = ga + prev_c
    d_pred = d_ga + U * (np.abs(pred) + d_ga)
    numer = pred - delta
    d_numer = d_pred + U * (np.abs(numer) + d_pred)
    denom = gg + 1e-8
    d_denom = d_gg + abs(1e-8 - F32_EPS) + U * (denom + d_gg)
    q = numer / denom
    with np.errstate(divide='ignore', invalid='ignore'):
        d_q = np.where(denom > d_denom, (d_numer + np.abs(q) * d_denom) / np.maximum(denom - d_denom, 1e-300), np.inf)
        d_q = d_q + U * (np.abs(q) + d_q)
        mult = np.maximum(q, 0.0)
        d_p = mult[..., None] * dg + ag * d_q[..., None] + d_q[..., None] * dg \
            + U * (mult + d_q)[..., None] * (ag + dg)
        x = a - mult[..., None] * g
        d_x = da + d_p + U * (np.abs(x) + da + d_p)
    fixed = np.clip(x, -1.0, 1.0)
    fixed_b = np.minimum(np.where(np.isfinite(d_x), MG * d_x, np.inf), 2.0)
    corrected = pred > delta
    c3 = corrected[..., None]
    return dict(a_safe=np.where(c3, fixed, a), a_safe_b=np.where(c3, fixed_b, da),
                other=np.where(c3, a, fixed), other_b=np.where(c3, da, fixed_b),
                pred=pred, pred_b=d_pred, corrected=corrected, edge=np.abs(pred - delta) <= d_pred)


def g_values(g_net, obs):
    """g = g_net(obs) in float64 and policy64's bound for an A-wide head"""
    g, dg, _ = policy64.mlp(policy64.layers(getattr(g_net, 'g_net', g_net)), obs)
    return g, dg


def rollout(ac, g_net, out, seed, t0=0, env_offset=0, correct=True, delta=0.0):
    """what rollout_safelayer's outputs should be, teacher-forced on the observations and the prev_cost it recorded:
    policy64.rollout for mu / act / logp / val / val_last, g and the correction on top"""
    w = policy64.rollout(policy64.ActorCritic(ac), out, seed, t0=t0, env_offset=env_offset)
    w['g'], w['g_b'] = g_values(g_net, np.asarray(out['obs']))
    if correct:
        c = correction64(w['g'], w['g_b'], w['act'], w['act_b'], np.asarray(out['prev_cost']), delta)
    else:
        z = np.zeros(w['act'].shape[:-1], bool)
        c = dict(a_safe=w['act'], a_safe_b=w['act_b'], other=w['act'], other_b=w['act_b'], corrected=z, edge=z)
    w['act_safe'], w['act_safe_b'] = c['a_safe'], c['a_safe_b']
    w['corr'] = c
    return w


def compare_act_safe(got, want, what=""):
    """every act_safe element within its bound; on an edge row either branch's value is accepted (row-wise: the whole
    row from one branch).  Returns (largest err / bound, median bound, share of edge rows)."""
    c = want['corr']
    g = np.asarray(got['act_safe'], np.float64)
    assert np.isfinite(g).all(), what
    def ratio(err, b):      # err / bound; an exact element (bound 0, the untouched branch on exact inputs) is 0 or inf
        with np.errstate(divide='ignore', invalid='ignore'):
            return np.where(err <= b, np.where(b > 0, err / b, 0.0), np.where(b > 0, err / b, np.inf))
    r_main = ratio(np.abs(g - c['a_safe']), c['a_safe_b'])
    r_other = ratio(np.abs(g - c['other']), c['other_b'])
    row_main, row_other = r_main.max(-1), r_other.max(-1)
    row = np.where(c['edge'], np.minimum(row_main, row_other), row_main)
    if not (row <= 1.0).all():
        i = np.unravel_index(np.argmax(row), row.shape)
        raise AssertionError(f"{what} act_safe: {int((row > 1).sum())} of {row.size} rows outside the float64 bound; worst "
                             f"at {tuple(int(j) for j in i)}: got {g[i]!r}, want {c['a_safe'][i]!r}, bound "
                             f"{c['a_safe_b'][i]!r}, edge {bool(c['edge'][i])}")
    return float(row.max()), float(np.median(c['a_safe_b'])), float(c['edge'].mean())


def closed_loop(O, ac, g_net, T, seed, delta=0.0, correct=True):
    """the safelayer collection loop on the CPU checker's engine `O` (oracle.gxo.OracleEngine, already reset: pass its
    observation as O.obs0) with the policy, g and the correction evaluated in float64 and the action handed over in
    float32: checker-generated observations and costs for sizing a test's inputs.  Returns time-major numpy arrays obs,
    prev_cost, cost, done and the float64 correction record of every step."""
    pol = policy64.ActorCritic(ac)
    N = O.N
    o, prev_c = O.obs0, np.zeros(N, np.float32)
    rec = dict(obs=[], prev_cost=[], cost=[], done=[], corrected=[], edge=[])
    env = np.arange(N, dtype=np.int64)
    for t in range(T):
        w = pol.step(o, seed, env, np.full(N, t, np.int64))
        g, dg = g_values(g_net, o)
        c = correction64(g, dg, w['act'], w['act_b'], prev_c, delta)
        a_safe = (c['a_safe'] if correct else w['act']).astype(np.float32)
        rec['obs'].append(o); rec['prev_cost'].append(prev_c); rec['corrected'].append(c['corrected']); rec['edge'].append(c['edge'])
        _, _, d, info = O.step(a_safe)
        o = O.reset_done()
        rec['cost'].append(info['cost']); rec['done'].append(d)
        prev_c = np.where(d > 0, np.float32(0), info['cost']).astype(np.float32)
    return {k: np.array(v) for k, v in rec.items()}
