"""The float64 restatements (oracle/policy64.py, tests/{safelayer64,usl64,lpg64,buffer64,fisher64}.py) and the host paths
of guardx_amd/rollout_buffer.py against the reference learners' OWN code, run on the CPU live from a checkout of the
reference (tests/reflearn.py).  Every kernel test compares a kernel with a restatement; these tests are what keeps a
restatement from being a misreading of the reference that kernel and test then share.  CPU only; the whole file skips
where the checkout is absent, and nothing of it is recorded here.

Tolerances.  Each comparison prints the largest difference between the reference and the restatement; the value
observed is written into the test's docstring (MEASURED) and asserted at 10 x that.  Each test also runs one planted
mistake in the restatement and asserts that it misses the same tolerance by 10 x or more.  Where the reference code can
be run in float64 (its modules .double(), float64 inputs) both sides are float64; where it casts to float32 itself it
runs in its own float32 against the float64 restatement.  Rows on a threshold (q near delta, max a near 1), where a
float32 and a float64 evaluation may stop for different reasons, are taken out by the restatement's own edge test; their
share is capped at EDGE_CAP.
"""
import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

EDGE_CAP = 0.02
F = np.float32


def settle(what, measured, planted, recorded):
    """print the comparison's line, then: the measured difference within 10 x the recorded one, the planted mistake's
    at least 10 x beyond that"""
    tol = 10.0 * recorded
    print(f"reference vs restatement: {what}: largest difference {measured:.3e} (recorded {recorded:.1e}, asserted at "
          f"{tol:.1e}); planted mistake {planted:.3e}")
    assert measured <= tol, (what, measured, tol)
    assert planted >= 10.0 * tol, (what, planted, tol)


def spread(net, scale, seed):
    """torch's default initialisation is tame (no unit near saturation, a flat critic): scale the Linear weights and give
    the biases a spread, in place"""
    import torch
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, torch.nn.Linear):
                m.weight.mul_(scale)
                m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=gen))
    return net


# ---------------------------------------------------------------------------------------------------------------------
# (a) the actor-critic step
# ---------------------------------------------------------------------------------------------------------------------
AC_CASES = [(64, 43, 2), (256, 80, 8), (64, 80, 2), (256, 43, 8)]        # hidden, D, A
AC_MEASURED = {"trpo": 6.4e-16, "cpo": 6.4e-16, "scpo": 1.2e-15}


def _ac_step_diffs(learner, hidden, D, A, planted):
    import torch
    from oracle import policy64
    import usl64
    n, seed = 50, (11, 12)
    Din = D + 1 if learner == "scpo" else D
    ac = reflearn.actor_critic(learner, D, A, hidden, seed=hidden + D + A)
    spread(ac, 2.0, 1)
    with torch.no_grad():
        ac.pi.log_std.copy_(torch.linspace(-1.5, 0.3, A))
    rng = np.random.default_rng(D + A)
    obs = rng.normal(size=(n, Din))
    if learner == "scpo":
        obs[:, -1] = np.abs(obs[:, -1])                                  # M, the running maximum of the cost
    ours = policy64.ActorCritic(ac)
    w = ours.step(obs, seed, np.arange(n), np.full(n, 3))
    ac = ac.double()
    o = torch.from_numpy(obs)
    with torch.no_grad():
        pi = ac.pi._distribution(o)
        ref = dict(mu=pi.mean.numpy(), logstd=np.broadcast_to(torch.log(pi.stddev).numpy(), (n, A)),
                   logp=ac.pi._log_prob_from_distribution(pi, torch.from_numpy(w['act'])).numpy(), val=ac.v(o).numpy())
        if learner != "trpo":
            ref['vc'] = ac.vc(o).numpy()
    got = dict(mu=w['mu'], logstd=np.broadcast_to(w['logstd'], (n, A)), logp=w['logp'], val=w['val'])
    if planted:
        std = np.exp(ours.log_std)                                      # the planted mistake: std where the variance belongs
        got['logp'] = np.sum(-((w['act'] - w['mu']) ** 2) / (2.0 * std) - ours.log_std - policy64.HALF_LOG_2PI, -1)
    if learner == "cpo":
        got['vc'] = policy64.critic(ac.vc, obs)[0]
    if learner == "scpo":
        mods = list(ac.vc.v_net)
        assert type(mods[-1]).__name__ == 'Softplus'
        pre, _, _ = policy64.mlp(policy64.layers(mods[:-1]), obs)
        got['vc'] = usl64.softplus64(pre[..., 0])
    assert set(got) == set(ref)
    return {k: float(np.abs(got[k] - ref[k]).max() / max(1.0, np.abs(ref[k]).max())) for k in ref}


@pytest.mark.parametrize("learner", ["trpo", "cpo", "scpo"])
def test_actor_critic_step(learner):
    """MLPActorCritic of <learner>_core.py in float64 (SCPO's on cat(obs, M), with its Softplus cost critic) against
    policy64.ActorCritic.step, policy64.critic and softplus64: pi.mean, log(pi.stddev), _log_prob_from_distribution at
    policy64's own action, v, vc; relative to max(1, the output's largest magnitude).
    MEASURED (largest over the cases and outputs), each asserted on its own: trpo 6.4e-16, cpo 6.4e-16, scpo 1.2e-15
    -> AC_MEASURED; the planted mistake 0.37.
    Planted: log pi(a) with the standard deviation where the variance belongs."""
    worst, planted = 0.0, np.inf
    for hidden, D, A in AC_CASES:
        d = _ac_step_diffs(learner, hidden, D, A, planted=False)
        p = _ac_step_diffs(learner, hidden, D, A, planted=True)
        print(f"  {learner} hidden {hidden} D {D} A {A}: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items()))
        worst, planted = max(worst, max(d.values())), min(planted, p['logp'])
    settle(f"actor-critic step, {learner}_core", worst, planted, AC_MEASURED[learner])


# ---------------------------------------------------------------------------------------------------------------------
# (b) safety_correction
# ---------------------------------------------------------------------------------------------------------------------
def _rows(n, D, A, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, D)).astype(F), (0.6 * rng.normal(size=(n, A))).astype(F), rng.random(n).astype(F)


def _deltas(q):
    """float32 deltas below, inside (two) and above the spread of q"""
    q = np.asarray(q, np.float64)
    return [float(F(v)) for v in (q.min() - 0.5, np.quantile(q, 0.3), np.quantile(q, 0.7), q.max() + 0.5)]


SAFELAYER_MEASURED = {False: 7.2e-15, True: 7.2e-15}        # the plain core, its one-episode twin


@pytest.mark.parametrize("one_episode", [False, True])
def test_safelayer_correction(one_episode):
    """C_Critic.safety_correction of safelayer_core.py and of its one-episode twin (whose multiplier is the general
    mult.view(-1, 1) * g; the plain one's cat((mult, mult)) serves A = 2 alone and raises at A = 8, which is pinned here)
    in float64 against safelayer64.correction64 on exact inputs, A = 2 and 8, widths 64 and 256, four deltas.
    MEASURED (largest |a_safe - reference| over the cases): plain 7.2e-15, one-episode 7.2e-15 -> SAFELAYER_MEASURED; the
    planted mistake 0.80 and 0.17.
    Planted: prev_cost dropped from the numerator."""
    import torch
    import safelayer64
    assert not reflearn.same_code("safelayer", "C_Critic")
    worst, planted, n = 0.0, np.inf, 64
    for A, hidden in ((2, 64), (8, 256), (2, 256), (8, 64)):
        D = 43
        cc = spread(reflearn.c_critic("safelayer", D, A, hidden, seed=A + hidden, one_episode=one_episode), 2.0, 2).double()
        obs, act, prev = _rows(n, D, A, A * hidden)
        g, _ = safelayer64.g_values(cc, obs)
        zero = np.zeros_like(g)
        pred = (g * act).sum(-1) + prev
        for delta in _deltas(pred):
            c = safelayer64.correction64(g, zero, act, zero, prev, delta)
            ok = np.abs(c['pred'] - delta) > 1e-9                        # float64 on both sides: no row sits that close
            assert ok.all()
            args = [torch.from_numpy(np.asarray(x, np.float64)) for x in (obs, act, prev)]
            was = torch.get_default_dtype()
            torch.set_default_dtype(torch.float64)                       # a_result = torch.zeros(act.shape) follows it
            try:
                if A != 2 and not one_episode:                               # (with no row to correct as well)
                    with pytest.raises(RuntimeError):
                        cc.safety_correction(*args, delta=delta)
                    continue
                ref = cc.safety_correction(*args, delta=delta).numpy()
            finally:
                torch.set_default_dtype(was)
            assert ref.dtype == np.float64
            worst = max(worst, float(np.abs(c['a_safe'] - ref).max()))
            if c['corrected'].any():
                wrong = safelayer64.correction64(g, zero, act, zero, np.zeros_like(prev), delta)
                wrong = np.where(c['corrected'][:, None], wrong['a_safe'], act)
                rows = c['corrected'] & (np.abs(ref) < 1).all(-1)        # (a clamped row can hide it)
                if rows.any():
                    planted = min(planted, float(np.abs(wrong - ref)[rows].max()))
    settle(f"safety_correction, safelayer_core{' (one-episode)' if one_episode else ''}", worst, planted, SAFELAYER_MEASURED[one_episode])


def memoryless_iterate(Q, obs, a, delta, niter, eta, grad_scale, carry=False):
    """usl64.QCritic.iterate as it stood before the reference was consulted, kept as the PLANTED variant: every pass
    steps along the fresh gradient alone.  carry=True is the rule of usl_core.py:180-194 (the running sum) through the
    same loop, which also collects the edge rows of every pass: -> a_safe, iters, stop, edge"""
    a = np.array(a, np.float64)
    n = a.shape[0]
    stop, iters, edge = np.full(n, -1), np.zeros(n, np.int64), np.zeros(n, bool)
    acc, dacc, da = None, None, np.zeros(n)
    for _ in range(niter):
        live = stop < 0
        if not live.any():
            break
        r = Q.one_pass(obs, a, delta, eta, grad_scale, da=da, acc=acc if carry else None, dacc=dacc if carry else None)
        acc, dacc = r['acc'], r['dacc']
        edge |= live & r['edge']
        st = np.where(live, r['stop'], stop)
        moved = live & (st < 0)
        a = np.where(moved[:, None], r['a_next'], a)
        da = np.where(moved, da + r['da_next'].max(-1), da)
        iters += moved
        stop = st
    return dict(a_safe=a, iters=iters, stop=np.where(stop < 0, 0, stop), edge=edge)


USL_MEASURED = {1: 2.8e-7, 2: 3.5e-7, 3: 4.1e-7, 20: 1.6e-6}


@pytest.mark.parametrize("niter", [1, 2, 3, 20])
def test_usl_correction(niter):
    """C_Critic.safety_correction of usl_core.py (float32: it casts its inputs itself) against usl64.QCritic.iterate with
    grad_scale = 1 / rows, 256 rows, A = 2 and 8, widths 64 and 256, four deltas, eta = 0.05; the one-episode twin is the
    same code (asserted).  Rows that are edge rows in some pass are excluded, at most EDGE_CAP of a case.
    MEASURED (largest |a_safe - reference|): Niter 1: 2.8e-7, 2: 3.5e-7, 3: 4.1e-7, 20: 1.6e-6 -> USL_MEASURED; edge rows 0
    of every case up to Niter = 3, at most 0.008 of a case at 20.
    Planted: the memoryless iteration (memoryless_iterate), which IS the rule at Niter = 1 and is therefore asserted from
    Niter = 2 on, over the rows that move twice or more: 1.6e-3 away at Niter = 2, 5.0e-3 at 3, 0.56 at 20.  Both figures
    are formed the same way, the largest difference over the cases' rows: the measured one must stay inside the
    tolerance on every row, the planted one must leave it on some row (a row that moves twice along nearly the same
    gradient is nearly where the memoryless step puts it, so the smallest planted difference says nothing)."""
    import torch
    import usl64
    assert reflearn.same_code("usl", "C_Critic")
    worst, planted, n, shares = 0.0, 0.0, 256, []
    for A, hidden in ((2, 64), (8, 256), (2, 256), (8, 64)):
        D = 43
        cc = spread(reflearn.c_critic("usl", D, A, hidden, seed=A + hidden), 1.5, 3)
        obs, act, _ = _rows(n, D, A, A * hidden + 1)
        Q = usl64.QCritic(cc)
        q0 = Q.forward(obs, act)['q']
        for delta in _deltas(q0):
            ref = cc.safety_correction(obs.copy(), act.copy(), None, delta=delta, Niter=niter, eta=0.05).numpy()
            assert ref.dtype == np.float32
            it = Q.iterate(obs, act, delta, niter, 0.05, 1.0 / n)
            ed = memoryless_iterate(Q, obs, act, delta, niter, 0.05, 1.0 / n, carry=True)
            np.testing.assert_array_equal(it['a_safe'], ed['a_safe'])
            ok = ~ed['edge']
            shares.append(float((~ok).mean()))
            assert (~ok).mean() <= EDGE_CAP, (A, hidden, delta, (~ok).mean())
            worst = max(worst, float(np.abs(it['a_safe'] - ref)[ok].max()))
            old = memoryless_iterate(Q, obs, act, delta, niter, 0.05, 1.0 / n)
            twice = ok & (it['iters'] >= 2)
            if twice.any():
                planted = max(planted, float(np.abs(old['a_safe'] - ref)[twice].max()))
    print(f"  usl Niter {niter}: edge rows per case {' '.join(f'{v:.3f}' for v in shares)}")
    if niter == 1:
        planted = np.inf
    settle(f"safety_correction, usl_core, Niter = {niter}", worst, planted, USL_MEASURED[niter])


LPG_MEASURED = 9.1e-7


def test_lpg_correction():
    """C_Critic.safety_correction of lpg_core.py (its own float32 / numpy mix; Q_init set by store_init on the first
    rows, as lpg.py:489-490 does) against lpg64.probe64 with grad_scale = 1 / rows, widths 64 and 256, five deltas.  The
    reference's multiplier is concatenate((lam, lam)) * G: it serves A = 2 alone and raises at A = 8 (pinned here at both
    widths; the one-episode twin is the same file), so lpg64's general lam[:, None] * G is compared at A = 2.  Edge rows (q near
    delta, lam near 0) excluded, at most EDGE_CAP of a case.
    MEASURED (largest |a_safe - reference|): 9.1e-7 -> LPG_MEASURED; the planted mistake 0.61.
    Planted: epsilon = |delta - Q_init| dropped from the numerator."""
    import torch
    import usl64
    import lpg64
    assert reflearn.same_code("lpg", "C_Critic")
    worst, planted, n, D, projected = 0.0, np.inf, 64, 43, 0
    for A, hidden in ((2, 64), (2, 256), (8, 64), (8, 256)):
        cc = spread(reflearn.c_critic("lpg", D, A, hidden, seed=A + hidden), 1.5, 4)
        obs, act, _ = _rows(n, D, A, A * hidden + 2)
        Q = usl64.QCritic(cc)
        q = Q.forward(obs, act)['q']
        # G carries the 1 / rows of pred_0.mean(), so G . a is small and lam > 0 needs epsilon = |delta - Q_init| smaller
        # still: the first step's rows lie within 1e-3 of the row whose q is the median, and one delta is their Q
        mid = int(np.argsort(q)[n // 2])
        obs0, act0, _ = _rows(n, D, A, A * hidden + 3)
        obs0, act0 = (obs[mid] + F(1e-3) * obs0).astype(F), (act[mid] + F(1e-3) * act0).astype(F)
        cc.store_init(obs0, act0)
        # Q_init is an INPUT of the projection, float32 as the reference keeps it (lpg64: "exact fp32 inputs act, q_init
        # and delta"): both sides get the reference's own.  (From a float64 Q_init instead, 1e-7 away, a_safe moves by
        # that over |G|, 2e-4 here: the projection's conditioning, inside lpg64's da_safe, not a disagreement.)
        q_init = cc.get_Q_init()
        assert q_init.dtype == np.float64 and np.abs(Q.forward(obs0, act0)['q'] - q_init).max() < 2e-6
        for delta in _deltas(q) + [float(F(np.median(q_init)))]:
            o, a = torch.from_numpy(obs), torch.from_numpy(act)
            w = lpg64.probe64(Q, obs, act, q_init, delta, 1.0 / n)
            if A != 2:                                                   # (with no row to correct as well)
                with pytest.raises(ValueError):
                    cc.safety_correction(o, a, None, delta=delta)
                continue
            ref = cc.safety_correction(o, a, None, delta=delta).numpy()
            ok = ~w['edge']
            assert (~ok).mean() <= EDGE_CAP, (hidden, delta, (~ok).mean())
            worst = max(worst, float(np.abs(w['a_safe'] - ref)[ok].max()))
            projected += int((ok & (w['branch'] == 1)).sum())
            wrong = lpg64.project64(act, w['G'], w['dG'], w['q'], w['dq'], np.full(n, delta), delta)   # epsilon = 0
            if (ok & (wrong['branch'] == 1)).any():
                planted = min(planted, float(np.abs(wrong['a_safe'] - ref)[ok].max()))
    assert projected >= 20, projected                                    # rows with lam > 0 were compared
    settle("safety_correction, lpg_core", worst, planted, LPG_MEASURED)


# ---------------------------------------------------------------------------------------------------------------------
# (c) the buffers
# ---------------------------------------------------------------------------------------------------------------------
BUFFERS = {   # learner: (class, keys stored beside obs act rew val logp mu logstd, in store()'s order)
    "trpo": "TRPOBufferX", "cpo": "CPOBufferX", "scpo": "SCPOBufferX", "safelayer": "SafeLayerBufferX",
    "usl": "UslBufferX", "lpg": "LpgBufferX",
}
BUFFER_SIZES = [(5, 9), (67, 24)]
# learner: the largest difference of the reference from buffer64; from the host path of its *_rollout_batch (None: no host path)
BUFFER_MEASURED = {"trpo": (5.9e-7, None), "cpo": (9.9e-7, None), "scpo": (1.0e-6, None), "safelayer": (5.9e-7, 1.9e-6),
                   "usl": (5.9e-7, 1.9e-6), "lpg": (5.9e-7, 1.9e-6)}
GAMMA, LAM, CGAMMA, CLAM = 0.99, 0.95, 1.0, 0.95


def drive(learner, g):
    """store / finish_path / get as the learner's collection loop drives them (trpo.py:465-547 and the same block of the
    others): store every step; where some env is done, finish_path with v (and vc) = 0 for the done envs (the others'
    entries, ac.step's value of the next observation, are never read: they are poisoned here) and done itself; at the
    epoch's end finish_path with zeros over every env.  -> the batch as numpy"""
    import torch
    T, N = g['rew'].shape
    D, A = g['obs'].shape[-1], g['act'].shape[-1]
    cls, = reflearn.main(learner, [BUFFERS[learner]])
    buf = cls(N, T, (D,), (A,), GAMMA, LAM) if learner != "scpo" else cls(N, T, (D,), (A,), GAMMA, LAM, CGAMMA, CLAM)
    t_ = lambda x: torch.from_numpy(np.ascontiguousarray(x))   # noqa: E731
    logstd = t_(np.broadcast_to(g['logstd'].reshape(1, A), (N, A)).copy())
    two = learner in ("cpo", "scpo")
    for t in range(T):
        o, a, r, v, lp, mu = (t_(g[k][t]) for k in ('obs', 'act', 'rew', 'val', 'logp', 'mu'))
        if learner == "trpo":
            buf.store(o, a, r, v, lp, mu, logstd)
        elif two:
            buf.store(o, a, r, v, lp, t_(g['cost_inc' if learner == "scpo" else 'cost'][t]), t_(g['vc'][t]), mu, logstd)
        elif learner == "safelayer":
            buf.store(o, a, t_(g['act_safe'][t]), r, v, lp, mu, logstd, t_(g['cost'][t]), t_(g['prev_cost'][t]))
        else:
            buf.store(o, a, t_(g['act_safe'][t]), r, v, lp, mu, logstd, t_(g['cost'][t]), t_(g['qc'][t]))
        if t + 1 == T:
            last, done = torch.zeros(N), np.ones(N)
        elif g['done'][t].any():
            done = g['done'][t]
            last = torch.full((N,), 1e6)
            last[np.where(done == 1)] = 0.0
        else:
            continue
        buf.finish_path(last, last.clone(), done) if two else buf.finish_path(last, done)
    return {k: v.numpy() for k, v in buf.get().items()}


def _buffer_inputs(N, T, kind):
    import buffer64 as b64
    rew, val, done, _ = b64.gae_inputs(N, T, kind, seed=3, mixed=kind == 'mixed')
    return b64.rollout_out(N, T, 6, 4, rew, val, done, seed=N + T)


def _restated(learner, g, ddof=0):
    """the batch from tests/buffer64.py in float64: {key: value}, env-major and flattened"""
    import buffer64 as b64
    close, _ = b64.rollout_paths(g['done'])
    (adv, _), (ret, _), (raw, braw) = b64.rollout64(g['rew'], g['val'], g['done'], None, b64.coef_gae(GAMMA, LAM))
    if ddof:
        adv = b64.normalize64(raw.T, braw.T, 1, None, ddof)[0]
    out = dict(adv=adv.reshape(-1), ret=b64.env_major(ret))
    if learner in ("cpo", "scpo"):
        cg_, cl_ = (CGAMMA, CLAM) if learner == "scpo" else (GAMMA, LAM)
        cost = g['cost_inc'] if learner == "scpo" else g['cost']
        (adc, _), (cret, _), _ = b64.rollout64(cost, g['vc'], g['done'], None, b64.coef_gae(cg_, cl_), scale=0)
        out.update(adc=adc.reshape(-1), cost_ret=b64.env_major(cret))
    if learner in ("usl", "lpg"):
        out['targetc'] = b64.env_major(b64.targetc64(g['cost'], g['qc'], close, GAMMA)[0])
    return out


EXACT_KEYS = {"trpo": (), "cpo": (), "scpo": (), "safelayer": ('act_safe', 'cost', 'prev_cost'),
              "usl": ('act_safe', 'cost'), "lpg": ('act_safe', 'cost')}


@pytest.mark.parametrize("learner", list(BUFFERS))
def test_buffers(learner):
    """store / finish_path / get of the learner's *BufferX class (float32 storage, scipy's filter in double) driven as
    its loop drives it, on synthetic rollouts of (N, T) = (5, 9) and (67, 24) with dones inside the epoch (the per-env
    branch) and without (the batch branch), against tests/buffer64.py (rollout64 with coef_gae, normalize64, targetc64)
    in float64 and, for safelayer / usl / lpg, against the host-tensor path of guardx_amd.rollout_buffer's
    *_rollout_batch (gae_rollout, cost_ and statewise_rollout_batch have no host path: they go through the kernels, which
    tests/test_gpu_buffer64.py holds to the same restatement).  The copied columns must be equal exactly.
    MEASURED (largest |difference| over adv, ret, adc, cost_ret, targetc), the two comparisons settled apart, each learner
    at its own figure: buffer64 5.9e-7 (trpo, safelayer, usl, lpg), 9.9e-7 (cpo), 1.0e-6 (scpo: adc); host path 1.9e-6
    (safelayer, usl, lpg: ret, whose filter the host path runs in float32) -> BUFFER_MEASURED; the planted mistake 6.3e-2
    against either.
    Planted: the sample deviation (ddof = 1) in the advantages' normalisation."""
    import torch
    import buffer64 as b64
    from guardx_amd import rollout_buffer as rb
    host = dict(safelayer=rb.safelayer_rollout_batch, usl=rb.usl_rollout_batch, lpg=rb.lpg_rollout_batch).get(learner)
    worst, worst_host, planted, planted_host = 0.0, 0.0, np.inf, np.inf
    for N, T in BUFFER_SIZES:
        for kind in ('mixed', 'none'):
            g = _buffer_inputs(N, T, kind)
            assert (g['done'][:-1].sum() > 0) == (kind == 'mixed')
            ref = drive(learner, g)
            want = _restated(learner, g)
            exact = ('obs', 'act', 'logp', 'mu') + EXACT_KEYS[learner]
            assert set(ref) == set(want) | set(exact) | {'logstd'}, sorted(ref)
            for k in exact:
                np.testing.assert_array_equal(ref[k], b64.env_major(g[k]), err_msg=k)
            np.testing.assert_array_equal(ref['logstd'], np.broadcast_to(g['logstd'], ref['logstd'].shape))
            d = {k: float(np.abs(want[k] - ref[k]).max()) for k in want}
            worst = max(worst, max(d.values()))
            wrong = _restated(learner, g, ddof=1)['adv']
            planted = min(planted, float(np.abs(wrong - ref['adv']).max()))
            line = f"  {learner} N {N} T {T} {kind}: " + "  ".join(f"{k} {v:.2e}" for k, v in d.items())
            if host is not None:
                got = {k: v.numpy() for k, v in host({k: torch.from_numpy(v) for k, v in g.items()}, GAMMA, LAM).items()}
                assert set(got) == set(ref)
                for k in exact + ('logstd',):
                    np.testing.assert_array_equal(got[k], ref[k], err_msg=k)
                h = {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in want}
                worst_host = max(worst_host, max(h.values()))
                planted_host = min(planted_host, float(np.abs(wrong - got['adv']).max()))
                line += "  | host path: " + "  ".join(f"{k} {v:.2e}" for k, v in h.items())
            print(line)
    settle(f"{BUFFERS[learner]}: buffer64", worst, planted, BUFFER_MEASURED[learner][0])
    assert (host is None) == (BUFFER_MEASURED[learner][1] is None)
    if host is not None:
        settle(f"{BUFFERS[learner]}: host path of {host.__name__}", worst_host, planted_host, BUFFER_MEASURED[learner][1])


# ---------------------------------------------------------------------------------------------------------------------
# (d) the Hessian-vector product and cg
# ---------------------------------------------------------------------------------------------------------------------
FISHER_MEASURED = {2: dict(hx=4.6e-16, cg=1.5e-14), 8: dict(hx=4.5e-16, cg=5.9e-15)}        # by A


@pytest.mark.parametrize("A", [2, 8])
def test_hessian_vector_product_and_cg(A):
    """auto_hession_x on the reference actor's own _d_kl (diagonal_gaussian_kl of trpo_core.py, old policy = the actor's
    detached output, as compute_kl_pi builds it) and cg of trpo.py, everything in float64, against fisher64.fvp64 and
    fisher64.cg64 (1, 2, 3 and 10 iterations): B = 37, D = 43, hidden 64.  Relative L2 of the whole vector.
    MEASURED: product 4.6e-16 (A = 2), 4.5e-16 (A = 8); solve 1.5e-14 (A = 2), 5.9e-15 (A = 8), each asserted on its own
    -> FISHER_MEASURED; the planted mistakes 0.38 and 0.47 or more.
    Planted: the first layer's tangent left out of the second layer's (dh1 W2' dropped) in the product; beta left out of
    the direction update (p = r) in the solve."""
    import torch
    import fisher64 as f64
    B, D, h = 37, 43, 64
    cg, auto_grad, auto_hession_x = reflearn.main("trpo", ["cg", "auto_grad", "auto_hession_x"])
    ac = reflearn.actor_critic("trpo", D, A, h, seed=A)
    pi = spread(ac.pi, 2.0, 5)
    with torch.no_grad():
        pi.log_std.copy_(torch.linspace(-1.0, 0.2, A))
    pi = pi.double()
    assert [tuple(p.shape) for p in pi.parameters()] == [(A,), (h, D), (h,), (h, h), (h,), (A, h), (A,)]
    theta = f64.flat(pi).numpy()
    rng = np.random.default_rng(A)
    obs = rng.normal(size=(B, D))
    o = torch.from_numpy(obs)
    with torch.no_grad():
        mu_old, ls_old = pi.mu_net(o), pi.log_std.detach().clone().expand(B, A)

    def Hx_ref(x):
        return auto_hession_x(pi._d_kl(o, mu_old, ls_old, device=torch.device("cpu")), pi, torch.from_numpy(np.asarray(x, np.float64)))

    def planted_fvp(x):                                   # fvp64 without dh1 @ W2.T
        ls, W1, b1, W2, b2, W3, b3 = f64.unpack(theta, D, A, h)
        dls, dW1, db1, dW2, db2, dW3, db3 = f64.unpack(x, D, A, h)
        h1 = np.tanh(obs @ W1.T + b1)
        h2 = np.tanh(h1 @ W2.T + b2)
        dh2 = (1.0 - h2 * h2) * (h1 @ dW2.T + db2)
        u = (h2 @ dW3.T + dh2 @ W3.T + db3) / (np.exp(2.0 * ls) + f64.EPS) / B
        gz2 = (u @ W3) * (1.0 - h2 * h2)
        gz1 = (gz2 @ W2) * (1.0 - h1 * h1)
        return f64.pack((f64.log_std_curvature(ls) * dls, gz1.T @ obs, gz1.sum(0), gz2.T @ h1, gz2.sum(0), u.T @ h2, u.sum(0)))

    xs = rng.normal(size=(4, theta.size))
    hx = max(f64.rel_l2(f64.fvp64(theta, x, obs, A, h), Hx_ref(x)) for x in xs)
    hx_planted = min(f64.rel_l2(planted_fvp(x), Hx_ref(x)) for x in xs)
    settle(f"auto_hession_x, A = {A}", hx, hx_planted, FISHER_MEASURED[A]['hx'])

    def planted_cg(Hx, g, iters):
        x, r, p = np.zeros_like(g), g.copy(), g.copy()
        for _ in range(iters):
            z = Hx(p)
            alpha = float(r @ r) / (float(p @ z) + f64.EPS)
            x += alpha * p
            r -= alpha * z
            p = r.copy()
        return x

    Hx = lambda v: f64.fvp64(theta, v, obs, A, h)   # noqa: E731
    worst, planted = 0.0, np.inf
    for g in xs[:2]:
        for k in (1, 2, 3, 10):
            ref = cg(Hx_ref, g.copy(), cg_iters=k)
            got, done, _ = f64.cg64(Hx, g, iters=k)
            assert done == k
            worst = max(worst, f64.rel_l2(got, ref))
            if k >= 2:
                planted = min(planted, f64.rel_l2(planted_cg(Hx, g, k), ref))
    settle(f"cg, A = {A}", worst, planted, FISHER_MEASURED[A]['cg'])


# ---------------------------------------------------------------------------------------------------------------------
# the loader leaves nothing behind
# ---------------------------------------------------------------------------------------------------------------------
def test_no_stand_in_is_left_in_sys_modules():
    import sys
    for learner in ("trpo", "cpo", "scpo", "safelayer", "usl", "lpg"):
        reflearn.core(learner)
    for name in reflearn.STAND_INS:
        m = sys.modules.get(name)
        assert m is None or getattr(m, '__file__', None) is not None, name      # absent, or the real package
    for name in ("jax", "mujoco"):
        assert name not in sys.modules or getattr(sys.modules[name], '__file__', None) is not None
