"""The line search of include/guardx_linesearch.h in numpy float64 (evaluate64, search64): the oracle of
tests/test_linesearch64.py (which checks it against the learners' formulation in torch float64),
tests/test_reference_linesearch.py and tests/test_gpu_linesearch.py.  Also the learners' own evaluation in torch (in the
precision it is asked for: the float32 one is the yardstick of the device's error), a plain numpy float32 statement of the
header's operations, and the cases the CPU and the GPU tests share.

Vectors are in the order of pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A].
A row of four is kl, pi_l, surr_cost, approx_kl."""
import copy
import functools

import numpy as np

import fisher64 as f64

EPS = 1e-8
H = 64
HALF_LOG_2PI = 0.5 * np.log(2.0 * np.pi)
STEPS = (0.0, 1.0, 0.8 ** 4, 0.8 ** 20)
SEEDS = (0, 1, 2)
ALLOWED = 4.0
DECIDABLE = 100.0


def candidate(theta, d, t):
    """theta_t: float32(double(theta) - t double(d)), rounded once; theta itself at t = 0"""
    theta = np.asarray(theta, dtype=np.float32)
    if t == 0.0:
        return theta.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        return (theta.astype(np.float64) - float(t) * np.asarray(d, dtype=np.float32).astype(np.float64)).astype(np.float32)


def rows64(theta_t, batch, variance=True, eps=EPS, swap=False, log_std_last=False):
    """(kl_row, logp, ratio) of the candidate theta_t over the batch, float64 throughout.  The keywords plant mistakes
    (tests/test_linesearch64.py): the standard deviation where the variance belongs, EPS dropped, the KL's argument pairs
    swapped, log_std read from the end of theta."""
    o = np.asarray(batch["obs"], dtype=np.float64)
    B, D = o.shape
    A = np.asarray(batch["act"]).shape[1]
    v = np.asarray(theta_t, dtype=np.float64)
    if log_std_last:
        v = np.concatenate([v[-A:], v[:-A]])
    ls, W1, b1, W2, b2, W3, b3 = f64.unpack(v, D, A, H)
    mu = np.tanh(np.tanh(o @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
    act, mu_old, lso = (np.asarray(batch[k], dtype=np.float64) for k in ("act", "mu", "logstd"))
    mu0, ls0, mu1, ls1 = (mu, ls + 0.0 * lso, mu_old, lso) if swap else (mu_old, lso, mu, ls + 0.0 * lso)
    e = 2.0 if variance else 1.0
    v0, v1 = np.exp(e * ls0), np.exp(e * ls1)
    kl_row = (0.5 * (((mu1 - mu0) ** 2 + v0) / (v1 + eps) - 1.0) + ls1 - ls0).sum(1)
    logp = (-(act - mu) ** 2 / (2.0 * np.exp(e * ls)) - ls - HALF_LOG_2PI).sum(1)
    ratio = np.exp(logp - np.asarray(batch["logp"], dtype=np.float64))
    return kl_row, logp, ratio


def means64(theta_t, batch, **kw):
    """[kl, pi_l, surr_cost, approx_kl] and the scales [mean |ratio adv|, mean |ratio adc|] of one candidate"""
    kl_row, logp, ratio = rows64(theta_t, batch, **kw)
    adv = np.asarray(batch["adv"], dtype=np.float64)
    adc = np.asarray(batch["adc"], dtype=np.float64) if batch.get("adc") is not None else np.zeros_like(adv)
    lpo = np.asarray(batch["logp"], dtype=np.float64)
    return (np.array([kl_row.mean(), -(ratio * adv).mean(), (ratio * adc).mean(), (lpo - logp).mean()]),
            np.array([np.abs(ratio * adv).mean(), np.abs(ratio * adc).mean()]))


def evaluate64(theta, d, batch, steps, **kw):
    """(len(steps), 4) float64 and the scales (len(steps), 2)"""
    with np.errstate(all="ignore"):
        got = [means64(candidate(theta, d, t), batch, **kw) for t in steps]
    return np.stack([g[0] for g in got]), np.stack([g[1] for g in got])


def accepts(m, old, target_kl, cost_margin, need_loss, has_adc):
    """The rule of include/guardx_linesearch.h on a row of four `m` and the row at t = 0 `old`, both rounded to float32 as
    the learners' .item() rounds them; comparisons in float64, a NaN rejects.  Transcribed from
      trpo.py:423      the KL's .item() at most target_kl, and the new loss's .item() at most the old one's
      cpo.py:545-548   the same KL test; the loss test only where optim_case > 1; and the surrogate cost's rise over the
                       old one at most the larger of -c and -cost_reduction
    need_loss is trpo's "always" and cpo's optim_case > 1; cost_margin is cpo's larger of -c and -cost_reduction."""
    r = lambda x: float(np.float32(x))                               # noqa: E731
    return bool(r(m[0]) <= target_kl and (need_loss == 0 or r(m[1]) <= r(old[1])) and
                (not has_adc or r(m[2]) - r(old[2]) <= cost_margin))


def search64(theta, d, batch, target_kl, cost_margin=0.0, need_loss=1, coeff=0.8, iters=100, **kw):
    """-> dict(accepted, theta_new, means (4,), old (4,), trace (evaluated rows, 4), steps): the learners' loop around
    evaluate64; accepted = -1 and theta_new = theta when no candidate is accepted"""
    has_adc = batch.get("adc") is not None
    old = evaluate64(theta, d, batch, [0.0], **kw)[0][0]
    trace, steps = [old], [coeff ** j for j in range(iters)]
    for j, t in enumerate(steps):
        m = evaluate64(theta, d, batch, [t], **kw)[0][0]
        trace.append(m)
        if accepts(m, old, target_kl, cost_margin, need_loss, has_adc):
            return dict(accepted=j, theta_new=candidate(theta, d, t), means=m, old=old, trace=np.stack(trace), steps=steps)
    return dict(accepted=-1, theta_new=np.asarray(theta, dtype=np.float32).copy(), means=old, old=old, trace=np.stack(trace),
                steps=steps)


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch), in the dtype asked for
# ---------------------------------------------------------------------------------------------------------------------
def assign_flat(pi, flat):
    """the learners' assign_net_param_from_flat"""
    import torch
    at = 0
    with torch.no_grad():
        for p in pi.parameters():
            n = p.numel()
            p.copy_(torch.from_numpy(np.array(flat[at:at + n])).reshape(p.shape).to(p.dtype))
            at += n


def learners_means(pi, theta_t, batch, dtype):
    """[kl, pi_l, surr_cost, approx_kl] the way the learners compute them (trpo.py:341-372, cpo's compute_cost_pi): a
    deep-copied actor with the flat parameters assigned, _d_kl's diagonal_gaussian_kl(mu_old, logstd_old, mu, log_std),
    Normal(mu, exp(log_std)).log_prob(act).sum(-1), every mean in `dtype`; -> float64 array of the four .item()s"""
    import torch
    from torch.distributions.normal import Normal
    tmp = copy.deepcopy(pi).to(dtype)
    assign_flat(tmp, theta_t)
    t = lambda k: torch.from_numpy(np.array(batch[k])).to(dtype)     # noqa: E731
    with torch.no_grad():
        mu = tmp.mu_net(t("obs"))
        kl = f64.mean_kl(t("mu"), t("logstd"), mu, tmp.log_std)      # the learners' diagonal_gaussian_kl, old to new
        logp = Normal(mu, torch.exp(tmp.log_std)).log_prob(t("act")).sum(axis=-1)
        ratio = torch.exp(logp - t("logp"))
        pi_l = -(ratio * t("adv")).mean()
        surr = (ratio * t("adc")).mean() if batch.get("adc") is not None else torch.zeros((), dtype=dtype)
        approx_kl = (t("logp") - logp).mean()
    return np.array([kl.item(), pi_l.item(), surr.item(), approx_kl.item()], dtype=np.float64)


def learners_evaluate(pi, theta, d, batch, steps, dtype):
    return np.stack([learners_means(pi, candidate(theta, d, t), batch, dtype) for t in steps])


# ---------------------------------------------------------------------------------------------------------------------
# the header's operations in plain numpy float32 (no emulation of the kernel's order)
# ---------------------------------------------------------------------------------------------------------------------
def evaluate32(theta, d, batch, steps):
    """mu in float32 (np.tanh and matmul on float32); a row's terms in float64 from the float32 inputs, the four row values
    rounded once to float32, logp rounded before logp_old is subtracted in float32, ratio the float64 exponential of that
    difference rounded to float32; the sums over rows in float64"""
    f, dd = np.float32, np.float64
    o = np.ascontiguousarray(batch["obs"], dtype=f)
    B, D = o.shape
    act, mu_old, lso, adv, lpo = (np.asarray(batch[k], dtype=f) for k in ("act", "mu", "logstd", "adv", "logp"))
    adc = np.asarray(batch["adc"], dtype=f) if batch.get("adc") is not None else np.zeros_like(adv)
    A = act.shape[1]
    out = []
    for t in steps:
        th = candidate(theta, d, t)
        at, parts = 0, []
        for shape in ((A,), (H, D), (H,), (H, H), (H,), (A, H), (A,)):
            n = int(np.prod(shape))
            parts.append(th[at:at + n].reshape(shape))
            at += n
        ls, W1, b1, W2, b2, W3, b3 = parts
        mu = np.tanh(np.tanh(o @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
        assert mu.dtype == f
        ls64 = ls.astype(dd)
        v1 = np.exp(2.0 * ls64)
        i1, i2 = 1.0 / (v1 + EPS), 1.0 / (2.0 * v1)
        dm, da = mu.astype(dd) - mu_old.astype(dd), act.astype(dd) - mu.astype(dd)
        kl_row = (0.5 * ((dm * dm + np.exp(2.0 * lso.astype(dd))) * i1 - 1.0) + (ls64 - lso.astype(dd))).sum(1).astype(f)
        logp = (-(da * da) * i2 - ls64 - HALF_LOG_2PI).sum(1).astype(f)
        diff = logp - lpo
        ratio = np.exp(diff.astype(dd)).astype(f)
        rows = [kl_row, ratio * adv, ratio * adc, lpo - logp]
        assert all(r.dtype == f for r in rows)
        s = [r.astype(dd).sum() / B for r in rows]
        out.append([s[0], -s[1], s[2], s[3]])
    return np.array(out, dtype=dd)


# ---------------------------------------------------------------------------------------------------------------------
# errors
# ---------------------------------------------------------------------------------------------------------------------
def errors(got, want, scales):
    """[kl, pi_l, surr_cost, approx_kl] errors of (steps, 4) `got` against float64 `want`: kl and approx_kl as the relative
    L2 over the steps, pi_l and surr_cost as the root-mean-square over the steps of the error relative to
    mean |ratio adv| / mean |ratio adc| at that step (0 where there is no adc)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    e = np.zeros(4)
    for i in (0, 3):
        e[i] = np.linalg.norm(got[:, i] - want[:, i]) / np.linalg.norm(want[:, i])
    for i, k in ((1, 0), (2, 1)):
        ok = scales[:, k] > 0
        e[i] = np.sqrt(np.mean(((got[ok, i] - want[ok, i]) / scales[ok, k]) ** 2)) if ok.any() else 0.0
    return e


def pooled(errs):
    """root-mean-square over the seeds, per quantity"""
    e = np.asarray(errs, dtype=np.float64)
    return np.sqrt(np.mean(e * e, axis=0))


# ---------------------------------------------------------------------------------------------------------------------
# cases, computed once per process and never written to
# ---------------------------------------------------------------------------------------------------------------------
def batch_of(pi, obs, seed=0, adc=True):
    """the batch a rollout of the float32 actor `pi` over `obs` (a float32 tensor) leaves: mu and logstd what the rollout stores
    (the float32 forward and the broadcast log_std); act sampled from it, logp its float32 log-probability; adv
    normalised, adc centred.  numpy float32, read-only"""
    import torch
    from torch.distributions.normal import Normal
    B, A = obs.shape[0], pi.log_std.numel()
    gen = torch.Generator().manual_seed(500 + seed)
    with torch.no_grad():
        mu = pi.mu_net(obs)
        std = torch.exp(pi.log_std)
        act = mu + std * torch.randn(B, A, generator=gen)
        logp = Normal(mu, std).log_prob(act).sum(axis=-1)
        logstd = pi.log_std.detach().reshape(1, A).expand(B, A).contiguous()
    adv = torch.randn(B, generator=gen)
    cost = torch.randn(B, generator=gen)
    if B > 1:
        adv = (adv - adv.mean()) / adv.std()
        cost = cost - cost.mean()
    batch = dict(obs=obs.numpy(), act=act.numpy(), adv=adv.numpy(), logp=logp.numpy(), mu=mu.numpy(), logstd=logstd.numpy(),
                 adc=cost.numpy() if adc else None)
    for v in batch.values():
        if v is not None:
            v.setflags(write=False)
    return batch


def make_batch(regime, D, A, B, seed=0, adc=True):
    """-> (pi, theta float32, batch): the regime's actor and obs (fisher64.problem) as the old policy, and batch_of them"""
    pi, obs, theta, _ = f64.problem(regime, D, A, B, seed)
    return pi, theta, batch_of(pi, obs, seed, adc)


def scaled_direction(theta, raw, batch, kl_goal):
    """raw scaled so that the float64 KL at t = 1 is about kl_goal (KL is close to quadratic in the step: two passes)"""
    d = np.asarray(raw, dtype=np.float64)
    for _ in range(3):
        kl = evaluate64(theta, d.astype(np.float32), batch, [1.0])[0][0, 0]
        d = d * np.sqrt(kl_goal / kl)
    return d.astype(np.float32)


@functools.lru_cache(maxsize=None)
def evaluate_case(regime, D, A, B, seed, steps=STEPS):
    """dict(pi, theta, d, batch, steps, want (steps, 4), scales, yard (4,): the errors of the learners' float32 evaluation)
    for a random direction whose KL at t = 1 is 0.05"""
    pi, theta, batch = make_batch(regime, D, A, B, seed)
    raw = np.random.default_rng(2000 + seed).standard_normal(f64.param_count(D, A, H))
    d = scaled_direction(theta, raw, batch, 0.05)
    want, scales = evaluate64(theta, d, batch, steps)
    yard = errors(learners_evaluate(pi, theta, d, batch, steps, _f32()), want, scales)
    for a in (d, want, scales, yard):
        a.setflags(write=False)
    return dict(pi=pi, theta=theta, d=d, batch=batch, steps=steps, want=want, scales=scales, yard=yard)


def _f32():
    import torch
    return torch.float32


def pooled_yard(regime, D, A, B, steps=STEPS):
    return pooled([evaluate_case(regime, D, A, B, s, steps)["yard"] for s in SEEDS])


def loss_gradient(pi, theta, batch, with_cost=False):
    """the gradient of pi_l (or of surr_cost) in theta at the old policy, float64, by autograd: the learners' g (and b)"""
    import torch
    from torch.distributions.normal import Normal
    tmp = copy.deepcopy(pi).to(torch.float64)
    assign_flat(tmp, np.asarray(theta, dtype=np.float64))
    t = lambda k: torch.from_numpy(np.array(batch[k])).to(torch.float64)     # noqa: E731
    logp = Normal(tmp.mu_net(t("obs")), torch.exp(tmp.log_std)).log_prob(t("act")).sum(axis=-1)
    ratio = torch.exp(logp - t("logp"))
    loss = (ratio * t("adc")).mean() if with_cost else -(ratio * t("adv")).mean()
    g = torch.autograd.grad(loss, list(tmp.parameters()))
    return torch.cat([x.reshape(-1) for x in g]).numpy()


SEARCH_SHAPE = ("default", 43, 2, 4099)
TARGET_KL = 0.01
# name -> how the case is made (search_case); every one is decidable (tests/test_linesearch64.py)
SEARCH_CASES = ("first", "kl_binds", "loss_binds", "loss_not_needed", "cost_binds", "none")


@functools.lru_cache(maxsize=None)
def search_case(name):
    """dict(pi, theta, d, batch, kw (the criteria and iters), ref (search64's result)).
      first            d = the loss gradient g, KL(1) = target / 2: accepted at j = 0
      kl_binds         d = g, KL(1) = 5 target: the KL admits j = 4 first
      loss_binds       a random d with KL(1) = 5 target under a bound of 10 target, and an adv made so that the loss
                       rises along the step from j = 3 up and falls from j = 4 down: j = 4
      loss_not_needed  the same with need_loss = 0: j = 0
      cost_binds       d = g, KL(1) = target / 2, adc oriented so that the cost rises along the step and a margin halfway
                       between the rises of j = 2 and j = 3: j = 3
      none             d = -g (ascent), iters = 10: nothing is accepted"""
    regime, D, A, B = SEARCH_SHAPE
    pi, theta, batch = make_batch(regime, D, A, B, seed=3, adc=name == "cost_binds")
    g = loss_gradient(pi, theta, batch)
    kw = dict(target_kl=TARGET_KL, cost_margin=0.0, need_loss=1, coeff=0.8, iters=100)
    if name == "first":
        d = scaled_direction(theta, g, batch, 0.5 * TARGET_KL)
    elif name == "kl_binds":
        d = scaled_direction(theta, g, batch, 5.0 * TARGET_KL)
    elif name in ("loss_binds", "loss_not_needed"):
        d = scaled_direction(theta, np.random.default_rng(77).standard_normal(g.size), batch, 5.0 * TARGET_KL)
        # L(t) = -mean((ratio_t - 1) adv) for a centred adv: the adv in the span of ratio - 1 at j = 3 and at j = 4 for which
        # L is +1 at the one and -1 at the other, then normalised as the learners normalise theirs.  Along a ray L is
        # close to -t (alpha + t gamma), so larger steps lose as well and smaller ones win.
        u = np.stack([rows64(candidate(theta, d, 0.8 ** j), batch)[2] - 1.0 for j in (3, 4)])
        u = u - u.mean(1, keepdims=True)
        p = np.linalg.solve(u @ u.T / B, np.array([-1.0, 1.0]))
        adv = p @ u
        batch = dict(batch, adv=((adv - adv.mean()) / adv.std()).astype(np.float32))
        batch["adv"].setflags(write=False)
        kw.update(target_kl=10.0 * TARGET_KL, need_loss=int(name == "loss_binds"))
    elif name == "cost_binds":
        b = loss_gradient(pi, theta, batch, with_cost=True)
        d = scaled_direction(theta, g / np.linalg.norm(g) - b / np.linalg.norm(b), batch, 0.5 * TARGET_KL)   # the cost rises
        m = evaluate64(theta, d, batch, [0.0, 0.8 ** 2, 0.8 ** 3])[0]
        r2, r3 = m[1:, 2] - m[0, 2]
        assert r2 > r3 > 0
        kw.update(cost_margin=float(0.5 * (r2 + r3)))
    elif name == "none":
        d = scaled_direction(theta, -g, batch, 0.5 * TARGET_KL)
        kw.update(iters=10)
    else:
        raise KeyError(name)
    d.setflags(write=False)
    ref = search64(theta, d, batch, **kw)
    return dict(pi=pi, theta=theta, d=d, batch=batch, kw=kw, ref=ref)



def search_yardstick(case):
    """(rows, 4): the absolute error of the learners' float32 evaluation that goes with each row of the case's trace: its
    pooled relative error over the trace's steps (errors()) times the row's own scale (|kl|, mean |ratio adv|,
    mean |ratio adc|, |approx_kl|)"""
    ref = case["ref"]
    steps = [0.0] + list(ref["steps"][:len(ref["trace"]) - 1])
    want, scales = evaluate64(case["theta"], case["d"], case["batch"], steps)
    rel = errors(learners_evaluate(case["pi"], case["theta"], case["d"], case["batch"], steps, _f32()), want, scales)
    size = np.stack([np.abs(want[:, 0]), scales[:, 0], scales[:, 1], np.abs(want[:, 3])], axis=1)
    return rel * size, rel, want, scales


def margins(case):
    """for every evaluated candidate (up to and including the accepted one) and every threshold it is tested against: the
    distance from the threshold in float64 over the yardstick's absolute error of that quantity -> list of (j, what, ratio)"""
    ref, kw = case["ref"], case["kw"]
    yard_abs, _, want, _ = search_yardstick(case)
    has_adc = case["batch"].get("adc") is not None
    out = []
    for r in range(1, len(want)):
        out.append((r - 1, "kl", abs(want[r, 0] - kw["target_kl"]) / yard_abs[r, 0]))
        if kw["need_loss"]:
            out.append((r - 1, "pi_l", abs(want[r, 1] - want[0, 1]) / (yard_abs[r, 1] + yard_abs[0, 1])))
        if has_adc:
            out.append((r - 1, "surr_cost", abs(want[r, 2] - want[0, 2] - kw["cost_margin"]) / (yard_abs[r, 2] + yard_abs[0, 2])))
    return out
