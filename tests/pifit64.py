"""The policy fit of include/guardx_pifit.h in numpy float64: the gradient of the learners' three actor losses in closed form
(grad64: pgrad64's forward and backward with the clipped row weight), torch's single-tensor Adam (vfit64.adam64) and the
learners' loop with its early stop around both (fit64) -- the oracle of tests/test_pifit64.py (which checks it against float64
autograd and a transcription of the loop around torch.optim.Adam), tests/test_reference_pifit.py and tests/test_gpu_pifit.py.
Also the learners' own method in torch (in the precision it is asked for: the float32 one is the yardstick of the device's
error) and the cases the CPU and the GPU tests share.

What is computed (include/guardx_pifit.h), per row with ratio = exp(logp - logp_old), lo = 1 - clip_ratio, hi = 1 + clip_ratio:
    loss = -mean(min(ratio adv, clamp(ratio, lo, hi) adv))     ('ratio'; without clip_ratio -mean(ratio adv))
    loss = -mean(logp adv)                                      ('logp')
    kl = mean(logp_old - logp)    cf = mean(ratio > hi or ratio < lo)    ent = sum_a(log_std + 0.5 + 0.5 log 2 pi)
    row weight c = -adv ratio active / B ('ratio'), -adv / B ('logp'); active = 0 exactly where adv > 0 and ratio > hi or
    adv < 0 and ratio < lo (where the clamped branch is the smaller: only the selected branch of torch.min passes), else 1
and from dmu = c (a - mu) / v1 and dlog_std = sum c ((a - mu)^2 / v1 - 1) on pgrad64's backward.  The loop, i = 0 .. iters - 1:
evaluate loss, kl, cf at the current parameters; stop if kl > target_kl (the threshold itself; a NaN does not stop); else one
Adam step, t = t + 1.  A stopped iteration takes no step and does not advance t.

Vectors are in the order of pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]."""
import copy
import functools

import numpy as np

import fisher64 as f64
import linesearch64 as l64
import pgrad64 as p64
import vfit64 as v64

H = 64
LR, BETAS, EPS = 3e-4, (0.9, 0.999), 1e-8        # the learners' pi_lr and torch.optim.Adam's defaults
CLIP = 0.2
ALLOWED = 4.0                                    # x the learners' float32 error: the project's allowance
DECIDABLE = l64.DECIDABLE
EDGE = 1e-5                                      # no row's ratio within this (relative) of 1 +- clip_ratio
LOSSES = (("ratio", CLIP), ("ratio", None), ("logp", None))      # ppo, espo, a2c
GRAD_MISTAKES = ("clip_by_ratio_alone",)
LOOP_MISTAKES = ("threshold_1p5", "stop_after_step", "step_counted_on_stop", "bias_restarts", "trace_past_stop")
TRACES = ("loss", "kl", "cf")


def forward64(theta, batch):
    """(logp, ratio) per row, float64: pgrad64.grad64's forward"""
    o = np.asarray(batch["obs"], dtype=np.float64)
    act, lpo = (np.asarray(batch[k], dtype=np.float64) for k in ("act", "logp"))
    ls, W1, b1, W2, b2, W3, b3 = f64.unpack(np.asarray(theta, dtype=np.float64), o.shape[1], act.shape[1], H)
    mu = np.tanh(np.tanh(o @ W1.T + b1) @ W2.T + b2) @ W3.T + b3
    da = act - mu
    logp = (-(da * da) / (2.0 * np.exp(2.0 * ls)) - ls - p64.HALF_LOG_2PI).sum(1)
    return logp, np.exp(logp - lpo)


def grad64(theta, batch, clip_ratio=CLIP, loss="ratio", mistake=None):
    """-> (g (P,), dict(loss, kl, cf, ent), ratio (B,)).  The backward is pgrad64.grad64's, whose row weight is -adv ratio / B:
    it is handed adv active ('ratio') or adv / ratio ('logp') as adv.  `mistake`: a planted one (GRAD_MISTAKES)"""
    assert loss in ("ratio", "logp") and (loss == "ratio" or clip_ratio is None)
    assert mistake is None or mistake in GRAD_MISTAKES
    adv, lpo = (np.asarray(batch[k], dtype=np.float64) for k in ("adv", "logp"))
    logp, ratio = forward64(theta, batch)
    cf, active = 0.0, np.ones_like(adv)
    if loss == "logp":
        value, weight = -(logp * adv).mean(), adv / ratio
    else:
        terms = ratio * adv
        if clip_ratio is not None:
            lo, hi = 1.0 - clip_ratio, 1.0 + clip_ratio
            terms = np.minimum(terms, np.clip(ratio, lo, hi) * adv)
            out = (ratio > hi) | (ratio < lo)
            cf = float(out.mean())
            cut = out if mistake == "clip_by_ratio_alone" else ((adv > 0) & (ratio > hi)) | ((adv < 0) & (ratio < lo))
            active = np.where(cut, 0.0, 1.0)
        value, weight = -terms.mean(), adv * active
    g, means = p64.grad64(theta, dict(obs=batch["obs"], act=batch["act"], logp=batch["logp"], adv=weight))
    return g, dict(loss=float(value), kl=float((lpo - logp).mean()), cf=cf, ent=means["ent"]), ratio


def fit64(theta, batch, iters, target_kl=None, clip_ratio=CLIP, loss="ratio", state=None, lr=LR, betas=BETAS, eps=EPS, mistake=None):
    """The learners' loop in float64 -> dict(thetas: the parameters after 0, 1, ... steps of this call (steps + 1 entries),
    theta: the last of them, loss / kl / cf: (iters,) traces, entry i at the parameters before step i and NaN past the stopping
    iteration, stop_iter: the iteration that stopped, else iters - 1, steps, ent (at the first parameters; None for iters = 0),
    state = dict(m, v, step) to hand to the next call (a new optimizer when None)).  `mistake`: a planted one (LOOP_MISTAKES)"""
    assert mistake is None or mistake in LOOP_MISTAKES
    theta = np.asarray(theta, dtype=np.float64)
    st = dict(state) if state is not None else v64.new_state(theta.size)
    tr = {k: np.full(iters, np.nan) for k in TRACES}
    thetas, steps, stop_iter, ent, stopped = [theta], 0, iters - 1, None, False
    for i in range(iters):
        g, info, _ = grad64(theta, batch, clip_ratio, loss)
        ent = info["ent"] if i == 0 else ent
        for k in TRACES:
            tr[k][i] = info[k]
        stopped = target_kl is not None and info["kl"] > (1.5 if mistake == "threshold_1p5" else 1.0) * target_kl
        if stopped and mistake != "stop_after_step":
            stop_iter = i
            st["step"] += mistake == "step_counted_on_stop"
            break
        st["step"] += 1
        steps += 1
        t = steps if mistake == "bias_restarts" else st["step"]
        theta, st["m"], st["v"] = v64.adam64(theta, st["m"], st["v"], g, t, lr, betas, eps)
        thetas.append(theta)
        if stopped:
            stop_iter = i
            break
    if mistake == "trace_past_stop" and stopped and stop_iter + 1 < iters:
        info = grad64(theta, batch, clip_ratio, loss)[1]
        for k in TRACES:
            tr[k][stop_iter + 1] = info[k]
    return dict(thetas=thetas, theta=theta, stop_iter=stop_iter, steps=steps, ent=ent, state=st, **tr)


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch), in the dtype asked for
# ---------------------------------------------------------------------------------------------------------------------
def learners_loss(pi, data, clip_ratio, loss):
    """compute_loss_pi of ppo (ppo_one_episode/ppo.py:268-284), espo (clip_ratio None; espo.py:255-269) and a2c ('logp';
    a2c.py:266-278), over tensors of pi's dtype -> (loss_pi, dict(kl, cf)) with the learners' .item()s"""
    import torch
    from torch.distributions.normal import Normal
    obs, act, adv, logp_old = data['obs'], data['act'], data['adv'], data['logp']
    logp = Normal(pi.mu_net(obs), torch.exp(pi.log_std)).log_prob(act).sum(axis=-1)
    ratio = torch.exp(logp - logp_old)
    cf = 0.0
    if loss == "logp":
        loss_pi = -(logp * adv).mean()
    elif clip_ratio is None:
        loss_pi = -(ratio * adv).mean()
    else:
        clip_adv = torch.clamp(ratio, 1 - clip_ratio, 1 + clip_ratio) * adv
        loss_pi = -(torch.min(ratio * adv, clip_adv)).mean()
        clipped = ratio.gt(1 + clip_ratio) | ratio.lt(1 - clip_ratio)
        cf = torch.as_tensor(clipped, dtype=torch.float32).mean().item()
    return loss_pi, dict(kl=(logp_old - logp).mean().item(), cf=cf)


def learners_gradient(pi, theta, batch, clip_ratio, loss, dtype):
    """one zero_grad / backward of the learners' loss in `dtype` -> (g, loss, kl, cf) as float64 numpy / floats"""
    import torch
    tmp = copy.deepcopy(pi).to(dtype)
    l64.assign_flat(tmp, np.asarray(theta))
    data = {k: torch.from_numpy(np.array(batch[k])).to(dtype) for k in ("obs", "act", "adv", "logp")}
    loss_pi, info = learners_loss(tmp, data, clip_ratio, loss)
    g = torch.autograd.grad(loss_pi, list(tmp.parameters()))
    return torch.cat([x.reshape(-1) for x in g]).double().numpy(), loss_pi.item(), info["kl"], info["cf"]


def learners_loop(pi, theta, batch, iters, target_kl=None, clip_ratio=CLIP, loss="ratio", carry=None, dtype=None, lr=LR):
    """The loop the learners run (ppo.py:307-316 with the `kl > target_kl: break`; StopIter = i after it) in `dtype` (torch
    dtype, default float64) around torch.optim.Adam, on a copy of `pi` holding `theta` -- or, with `carry` (what an earlier
    call returned as its second value), on that call's actor and optimizer, as an epoch follows an epoch.
    -> (dict as fit64's without state and ent, carry)"""
    import torch
    dtype = dtype or torch.float64
    if carry is None:
        tmp = copy.deepcopy(pi).to(dtype)
        l64.assign_flat(tmp, np.asarray(theta))
        carry = (tmp, torch.optim.Adam(tmp.parameters(), lr=lr))
    tmp, opt = carry
    data = {k: torch.from_numpy(np.array(batch[k])).to(dtype) for k in ("obs", "act", "adv", "logp")}
    flat = lambda: torch.cat([p.detach().reshape(-1) for p in tmp.parameters()]).double().numpy().copy()     # noqa: E731
    tr = {k: np.full(iters, np.nan) for k in TRACES}
    thetas, steps, i = [flat()], 0, -1
    for i in range(iters):
        opt.zero_grad()
        loss_pi, info = learners_loss(tmp, data, clip_ratio, loss)
        tr["loss"][i], tr["kl"][i], tr["cf"][i] = loss_pi.item(), info["kl"], info["cf"]
        if target_kl is not None and info["kl"] > target_kl:
            break
        loss_pi.backward()
        opt.step()
        steps += 1
        thetas.append(flat())
    return dict(thetas=thetas, theta=thetas[-1], stop_iter=i, steps=steps, **tr), carry


# ---------------------------------------------------------------------------------------------------------------------
# comparisons
# ---------------------------------------------------------------------------------------------------------------------
def same_trace(got, want):
    """the largest absolute difference of two traces whose NaN entries sit in the same places; inf where they do not"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    if got.shape != want.shape or (np.isnan(got) != np.isnan(want)).any():
        return float("inf")
    ok = ~np.isnan(want)
    return float(np.max(np.abs(got[ok] - want[ok]))) if ok.any() else 0.0


def loop_difference(got, want):
    """the largest of: the loss and kl traces' absolute differences, the relative L2 of the parameters after every step, and inf
    where stop_iter, steps, the number of recorded parameter vectors or an entry of cf differ (cf to 1e-7: the learners' is a
    float32 mean of zeros and ones, and a row counted otherwise moves it by 1 / B)"""
    if (got["stop_iter"], got["steps"], len(got["thetas"])) != (want["stop_iter"], want["steps"], len(want["thetas"])):
        return float("inf")
    if same_trace(got["cf"], want["cf"]) > 1e-7:
        return float("inf")
    d = [same_trace(got[k], want[k]) for k in TRACES[:2]]
    d += [f64.rel_l2(a, b) for a, b in zip(got["thetas"], want["thetas"])]
    return max(d)


# ---------------------------------------------------------------------------------------------------------------------
# cases, computed once per process and never written to
# ---------------------------------------------------------------------------------------------------------------------
# where logp_old is moved to, by the rank of a row's adv within its sign, cycling: four rows inside the range, three whose ratio
# is above it, three below (ratio = exp(-shift) at the first parameters)
PATTERN = ("in", "in", "up", "down", "in", "up", "down", "in", "up", "down")
ADV_SCALE = 1.5
GROUP_SHARE, INSIDE_SHARE = 0.10, 0.30


def shifted(batch, seed):
    """`batch` with logp_old moved off the actor's own logp and adv scaled: ratio starts inside [0.87, 1.13] on four rows in
    ten, in [1.27, 1.8] on three and in [0.55, 0.77] on three, whatever the sign of adv (tests/test_pifit64.py asserts the
    shares)"""
    rng = np.random.default_rng(900 + seed)
    adv = np.asarray(batch["adv"], dtype=np.float64)
    B = adv.size
    log_ratio = np.zeros(B)
    for sign in (adv > 0, adv <= 0):
        rows = np.flatnonzero(sign)
        rows = rows[np.argsort(adv[rows], kind="stable")]
        for n, r in enumerate(rows):
            kind = PATTERN[n % len(PATTERN)]
            log_ratio[r] = {"in": rng.uniform(np.log(0.87), np.log(1.13)), "up": rng.uniform(np.log(1.27), np.log(1.8)),
                            "down": rng.uniform(np.log(0.55), np.log(0.77))}[kind]
    out = dict(batch, logp=(np.asarray(batch["logp"], dtype=np.float64) - log_ratio).astype(np.float32),
               adv=(ADV_SCALE * adv).astype(np.float32))
    for k in ("logp", "adv"):
        out[k].setflags(write=False)
    return out


def shares(ratio, adv, clip_ratio=CLIP):
    """dict(up_pos, up_neg, down_pos, down_neg, inside): the share of the rows in each"""
    up, down = ratio > 1.0 + clip_ratio, ratio < 1.0 - clip_ratio
    pos = np.asarray(adv) > 0
    return dict(up_pos=float((up & pos).mean()), up_neg=float((up & ~pos).mean()), down_pos=float((down & pos).mean()),
                down_neg=float((down & ~pos).mean()), inside=float((~up & ~down).mean()))


def edge_distance(ratio, clip_ratio=CLIP):
    """the smallest relative distance of a row's ratio from 1 - clip_ratio or 1 + clip_ratio"""
    return float(min(np.min(np.abs(ratio / (1.0 + clip_ratio) - 1.0)), np.min(np.abs(ratio / (1.0 - clip_ratio) - 1.0))))


GRAD_ROWS = (1, 63, 64, 65, 257)
GRAD_WIDTHS = (43, 44, 64)
GRAD_CANDIDATES = (0, 1, 2, 3)
MEANS_TOL = 1e-5        # loss, kl against float64: some 100 float32 ulp of a row's logp, of order 1, as tests/test_gpu_pgrad.py holds its means
# regime, D, A, B: every shape tests/test_gpu_pifit.py takes a gradient at
SHAPES = tuple([("default", D, 2, B) for D in GRAD_WIDTHS for B in GRAD_ROWS] + [("default", 43, 2, 16385)] +
               [("default", D, 2, v64.EDGE_ROWS) for D in p64.EDGE_WIDTHS] + [("default", 43, 8, 130), ("default", 43, 10, 130)] +
               [("trained", 43, 2, 257), ("saturated", 43, 2, 257)])
# seeds whose ratio comes within EDGE of 1 +- clip_ratio on some row, kept out by name (tests/test_pifit64.py)
GRAD_KEPT_OUT = {}


def grad_seeds(regime, D, A, B):
    return tuple(s for s in GRAD_CANDIDATES if s not in GRAD_KEPT_OUT.get((regime, D, A, B), ()))


def grad_yardstick(regime, D, A, B, clip_ratio=CLIP, loss="ratio"):
    """(whole, {block: error}): grad_errors of the learners' float32 autograd pooled over grad_seeds"""
    return p64.pool([gradient_case(regime, D, A, B, s, clip_ratio, loss)["yard"] for s in grad_seeds(regime, D, A, B)])

FIT_SHAPES = ((43, 257), (64, 130))                         # D, B
FIT_CANDIDATES = (0, 1, 2, 3, 4, 5, 6, 7)
# Seeds kept out by name, and the condition each fails (tests/test_pifit64.py: test_the_fit_seeds_are_decidable shows that it does
# and that the others pass all three).  "edge": a row's float64 ratio comes within EDGE of 1 +- clip_ratio at a compared
# iteration, so that float32 may count it on the other side.  "spread": the float32 loop's own displacement error is more than
# SPREAD x the median over the candidates.  Such a seed has an entry of g within a few times Adam's eps = 1e-8 of zero (the rest
# are 1e-4 and up), where the step lr g / (|g| + eps) turns on the last bits of g: one entry in 7000 carries the whole error
# (8 x to 400 x the median), and a comparison on it measures that entry's lottery and not the method -- pgrad64's rule, for
# vfit64's reason.
FIT_KEPT_OUT = {(43, 257): {1: "spread", 2: "spread", 3: "edge"}, (64, 130): {1: "edge", 3: "edge", 5: "spread", 6: "spread"}}
SPREAD = p64.SPREAD
FIT_KS = (1, 2, 3, 10)
MID = 3                                                     # the mid-loop stop


def fit_seeds(D, B):
    return tuple(s for s in FIT_CANDIDATES if s not in FIT_KEPT_OUT[D, B])


@functools.lru_cache(maxsize=None)
def gradient_case(regime, D, A, B, seed, clip_ratio=CLIP, loss="ratio"):
    """dict(pi, theta, batch, g, info (float64 oracle), ratio, edge: its edge_distance, learners: the float32 loss, kl and cf,
    yard: grad_errors of the learners' float32 autograd)"""
    import torch
    pi, theta, batch = l64.make_batch(regime, D, A, B, seed, adc=False)
    batch = shifted(batch, seed)
    g, info, ratio = grad64(theta, batch, clip_ratio, loss)
    lg, ll, lk, lc = learners_gradient(pi, theta, batch, clip_ratio, loss, torch.float32)
    g.setflags(write=False)
    return dict(pi=pi, theta=theta, batch=batch, g=g, info=info, ratio=ratio, learners=dict(loss=ll, kl=lk, cf=lc),
                edge=edge_distance(ratio, clip_ratio) if clip_ratio is not None else 1.0, yard=p64.grad_errors(lg, g, D, A))


def trace_errors(got, want, scale, k):
    """the largest error of the first k entries of the loss trace and of the kl trace, relative to `scale` = (mean |ratio adv|,
    mean |logp_old - logp|) at the first parameters: both are means of terms of either sign, and kl passes through zero on
    some seeds"""
    return (max(abs(got["loss"][i] - want["loss"][i]) / scale[0] for i in range(k)),
            max(abs(got["kl"][i] - want["kl"][i]) / scale[1] for i in range(k)))


def fit_errors(run, ref, scale):
    """{("theta", k): relative L2 of the displacement theta_k - theta_0, ("loss", k), ("kl", k): trace_errors} against the
    float64 `ref`, k in FIT_KS; `run`: dict(thetas, loss, kl) of ten unstopped iterations"""
    errs = {}
    for k in FIT_KS:
        errs["theta", k] = f64.rel_l2(np.asarray(run["thetas"][k], np.float64) - ref["thetas"][0], ref["thetas"][k] - ref["thetas"][0])
        errs["loss", k], errs["kl", k] = trace_errors(run, ref, scale, k)
    return errs


def pool_fits(errs):
    return {key: f64.pooled([e[key] for e in errs]) for key in errs[0]}


@functools.lru_cache(maxsize=None)
def fit_case(D, B, seed, clip_ratio=CLIP, loss="ratio"):
    """dict(pi, theta, batch, ref: fit64 over max(FIT_KS) unstopped iterations, states[k]: the optimizer's state after k steps,
    scale, f32: the learners' float32 loop over the same, yard: its fit_errors, kl_err: its largest absolute kl error,
    edge: the smallest edge_distance over the iterations compared, targets: {0, MID, None: a target_kl that stops there})"""
    import torch
    pi, theta, batch = l64.make_batch("default", D, 2, B, seed, adc=False)
    batch = shifted(batch, seed)
    n = max(FIT_KS)
    ref = fit64(theta, batch, n + 1, None, clip_ratio, loss)     # one more evaluation: kl at the parameters after n steps
    states, st, th = [v64.new_state(theta.size)], None, theta
    for _ in range(n):
        r = fit64(th, batch, 1, None, clip_ratio, loss, state=st)
        st, th = r["state"], r["theta"]
        states.append(st)
    adv = np.asarray(batch["adv"], dtype=np.float64)
    logp0, ratio0 = forward64(theta, batch)
    scale = (float(np.abs(ratio0 * adv).mean()), float(np.abs(np.asarray(batch["logp"], dtype=np.float64) - logp0).mean()))
    f32, _ = learners_loop(pi, theta, batch, n, None, clip_ratio, loss, dtype=torch.float32)
    yard = fit_errors(f32, ref, scale)
    kl_err = max(abs(f32["kl"][i] - ref["kl"][i]) for i in range(n))
    edge = min(edge_distance(forward64(t, batch)[1], clip_ratio) for t in ref["thetas"]) if clip_ratio is not None else 1.0
    kl = ref["kl"]
    targets = {0: 0.5 * kl[0] if kl[0] > 0 else 2.0 * kl[0], MID: 0.5 * (max(kl[:MID]) + kl[MID]),
               None: max(kl) + max(1.0, abs(max(kl)))}
    return dict(pi=pi, theta=theta, batch=batch, ref=ref, states=states, scale=scale, f32=f32, yard=yard, kl_err=kl_err, edge=edge,
                targets=targets)


def stop_margin(case, where):
    """how far the case's target_kl for a stop at `where` (0, MID, None) sits from the oracle's kl entries on either side of
    the decision, in units of the float32 loop's kl error: (the nearest entry that must not stop, the entry that must)"""
    kl, tkl = case["ref"]["kl"], case["targets"][where]
    n = max(FIT_KS)
    last = n if where is None else where
    below = min((tkl - kl[i]) for i in range(last)) if last > 0 else float("inf")
    above = (kl[last] - tkl) if where is not None else float("inf")
    return below / case["kl_err"], above / case["kl_err"]


def fit_spread(D, B):
    """{seed: the larger of its float32 displacement yardsticks' (k = 1 and k = 10) factors over the median of FIT_CANDIDATES}"""
    yards = {s: fit_case(D, B, s)["yard"] for s in FIT_CANDIDATES}
    med = {k: float(np.median([y["theta", k] for y in yards.values()])) for k in (1, max(FIT_KS))}
    return {s: max(yards[s]["theta", k] / med[k] for k in med) for s in FIT_CANDIDATES}


@functools.lru_cache(maxsize=None)
def fit_yardstick(D, B):
    """the learners' float32 loop's fit_errors, pooled over fit_seeds"""
    return pool_fits([fit_case(D, B, s)["yard"] for s in fit_seeds(D, B)])
