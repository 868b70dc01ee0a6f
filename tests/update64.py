"""A whole epoch of the TRPO family's update() in float64, composed of the stages' oracles: pgrad64.grad64 -> fisher64.fvp64 and
cg64 -> (cpo: pgrad64.cpo_direction64) -> linesearch64.search64 -> vfit64.fit64 for the critics (trpo_update64, cpo_update64,
critics64).  Nothing is restated here; what this file adds is the order of the stages, what crosses from one to the next
(g, b and x_direction are rounded once to float32 there, as on the device, so that the search runs on the vector the
device's search would be given) and the state an epoch hands to the next.  The oracle of tests/test_update64.py (which checks
it against the learners' formulation in torch float64 and plants mistakes at the seams) and of tests/test_gpu_update.py.

Also the yardstick (learners_update32: the same epoch the way the learners run it, float32 torch on the CPU), the distance of
every branch test of CPO's ladder from its threshold (ladder_margins, the sibling of linesearch64.margins) and the sequences
of epochs the CPU and the GPU tests share.

Vectors are in the order of pi.parameters() (log_std first) and of critic.parameters()."""
import copy
import functools
import math

import numpy as np

import fisher64 as f64
import linesearch64 as l64
import pgrad64 as p64
import vfit64 as v64

EPS = 1e-8
H = 64
ALLOWED = 4.0                                    # x the learners' float32 error: the project's allowance
DECIDABLE = l64.DECIDABLE
TARGET_KL, CG_ITERS, COEFF, ITERS, V_ITERS = 0.01, 10, 0.8, 20, 5
COST_REDUCTION = 0.0                             # the learners' default
HYPER = dict(target_kl=TARGET_KL, cg_iters=CG_ITERS, coeff=COEFF, iters=ITERS)

# the mistakes tests/test_update64.py plants, each a keyword of the oracle (the first two as fisher_theta and search_theta)
MISTAKES = ("fisher_at_previous_theta", "search_from_previous_theta", "moments_zeroed", "step_restarts", "need_loss_always",
            "margin_without_max", "second_solve_on_g", "ret_for_cost_ret")


def f32(v):
    return np.asarray(v, dtype=np.float64).astype(np.float32)


def _solve(Hx, rhs, cg_iters):
    """the learners' cg and x' H x"""
    x, _, _ = f64.cg64(Hx, rhs, iters=cg_iters)
    return x, float(x @ Hx(x))


def _fisher(theta, batch, damping):
    obs, A = np.asarray(batch["obs"]), np.asarray(batch["act"]).shape[1]
    return lambda v: f64.fvp64(theta, v, obs, A, damping=damping)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle
# ---------------------------------------------------------------------------------------------------------------------
def trpo_update64(theta, batch, target_kl=TARGET_KL, cg_iters=CG_ITERS, damping=0.0, coeff=COEFF, iters=ITERS, *,
                  fisher_theta=None, search_theta=None):
    """trpo's update() from buf.get() to the assignment -> dict(g, x (both float32), x64 (x before its rounding), s, accepted,
    theta_new, trace, means (the four at theta_new), ginfo (grad64's means), search (search64's result)).  The keywords plant
    mistakes: the Fisher matrix taken at `fisher_theta`, the search run from `search_theta`."""
    g = f32(p64.grad64(theta, batch)[0])
    ginfo = p64.grad64(theta, batch)[1]
    Hx = _fisher(theta if fisher_theta is None else fisher_theta, batch, damping)
    x_hat, s = _solve(Hx, g, cg_iters)
    x64 = math.sqrt(2.0 * target_kl / (s + EPS)) * x_hat
    x = f32(x64)
    srch = l64.search64(theta if search_theta is None else search_theta, x, batch, target_kl, 0.0, 1, coeff, iters)
    return dict(g=g, x=x, x64=x64, s=s, accepted=srch["accepted"], theta_new=srch["theta_new"], trace=srch["trace"],
                means=srch["means"], ginfo=ginfo, search=srch, need_loss=1, cost_margin=0.0)


def cpo_update64(theta, batch, c, cost_reduction=COST_REDUCTION, target_kl=TARGET_KL, cg_iters=CG_ITERS, damping=0.0, coeff=COEFF,
                 iters=ITERS, *, fisher_theta=None, search_theta=None, need_loss_always=False, margin_without_max=False,
                 second_solve_on_g=False):
    """cpo's update() from buf.get() to the assignment -> trpo_update64's dict and b, optim_case, lam, nu, f_a_wins, need_loss,
    cost_margin = max(-c, -cost_reduction) and ladder (cpo_direction64's whole result).  The keywords plant mistakes."""
    c = float(c)
    g64, ginfo = p64.grad64(theta, batch)
    g, b = f32(g64), f32(p64.grad64(theta, batch, cost=True)[0])
    Hx = _fisher(theta if fisher_theta is None else fisher_theta, batch, damping)
    Hinv_g, _ = _solve(Hx, g, cg_iters)
    approx_g = Hx(Hinv_g)
    Hinv_b, s = _solve(Hx, g if second_solve_on_g else b, cg_iters)
    lad = p64.cpo_direction64(b, Hinv_g, Hinv_b, approx_g, s, c, target_kl)
    x = f32(lad["x"])
    need_loss = 1 if need_loss_always else int(lad["optim_case"] > 1)
    cost_margin = -c if margin_without_max else max(-c, -float(cost_reduction))
    srch = l64.search64(theta if search_theta is None else search_theta, x, batch, target_kl, cost_margin, need_loss, coeff, iters)
    return dict(g=g, b=b, x=x, x64=lad["x"], s=s, accepted=srch["accepted"], theta_new=srch["theta_new"], trace=srch["trace"],
                means=srch["means"], ginfo=ginfo, search=srch, optim_case=lad["optim_case"], lam=lad["lam"], nu=lad["nu"],
                f_a_wins=lad["f_a_wins"], need_loss=need_loss, cost_margin=cost_margin, ladder=lad, c=c)


def critics64(theta_v, state_v, theta_vc, state_vc, batch, iters=V_ITERS, *, moments_zeroed=False, step_restarts=False,
              ret_for_cost_ret=False):
    """the closing block of update(): fit64 of v on ret and, where theta_vc is given, of vc on cost_ret, each from its own
    optimizer state (None: a new optimizer) -> dict(v=dict(theta, losses, state), vc=... or None).  The keywords plant
    mistakes: Adam's moments zeroed before the call, its step count restarted, ret fitted by vc."""
    obs = np.asarray(batch["obs"])

    def one(theta, state, ret):
        st = dict(state) if state is not None else v64.new_state(np.asarray(theta).size)
        if moments_zeroed:
            st.update(m=np.zeros_like(st["m"]), v=np.zeros_like(st["v"]))
        thetas, losses, st = v64.fit64(theta, obs, np.asarray(ret), iters, state=st, mistake="step_restarts" if step_restarts else None)
        return dict(theta=thetas[-1], losses=losses, state=st)

    return dict(v=one(theta_v, state_v, batch["ret"]),
                vc=None if theta_vc is None else one(theta_vc, state_vc, batch["ret" if ret_for_cost_ret else "cost_ret"]))


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch), in the dtype asked for: float32 is the yardstick, float64 what the oracle is checked against
# ---------------------------------------------------------------------------------------------------------------------
def learners_update32(pi, theta, batch, c=None, cost_reduction=COST_REDUCTION, target_kl=TARGET_KL, cg_iters=CG_ITERS, damping=0.0,
                      coeff=COEFF, iters=ITERS, dtype=None, given=None):
    """The epoch the way the learners run it (trpo.py and cpo.py's update() up to the assignment; cpo with `c`): auto_grad for
    g and b (pgrad64.learners_gradient), the double backward for Hx (fisher64.autograd_fvp) inside the learners' cg, the dots
    and the ladder on host scalars, the search over linesearch64.learners_means with linesearch64.accepts.  `dtype`: float32
    (the default) is the learners' own run, with their float32 numpy vectors (fisher64.learners_cg32); float64 is their
    formulation in float64 (fisher64.cg64 around the same double backward).  `given`: dict(g, b, x), what crosses a stage
    boundary, to go on from in place of what was computed (the float64 check hands over the oracle's rounded ones, so that
    no entry's rounding can differ and a stage is compared on the input the oracle's stage had).  -> the keys of cpo_update64's dict that have a counterpart."""
    import torch
    dtype = dtype or torch.float32
    single = dtype == torch.float32
    nt = np.float32 if single else np.float64
    cpo = c is not None
    tmp = copy.deepcopy(pi).to(dtype)
    l64.assign_flat(tmp, np.asarray(theta))
    obs = torch.from_numpy(np.array(batch["obs"])).to(dtype)
    Hx = lambda v: f64.autograd_fvp(tmp, obs, torch.from_numpy(np.ascontiguousarray(v, dtype=nt))).numpy() + nt(damping) * v   # noqa: E731
    cg = (lambda rhs: f64.learners_cg32(Hx, rhs, cg_iters)) if single else (lambda rhs: f64.cg64(Hx, rhs, iters=cg_iters)[0])
    given = given or {}
    g = p64.learners_gradient(pi, theta, batch, False, dtype).astype(nt)
    out = dict(g=g)
    g = np.asarray(given.get("g", g), dtype=nt)
    if cpo:
        b = p64.learners_gradient(pi, theta, batch, True, dtype).astype(nt)
        out.update(b=b)
        b = np.asarray(given.get("b", b), dtype=nt)
        Hinv_g = cg(g)
        approx_g = Hx(Hinv_g)
        Hinv_b = cg(b)
        dots = dict(q=np.dot(Hinv_g, approx_g), r=np.dot(Hinv_b, approx_g), bb=np.dot(b, b))
        s = np.dot(Hinv_b, Hx(Hinv_b))
        lad = p64.cpo_direction64(b, Hinv_g, Hinv_b, approx_g, s, float(c), target_kl, dots=dots)    # the ladder on Python floats
        x = lad["x"].astype(nt)
        need_loss, cost_margin = int(lad["optim_case"] > 1), max(-float(c), -float(cost_reduction))
        out.update(optim_case=lad["optim_case"], lam=lad["lam"], nu=lad["nu"], f_a_wins=lad["f_a_wins"], ladder=lad, c=float(c))
    else:
        x_hat = cg(g)
        s = np.dot(x_hat, Hx(x_hat))
        x = (np.sqrt(2.0 * target_kl / (s + EPS)) * x_hat).astype(nt)
        need_loss, cost_margin = 1, 0.0
    d = np.asarray(given.get("x", x))
    th = np.asarray(theta, dtype=np.float32)
    step = (lambda t: th - t * d) if single and "x" not in given else (lambda t: l64.candidate(th, d, t))
    old = l64.learners_means(pi, th, batch, dtype)
    accepted, theta_new, trace = -1, th.copy(), [old]
    for j in range(iters):
        cand = step(coeff ** j)
        m = l64.learners_means(pi, cand, batch, dtype)
        trace.append(m)
        if l64.accepts(m, old, target_kl, cost_margin, need_loss, cpo):
            accepted, theta_new = j, np.asarray(cand, dtype=np.float32)
            break
    out.update(x=x, s=float(s), accepted=accepted, theta_new=theta_new, trace=np.stack(trace), need_loss=need_loss,
               cost_margin=cost_margin)
    return out


def learners_fit(critic, optimizer, theta, state, obs, ret, iters=V_ITERS):
    """vfit64.learners_loop on `critic` (in its dtype) with its one torch.optim.Adam, both first set to `theta` and to
    `state` = dict(m, v, step) in place (None: left as they are) -> (theta after the loop, the losses)"""
    import torch
    dtype = next(critic.parameters()).dtype
    v64.assign_flat(critic, np.asarray(theta))
    if state is not None:
        at = 0
        for p in critic.parameters():
            n = p.numel()
            part = lambda k: torch.from_numpy(np.array(state[k][at:at + n])).reshape(p.shape).to(dtype).clone()   # noqa: E731
            optimizer.state[p] = dict(step=torch.tensor(float(state["step"])), exp_avg=part("m"), exp_avg_sq=part("v"))
            at += n
    t = lambda a: torch.from_numpy(np.array(a)).to(dtype)       # noqa: E731
    thetas, losses, _ = v64.learners_loop(critic, t(obs), t(ret), iters, optimizer=optimizer)
    return thetas[-1], losses


def ladder_margins(ref, learn):
    """linesearch64.margins for the ladder: for every branch test the oracle's ladder evaluated (ref = cpo_update64's result),
    the distance from the threshold in float64 over the absolute error of the same quantity in learners_update32's run
    (learn) -> list of (what, ratio); an error of exactly 0 (c is handed to both as it is) gives inf."""
    a, b = ref["ladder"], learn["ladder"]
    ratio = lambda dist, err: (math.inf if dist != 0.0 else 0.0) if err == 0.0 else abs(dist) / abs(err)       # noqa: E731
    out = [("b.b <= 1e-8", ratio(a["bb"] - 1e-8, b["bb"] - a["bb"])), ("c < 0", ratio(ref["c"], learn["c"] - ref["c"]))]
    if a["optim_case"] != 4:
        out.append(("B >= 0", ratio(a["B"], b["B"] - a["B"])))
    if a["optim_case"] in (1, 2) and b["f_a"] is not None:
        out.append(("f_a >= f_b", ratio(a["f_a"] - a["f_b"], (b["f_a"] - b["f_b"]) - (a["f_a"] - a["f_b"]))))
    return out


def search_margins(epoch):
    """linesearch64.margins of the epoch's search: list of (j, what, ratio)"""
    ref = epoch["ref"]
    kw = dict(target_kl=TARGET_KL, cost_margin=ref["cost_margin"], need_loss=ref["need_loss"], coeff=COEFF, iters=ITERS)
    return l64.margins(dict(pi=epoch["pi"], theta=epoch["theta"], d=ref["x"], batch=epoch["batch"], kw=kw, ref=ref["search"]))


# ---------------------------------------------------------------------------------------------------------------------
# the sequences, computed once per process and never written to
# ---------------------------------------------------------------------------------------------------------------------
# name -> learner, regime, damping, D, A, the rows and c of every epoch, the seed.  Rows shrink and then grow past the first:
# stale partials in a kept workspace, then a workspace regrown with launches still queued.  D = 96 is the width from which b
# is a second pass.  c reaches optim_case 2, 1, 3 (and 1, 2, 0 in cpo_wide): tests/test_update64.py asserts it.
# The seeds are chosen for decidability (a condition on the inputs, asserted in tests/test_update64.py): seed 0 for the damped
# sequences (every threshold at least 975 float32 errors away); undamped, seed 0 leaves f_a >= f_b 47 float32 errors from a
# tie in cpo_default, so trpo_default takes seed 4 (accepted = 1, 0, 2, margins from 5.6e3) and cpo_default seed 8 (the
# first of 0 .. 15 with every margin above 1e4).
# The float32 learners' error of x_direction per epoch, and its spread about the median (tests/test_update64.py prints them;
# one CPU, they move with the BLAS):
#   trpo_default  3.7e-05 1.7e-04 5.3e-05  (3.19 x)     undamped: a ten-step float32 CG on an undamped Fisher matrix is a
#   cpo_default   1.1e-05 2.0e-06 8.4e-05  (7.44 x)     lottery the reference shares; recorded, not asserted
#   trpo_trained  2.2e-06 2.2e-06 2.4e-06  (1.12 x)     damped: asserted within pgrad64.SPREAD = 3 x
#   cpo_trained   2.2e-06 5.2e-06 2.4e-06  (2.18 x)
#   cpo_wide      1.3e-06 1.2e-06 1.2e-06  (1.05 x)
SEQUENCES = {
    "trpo_default": dict(learner="trpo", regime="default", damping=0.0, D=43, A=2, rows=(257, 130, 321), c=(None, None, None), seed=4),
    "trpo_trained": dict(learner="trpo", regime="trained", damping=0.1, D=43, A=2, rows=(257, 130, 321), c=(None, None, None), seed=0),
    "cpo_default": dict(learner="cpo", regime="default", damping=0.0, D=43, A=2, rows=(257, 130, 321), c=(-0.01, 0.02, -1.0), seed=8),
    "cpo_trained": dict(learner="cpo", regime="trained", damping=0.1, D=43, A=2, rows=(257, 130, 321), c=(-0.01, 0.02, -1.0), seed=0),
    "cpo_wide": dict(learner="cpo", regime="default", damping=0.1, D=96, A=8, rows=(130, 65, 130), c=(0.02, -0.01, 3.0), seed=0),
    # for the objects kept across epochs (tests/test_gpu_update.py): cpo_trained at one row count throughout
    "cpo_trained_257": dict(learner="cpo", regime="trained", damping=0.1, D=43, A=2, rows=(257, 257, 257), c=(-0.01, 0.02, -1.0), seed=0),
}
COMPARED = ("trpo_default", "trpo_trained", "cpo_default", "cpo_trained", "cpo_wide")
EXPECTED_CASES = {"cpo_default": (2, 1, 3), "cpo_trained": (2, 1, 3), "cpo_wide": (1, 2, 0), "cpo_trained_257": (2, 1, 3)}
QUANTITIES = ("x", "disp", "v", "v_loss", "vc", "vc_loss")


def actor_at(pi, theta):
    """a copy of the float32 actor `pi` holding the flat parameters `theta`"""
    tmp = copy.deepcopy(pi)
    l64.assign_flat(tmp, np.asarray(theta))
    return tmp


def epoch_batch(pi, regime, D, A, B, seed, adc):
    """linesearch64.batch_of the actor `pi` over fresh obs of the regime (fisher64.problem's, under `seed`), and the critics'
    targets ret = 1 + 2 N(0, 1) and cost_ret = 0.5 + N(0, 1); numpy float32, read-only"""
    import torch
    obs = f64.problem(regime, D, A, B, seed)[1]
    batch = dict(l64.batch_of(pi, obs, seed, adc))
    gen = torch.Generator().manual_seed(700 + seed)
    batch["ret"] = (1.0 + 2.0 * torch.randn(B, generator=gen)).numpy()
    batch["cost_ret"] = (0.5 + torch.randn(B, generator=gen)).numpy()
    for k in ("ret", "cost_ret"):
        batch[k].setflags(write=False)
    return batch


def displacement_errors(theta, got, want):
    return f64.rel_l2(np.asarray(got, np.float64) - np.asarray(theta, np.float64), np.asarray(want, np.float64) - np.asarray(theta, np.float64))


def loss_errors(got, want):
    return max(v64.rel_err(a, b) for a, b in zip(got, want))


def stored(state):
    """an optimizer state as the device stores it: m and v rounded to float32"""
    return dict(m=f32(state["m"]), v=f32(state["v"]), step=int(state["step"]))


def oracle_epoch(spec, theta, batch, c, **mistakes):
    kw = dict(HYPER, damping=spec["damping"])
    return cpo_update64(theta, batch, c, COST_REDUCTION, **kw, **mistakes) if spec["learner"] == "cpo" else trpo_update64(theta, batch, **kw, **mistakes)


@functools.lru_cache(maxsize=None)
def sequence(name):
    """dict(spec, pi, v, vc (the float32 modules the sequence starts from; vc None for trpo), epochs): every epoch a dict of
    B, c, seed, pi and theta (the actor it starts from), theta_v, state_v, theta_vc, state_vc, batch (batch_of that actor
    over fresh obs, with ret and cost_ret), ref and crit (the oracle's update and critics), learn (learners_update32's
    result) and yard: the learners' float32 errors against the oracle, by QUANTITIES.  The next epoch starts from the
    oracle's results as the device would store them (float32)."""
    import torch
    spec = SEQUENCES[name]
    regime, D, A, seed, cpo = spec["regime"], spec["D"], spec["A"], spec["seed"], spec["learner"] == "cpo"
    pi0 = f64.problem(regime, D, A, 1, seed)[0]
    scale = v64.REGIMES[regime]["scale"]
    v0 = v64.make_critic(D, H, seed=seed + 10, scale=scale)
    vc0 = v64.make_critic(D, H, seed=seed + 20, scale=scale) if cpo else None
    theta = f64.flat(pi0).numpy().copy()
    theta_v, state_v = v64.flat(v0).numpy().copy(), stored(v64.new_state(v64.param_count(D)))
    theta_vc, state_vc = (v64.flat(vc0).numpy().copy(), stored(v64.new_state(v64.param_count(D)))) if cpo else (None, None)
    lv, lvc = copy.deepcopy(v0), copy.deepcopy(vc0)                          # the learners' critics, each with its one Adam
    opt_v = torch.optim.Adam(lv.parameters(), lr=v64.LR)
    opt_vc = torch.optim.Adam(lvc.parameters(), lr=v64.LR) if cpo else None
    epochs = []
    for e, (B, c) in enumerate(zip(spec["rows"], spec["c"])):
        pi = actor_at(pi0, theta)
        batch = epoch_batch(pi, regime, D, A, B, seed + 1 + e, cpo)
        ref = oracle_epoch(spec, theta, batch, c)
        crit = critics64(theta_v, state_v, theta_vc, state_vc, batch)
        learn = learners_update32(pi, theta, batch, c, COST_REDUCTION, damping=spec["damping"], **HYPER)
        yard = dict(x=f64.rel_l2(learn["x"], ref["x"]), disp=displacement_errors(theta, learn["theta_new"], ref["theta_new"]) if ref["accepted"] >= 0 and learn["accepted"] == ref["accepted"] else math.nan)
        for k, crt, opt, th_k, st_k, ret in (("v", lv, opt_v, theta_v, state_v, "ret"), ("vc", lvc, opt_vc, theta_vc, state_vc, "cost_ret")):
            if crt is not None:
                th32, losses = learners_fit(crt, opt, th_k, st_k, batch["obs"], batch[ret])
                yard[k] = displacement_errors(th_k, th32, crit[k]["theta"])
                yard[k + "_loss"] = loss_errors(losses, crit[k]["losses"])
        epochs.append(dict(B=B, c=c, seed=seed + 1 + e, pi=pi, theta=theta, theta_v=theta_v, state_v=state_v, theta_vc=theta_vc,
                           state_vc=state_vc, batch=batch, ref=ref, crit=crit, learn=learn, yard=yard))
        theta = ref["theta_new"]
        theta_v, state_v = f32(crit["v"]["theta"]), stored(crit["v"]["state"])
        if cpo:
            theta_vc, state_vc = f32(crit["vc"]["theta"]), stored(crit["vc"]["state"])
    return dict(spec=spec, name=name, pi=pi0, v=v0, vc=vc0, epochs=tuple(epochs))


def yardstick(name):
    """{quantity: the learners' float32 error, pooled (root-mean-square) over the sequence's epochs}"""
    eps = sequence(name)["epochs"]
    return {k: f64.pooled([e["yard"][k] for e in eps]) for k in QUANTITIES if k in eps[0]["yard"]}


def spread(name, k):
    """the largest distance of an epoch's yardstick `k` from the median over the sequence's epochs, as a factor >= 1"""
    ys = [e["yard"][k] for e in sequence(name)["epochs"]]
    med = float(np.median(ys))
    return max(math.exp(abs(math.log(y / med))) for y in ys)
