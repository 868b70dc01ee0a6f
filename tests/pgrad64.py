"""The surrogate gradients and CPO's step direction of include/guardx_pgrad.h in numpy float64 (grad64, cpo_direction64): the
oracle of tests/test_pgrad64.py (which checks it against float64 autograd of the learners' two losses and against a literal
transcription of the ladder), tests/test_reference_pgrad.py and tests/test_gpu_pgrad.py.  Also the learners' own gradient in
torch (in the precision it is asked for: the float32 one is the yardstick of the device's error) and the cases the CPU and the
GPU tests share.

Vectors are in the order of pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]."""
import copy
import functools
import math

import numpy as np

import fisher64 as f64
import linesearch64 as l64
import vfit64 as v64

EPS = 1e-8
H = 64
HALF_LOG_2PI = l64.HALF_LOG_2PI
ALLOWED = 4.0                                    # x the learners' float32 error: the project's allowance
BLOCKS = ("log_std",) + f64.BLOCKS
MISTAKES = ("ratio_is_one", "no_minus_one", "std_for_variance", "no_one_over_b", "log_std_last")


def block_slices(D, A):
    return dict(log_std=slice(0, A), **f64.block_slices(D, A, H))


def grad64(theta, batch, cost=False, mistake=None):
    """-> (gradient (P,), dict(pi_l, surr_cost, approx_kl, ent)): the header's closed form, float64 throughout.  cost: the
    gradient of surr_cost = mean(ratio adc) instead of loss_pi = -mean(ratio adv).  `mistake` plants one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    o = np.asarray(batch["obs"], dtype=np.float64)
    B, D = o.shape
    act, adv, lpo = (np.asarray(batch[k], dtype=np.float64) for k in ("act", "adv", "logp"))
    adc = np.asarray(batch["adc"], dtype=np.float64) if batch.get("adc") is not None else np.zeros_like(adv)
    A = act.shape[1]
    ls, W1, b1, W2, b2, W3, b3 = f64.unpack(np.asarray(theta, dtype=np.float64), D, A, H)
    h1 = np.tanh(o @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    mu = h2 @ W3.T + b3
    v1 = np.exp(ls) if mistake == "std_for_variance" else np.exp(2.0 * ls)
    da = act - mu
    logp = (-(da * da) / (2.0 * np.exp(2.0 * ls)) - ls - HALF_LOG_2PI).sum(1)
    ratio = np.exp(logp - lpo)
    means = dict(pi_l=-(ratio * adv).mean(), surr_cost=(ratio * adc).mean(), approx_kl=(lpo - logp).mean(),
                 ent=float((ls + 0.5 + HALF_LOG_2PI).sum()))
    r = np.ones_like(ratio) if mistake == "ratio_is_one" else ratio
    c = (adc if cost else -adv) * r / (1.0 if mistake == "no_one_over_b" else B)
    dls = (c[:, None] * (da * da / v1 - (0.0 if mistake == "no_minus_one" else 1.0))).sum(0)
    dmu = c[:, None] * da / v1
    dW3, db3 = dmu.T @ h2, dmu.sum(0)
    dz2 = (dmu @ W3) * (1.0 - h2 * h2)
    dW2, db2 = dz2.T @ h1, dz2.sum(0)
    dz1 = (dz2 @ W2) * (1.0 - h1 * h1)
    dW1, db1 = dz1.T @ o, dz1.sum(0)
    net = [dW1, db1, dW2, db2, dW3, db3]
    parts = net + [dls] if mistake == "log_std_last" else [dls] + net
    return np.concatenate([p.reshape(-1) for p in parts]), means


def learners_gradient(pi, theta, batch, cost, dtype):
    """the learners' auto_grad(loss_pi, ac.pi) / auto_grad(surr_cost, ac.pi) (trpo.py, cpo.py:445-446) in `dtype`: the flat
    gradient of the loss over Normal(mu_net(obs), exp(log_std)).log_prob(act).sum(-1), as float64 numpy"""
    import torch
    from torch.distributions.normal import Normal
    tmp = copy.deepcopy(pi).to(dtype)
    l64.assign_flat(tmp, np.asarray(theta))
    t = lambda k: torch.from_numpy(np.array(batch[k])).to(dtype)     # noqa: E731
    logp = Normal(tmp.mu_net(t("obs")), torch.exp(tmp.log_std)).log_prob(t("act")).sum(axis=-1)
    ratio = torch.exp(logp - t("logp"))
    loss = (ratio * t("adc")).mean() if cost else -(ratio * t("adv")).mean()
    g = torch.autograd.grad(loss, list(tmp.parameters()))
    return torch.cat([x.reshape(-1) for x in g]).double().numpy()


def grad_errors(got, want, D, A):
    """(the relative L2 of the whole vector, {block: its relative L2}); a block whose float64 value is zero reads 0"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    blocks = {}
    for k, sl in block_slices(D, A).items():
        n = np.linalg.norm(want[sl])
        blocks[k] = float(np.linalg.norm(got[sl] - want[sl]) / n) if n > 0 else 0.0
    return f64.rel_l2(got, want), blocks


def pool(errs):
    """root-mean-square over the seeds of a list of grad_errors"""
    whole = f64.pooled([e[0] for e in errs])
    return whole, {k: f64.pooled([e[1][k] for e in errs]) for k in errs[0][1]}


# ---------------------------------------------------------------------------------------------------------------------
# CPO's direction
# ---------------------------------------------------------------------------------------------------------------------
def cpo_direction64(b, Hinv_g, Hinv_b, approx_g, s, c, target_kl, dots=None):
    """The header's ladder on numpy float64: -> dict(optim_case, lam, nu, q, r, s, A, B, x, f_a_wins, la_first, bb, f_a, f_b).
    f_a_wins and la_first (cases 1 and 2 only, else None) say which of f_a >= f_b and c < 0 (LA before LB) held; f_a and f_b are
    the two values compared there.  `dots`: dict(q, r, bb), the three dots as a caller took them (the learners take theirs
    in float32: tests/update64.py), in place of the float64 ones of the vectors."""
    b, Hinv_g, Hinv_b, approx_g = (np.asarray(v, dtype=np.float64) for v in (b, Hinv_g, Hinv_b, approx_g))
    s, c, tkl = float(s), float(c), float(target_kl)
    q = float(Hinv_g @ approx_g) if dots is None else float(dots["q"])
    bb = float(b @ b) if dots is None else float(dots["bb"])
    f_a_wins = la_first = f_a = f_b = None
    with np.errstate(all="ignore"):
        if bb <= 1e-8 and c < 0:
            Hinv_b = np.zeros_like(Hinv_g)
            r = s = A = B = 0.0
            case = 4
        else:
            r = float(Hinv_b @ approx_g) if dots is None else float(dots["r"])
            A = q - r * r / s
            B = 2.0 * tkl - c * c / s
            case = 3 if (c < 0 and B < 0) else 2 if (c < 0 and B >= 0) else 1 if (c >= 0 and B >= 0) else 0
        if case in (3, 4):
            lam, nu = math.sqrt(q / (2.0 * tkl)), 0.0
        elif case in (1, 2):
            rc = r / c
            la_first = c < 0
            LA, LB = ((0.0, rc), (rc, math.inf)) if la_first else ((rc, math.inf), (0.0, rc))
            proj = lambda x, L: max(L[0], min(L[1], x))      # noqa: E731  (Python's: the first argument unless the second wins)
            lam_a = proj(float(np.sqrt(A / B)), LA)
            lam_b = proj(math.sqrt(q / (2.0 * tkl)), LB)
            f_a = -0.5 * (A / (lam_a + EPS) + B * lam_a) - r * c / (s + EPS)
            f_b = -0.5 * (q / (lam_b + EPS) + 2.0 * tkl * lam_b)
            f_a_wins = bool(f_a >= f_b)
            lam = lam_a if f_a_wins else lam_b
            nu = max(0, lam * c - r) / (s + EPS)
        else:
            lam, nu = 0.0, math.sqrt(2.0 * tkl / (s + EPS))
        x = (1.0 / (lam + EPS)) * (Hinv_g + nu * Hinv_b) if case > 0 else nu * Hinv_b
    return dict(optim_case=case, lam=lam, nu=nu, q=q, r=r, s=s, A=A, B=B, x=x, f_a_wins=f_a_wins, la_first=la_first, bb=bb,
                f_a=f_a, f_b=f_b)


SITUATIONS = ("case0", "case1_fa", "case1_fb", "case2_fa", "case2_fb", "case3", "case4")
DIRECTION_P = 2500          # more than two passes of the kernel's 1024 lanes, and no multiple of them


@functools.lru_cache(maxsize=None)
def direction_inputs(name):
    """dict(b, Hinv_g, Hinv_b, approx_g (float32), s, c, target_kl) that lands in the situation `name`: Hinv_g, Hinv_b random,
    approx_g = M Hinv_g and s = Hinv_b' M Hinv_b for a diagonal positive M (so q > 0, s > 0 and A >= 0 by Cauchy-Schwarz), with
    c and target_kl moved until the ladder takes the branch asked for (tests/test_pgrad64.py asserts that it does)."""
    rng = np.random.default_rng(SITUATIONS.index(name))
    P = DIRECTION_P
    M = rng.uniform(0.5, 2.0, P)
    f = np.float32
    Hg, Hb = rng.standard_normal(P).astype(f), rng.standard_normal(P).astype(f)
    b = (M * Hb).astype(f)
    if name.endswith("_fa"):                     # g nearly against b, so that the trust region's own step breaks the constraint
        Hg = (Hg * 0.05 - Hb).astype(f)
    if name.endswith("_fb"):                     # g leaning along b: the trust region's own step keeps the constraint
        Hg = (Hg + 0.05 * Hb).astype(f)
    ag = (M * Hg.astype(np.float64)).astype(f)
    s = float(f(Hb.astype(np.float64) @ (M * Hb.astype(np.float64))))
    tkl = 0.01
    reach = math.sqrt(2.0 * tkl * s)             # |c| below it: the boundary cuts the trust region (B >= 0)
    c = {"case0": 2.0 * reach, "case1_fa": 0.5 * reach, "case1_fb": 0.02 * reach, "case2_fa": -0.5 * reach,
         "case2_fb": -0.02 * reach, "case3": -2.0 * reach, "case4": -1.0}[name]
    if name == "case4":
        b = np.zeros(P, f)
        Hb = np.full(P, np.nan, f)               # what a solve of nothing might leave: it must not reach the output
        s = float("nan")
    out = dict(b=b, Hinv_g=Hg, Hinv_b=Hb, approx_g=ag, s=s, c=float(c), target_kl=tkl)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# cases, computed once per process and never written to
# ---------------------------------------------------------------------------------------------------------------------
CANDIDATE_SEEDS = (0, 1, 2, 3)
# A kept seed's float32 yardsticks are within SPREAD x of the median over the four.  3, not the 2 of vfit's displacements: over
# these shapes the draws reach 2.0 x (D = 1) and 1.95 x (the trained regime) with nothing wrong with them, and a bound that
# sits on a draw flips with the CPU's float32 sums.  What the rule is for is a seed an order of magnitude off (vfit's seed 0:
# 30 x).  A seed 3 x off moves the pooled yardstick of four by sqrt((3 + 9) / 4) = 1.7 x at the most, inside the allowance of 4.
SPREAD = 3.0
# the one seed in four a shape may keep out (tests/test_pgrad64.py:test_the_seeds_are_well_conditioned): none does
KEPT_OUT = {}
ROWS = (1, 63, 64, 65, 257, 4099)
# the first-layer instantiations of gx_pgrad.hip at their edges: vfit's list, which has none of 33 .. 49, and those
EDGE_WIDTHS = v64.EDGE_WIDTHS + (33, 44, 45, 48, 49)
# regime, D, A, B: every shape tests/test_gpu_pgrad.py compares at
SHAPES = tuple([("default", D, 2, B) for D in (43, 64) for B in ROWS] + [("default", 43, 8, 130), ("default", 43, 10, 130)] +
               [("default", D, 2, v64.EDGE_ROWS) for D in EDGE_WIDTHS] + [("trained", 43, 2, 257), ("saturated", 43, 2, 257)] +
               [("default", 43, 2, 16385)])


@functools.lru_cache(maxsize=None)
def gradient_case(regime, D, A, B, seed):
    """dict(pi, theta, batch, g, b, means (float64 oracle), yard_g, yard_b: grad_errors of the learners' float32 autograd)"""
    pi, theta, batch = l64.make_batch(regime, D, A, B, seed)
    import torch
    g, means = grad64(theta, batch)
    b, _ = grad64(theta, batch, cost=True)
    yard_g = grad_errors(learners_gradient(pi, theta, batch, False, torch.float32), g, D, A)
    yard_b = grad_errors(learners_gradient(pi, theta, batch, True, torch.float32), b, D, A)
    for a in (g, b):
        a.setflags(write=False)
    return dict(pi=pi, theta=theta, batch=batch, g=g, b=b, means=means, yard_g=yard_g, yard_b=yard_b)


def kept_seeds(regime, D, A, B):
    """The seeds the GPU comparison pools over at this shape: CANDIDATE_SEEDS without the shape's entry of KEPT_OUT, the same
    on every machine.  Standardised adv makes g a sum with heavy cancellation, and a seed on which float32 autograd itself
    is an outlier measures the lottery, not the method: tests/test_pgrad64.py holds every kept seed's yardsticks to within
    SPREAD x of the median over the four, and shows the seed kept out to be outside."""
    return tuple(s for s in CANDIDATE_SEEDS if s != KEPT_OUT.get((regime, D, A, B)))


def seed_spread(regime, D, A, B):
    """{seed: the larger of its two float32 yardsticks' distances (g, b) from the median over CANDIDATE_SEEDS, as a factor >= 1}"""
    yards = {s: (gradient_case(regime, D, A, B, s)["yard_g"][0], gradient_case(regime, D, A, B, s)["yard_b"][0]) for s in CANDIDATE_SEEDS}
    med = [float(np.median([y[i] for y in yards.values()])) for i in (0, 1)]
    return {s: math.exp(max(abs(math.log(yards[s][i] / med[i])) for i in (0, 1))) for s in CANDIDATE_SEEDS}


def yardstick(regime, D, A, B):
    """-> (pooled yard_g, pooled yard_b) over the kept seeds, each (whole, {block: error})"""
    cases = [gradient_case(regime, D, A, B, s) for s in kept_seeds(regime, D, A, B)]
    return pool([c["yard_g"] for c in cases]), pool([c["yard_b"] for c in cases])
