"""tests/pgrad64.py against the reference learners' OWN code, run on the CPU live from a checkout of the reference
(tests/reflearn.py), in the manner of tests/test_reference_linesearch.py: the reference's auto_grad over its
MLPGaussianActor.forward(obs, act), in float64, against grad64.  CPU only; the whole file skips where the checkout is absent,
and nothing of it is recorded here.

The largest difference observed is written down (MEASURED) and asserted at 10 x that; one planted mistake in the oracle must
miss the same tolerance by 10 x or more.  CPO's ladder lives inside update() and cannot be imported: its lines are read from the checkout
and run here, live, against the restatement pgrad64.cpo_direction64; none of them is kept in this repository."""
import os
import re

import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

MEASURED = {"trpo": 7.0e-16, "cpo": 7.0e-16}


@pytest.mark.parametrize("learner", ["trpo", "cpo"])
def test_grad64_is_the_references_auto_grad(learner):
    """MEASURED: 7.0e-16 (trpo and cpo, whose actors and auto_grad are the same code), the relative L2 of the flat gradient,
    the worse of g and b; the planted mistake (ratio taken as 1) 2.5e-1"""
    import copy
    import torch
    import fisher64 as f64
    import linesearch64 as l64
    import pgrad64 as p64
    D, A, B = 43, 2, 257
    auto_grad, = reflearn.main(learner, ["auto_grad"])
    pi = reflearn.actor_critic(learner, D, A, 64, seed=5).pi
    with torch.no_grad():
        pi.log_std.copy_(torch.linspace(-1.0, 0.2, A))
    obs = torch.randn(B, D, generator=torch.Generator().manual_seed(9))
    batch = l64.batch_of(pi, obs, seed=4)
    batch = dict(batch, logp=batch["logp"] + 0.3 * np.random.default_rng(6).standard_normal(B).astype(np.float32))   # ratio is not 1
    theta = f64.flat(pi).numpy()
    pi64 = copy.deepcopy(pi).double()
    t = lambda k: torch.from_numpy(np.array(batch[k])).double()      # noqa: E731
    worst, planted = 0.0, np.inf
    for cost in (False, True):
        _, logp = pi64(t("obs"), t("act"))
        ratio = torch.exp(logp - t("logp"))
        loss = (ratio * t("adc")).mean() if cost else -(ratio * t("adv")).mean()
        want = auto_grad(loss, pi64)
        assert isinstance(want, np.ndarray) and want.dtype == np.float64 and want.shape == theta.shape
        worst = max(worst, f64.rel_l2(p64.grad64(theta, batch, cost=cost)[0], want))
        planted = min(planted, f64.rel_l2(p64.grad64(theta, batch, cost=cost, mistake="ratio_is_one")[0], want))
    tol = 10.0 * MEASURED[learner]
    print(f"reference auto_grad vs grad64 ({learner}): largest difference {worst:.3e} (recorded {MEASURED[learner]:.1e}, asserted at "
          f"{tol:.1e}); planted mistake {planted:.3e}")
    assert worst <= tol and planted >= 10.0 * tol


def _lines(learner, first, last):
    path = os.path.join(reflearn.LIBX, learner, learner + ".py")
    return "".join(open(path).readlines()[first - 1:last])


def _names(s):
    return re.findall(r"[A-Za-z_]\w*|<=|>=|<|>", re.sub(r"#.*", "", s))


def reference_ladder(i):
    """cpo.py:468-525 read from the checkout and run as they stand, live, on the inputs `i` (pgrad64.direction_inputs), with
    Python scalars: cg gives back the supplied Hinv_b, and Hx a vector whose product with Hinv_b is the supplied s; the
    reference's prints are swallowed.  -> the namespace the lines leave"""
    import textwrap
    vec = {k: np.asarray(i[k], dtype=np.float64) for k in ("b", "Hinv_g", "Hinv_b", "approx_g")}
    ns = dict(np=np, EPS=1e-8, b=vec["b"], Hinv_g=vec["Hinv_g"], approx_g=vec["approx_g"], c=i["c"], target_kl=i["target_kl"],
              q=vec["Hinv_g"].T @ vec["approx_g"], cg=lambda Hx, rhs: vec["Hinv_b"], Hx=lambda v: v * (i["s"] / (v @ v)),
              colorize=lambda *a, **k: "", print=lambda *a, **k: None)
    exec(compile(textwrap.dedent(_lines("cpo", 468, 525)), "cpo.py:468-525", "exec"), ns)
    return ns


def test_cpo_direction64_is_the_references_ladder():
    """the checkout's own lines against pgrad64.cpo_direction64 in the seven situations of tests/test_pgrad64.py: the same
    optim_case; lam, nu and x_direction at 1e-12 (measured: 5.7e-14 at worst, in the two situations where A = q - r^2 / s
    loses three digits of q and the stand-in for Hx gives s back to an ulp; exact zeros elsewhere)"""
    import pgrad64 as p64
    worst = 0.0
    for name in p64.SITUATIONS:
        i = p64.direction_inputs(name)
        ns, got = reference_ladder(i), p64.cpo_direction64(**i)
        assert ns["optim_case"] == got["optim_case"] == int(name[4])
        errs = [abs(float(ns[k]) - got[k]) / abs(got[k]) if got[k] else abs(float(ns[k])) for k in ("lam", "nu")]
        x = np.asarray(ns["x_direction"], dtype=np.float64)
        errs.append(np.linalg.norm(x - got["x"]) / np.linalg.norm(got["x"]))
        print(f"{name}: optim_case {ns['optim_case']}; lam, nu, x_direction differ by {errs[0]:.1e}, {errs[1]:.1e}, {errs[2]:.1e}")
        assert np.isfinite(x).all() and max(errs) <= 1e-12
        worst = max(worst, max(errs))
    print(f"the largest difference: {worst:.1e}")


def test_the_lines_the_header_singles_out():
    """cpo.py:445-525: the names and comparisons of the lines include/guardx_pgrad.h restates, in their order (the lines
    themselves are not repeated here): the two gradients, the first solve, the skip, the order of LA and LB, the tie rule,
    the EPS placements and the direction"""
    assert _names(_lines("cpo", 445, 446)) == ["g", "auto_grad", "loss_pi", "ac", "pi", "b", "auto_grad", "surr_cost", "ac", "pi"]
    assert _names(_lines("cpo", 459, 462)) == ["Hinv_g", "cg", "Hx", "g", "approx_g", "Hx", "Hinv_g", "q", "Hinv_g", "T", "approx_g"]
    assert _names(_lines("cpo", 468, 470)) == ["if", "b", "T", "b", "<=", "e", "and", "c", "<", "Hinv_b", "r", "s", "A", "B", "optim_case"]
    assert _names(_lines("cpo", 508, 509)) == ["LA", "LB", "r", "c", "r", "c", "np", "inf", "LA", "LB", "LA", "LB", "if", "c", "<", "else", "LB", "LA"]
    assert _names(_lines("cpo", 515, 515)) == ["lam", "lam_a", "if", "f_a", "lam_a", ">=", "f_b", "lam_b", "else", "lam_b"]
    assert _names(_lines("cpo", 517, 517)) == ["nu", "max", "lam", "c", "r", "s", "EPS"]
    assert _names(_lines("cpo", 521, 521)) == ["nu", "np", "sqrt", "target_kl", "s", "EPS"]
    assert _names(_lines("cpo", 525, 525)) == ["x_direction", "lam", "EPS", "Hinv_g", "nu", "Hinv_b", "if", "optim_case", ">", "else", "nu", "Hinv_b"]


def test_pcpo_has_another_direction():
    """pcpo decides optim_case as cpo does but steps along trpo_step Hinv_g - cpo_step Linv_b: guardx_amd.pgrad lists it as
    not served"""
    text = re.sub(r"#.*", "", open(os.path.join(reflearn.LIBX, "pcpo", "pcpo.py")).read())
    line = [ln for ln in text.splitlines() if re.match(r"\s*x_direction\s*=", ln)]
    assert len(line) == 1 and _names(line[0]) == ["x_direction", "trpo_step", "Hinv_g", "cpo_step", "Linv_b"]
    from guardx_amd import pgrad
    assert "pcpo" in pgrad.__doc__
