"""tests/linesearch64.py against the reference learners' OWN code, run on the CPU live from a checkout of the reference
(tests/reflearn.py), in the manner of tests/test_reference_learners.py: the reference's MLPGaussianActor._d_kl,
forward(obs, act) and diagonal_gaussian_kl in float64 against evaluate64.  CPU only; the whole file skips where the
checkout is absent, and nothing of it is recorded here.

The largest difference observed is written down (MEASURED) and asserted at 10 x that; one planted mistake in the oracle
must miss the same tolerance by 10 x or more.  The acceptance rule lives inside update() and cannot be imported: it is
transcribed, with its lines, in linesearch64.accepts, and checked here against the text of the checkout.
"""
import os
import re

import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

MEASURED = {"trpo": 3.4e-15, "cpo": 3.4e-15}
STEPS = (0.0, 1.0, 0.8 ** 4)


def reference_means(core, pi64, batch):
    """[kl, pi_l, surr_cost, approx_kl] from the reference's own methods (trpo.py:341-372, cpo's compute_cost_pi), float64"""
    import torch
    t = lambda k: torch.from_numpy(np.array(batch[k])).double()      # noqa: E731
    with torch.no_grad():
        kl = pi64._d_kl(t("obs"), t("mu"), t("logstd"), device=torch.device("cpu"))
        mu = pi64.mu_net(t("obs"))
        assert float(kl) == float(core.diagonal_gaussian_kl(t("mu"), t("logstd"), mu, pi64.log_std))
        _, logp = pi64(t("obs"), t("act"))
        ratio = torch.exp(logp - t("logp"))
        return np.array([kl.item(), -(ratio * t("adv")).mean().item(), (ratio * t("adc")).mean().item(),
                         (t("logp") - logp).mean().item()])


@pytest.mark.parametrize("learner", ["trpo", "cpo"])
def test_evaluate64_is_the_references_kl_and_log_prob(learner):
    """MEASURED: 3.3e-15 (trpo and cpo, whose actors are the same code) in linesearch64.errors' measure; the planted
    mistake (the KL's argument pairs swapped) 7.0e-2"""
    import copy
    import torch
    import fisher64 as f64
    import linesearch64 as l64
    D, A, B = 43, 2, 257
    core = reflearn.core(learner)
    pi = reflearn.actor_critic(learner, D, A, 64, seed=5).pi
    with torch.no_grad():
        pi.log_std.copy_(torch.linspace(-1.0, 0.2, A))
    obs = torch.randn(B, D, generator=torch.Generator().manual_seed(9))
    batch = l64.batch_of(pi, obs, seed=4)
    theta = f64.flat(pi).numpy()
    d = l64.scaled_direction(theta, np.random.default_rng(3).standard_normal(theta.size), batch, 0.05)
    want, scales = l64.evaluate64(theta, d, batch, STEPS)
    wrong, _ = l64.evaluate64(theta, d, batch, STEPS, swap=True)
    got = []
    for t in STEPS:
        tmp = copy.deepcopy(pi).double()
        l64.assign_flat(tmp, l64.candidate(theta, d, t))
        got.append(reference_means(core, tmp, batch))
    got = np.stack(got)
    measured, planted = l64.errors(got, want, scales).max(), l64.errors(got, wrong, scales).max()
    tol = 10.0 * MEASURED[learner]
    print(f"reference vs evaluate64 ({learner}): largest difference {measured:.3e} (recorded {MEASURED[learner]:.1e}, asserted at "
          f"{tol:.1e}); planted mistake {planted:.3e}")
    assert measured <= tol and planted >= 10.0 * tol


def _lines(learner, first, last):
    path = os.path.join(reflearn.LIBX, learner, learner + ".py")
    return "".join(open(path).readlines()[first - 1:last])


def test_the_acceptance_rule_is_the_one_transcribed():
    """linesearch64.accepts cites trpo.py:423 and cpo.py:545-548: the names compared there, in their order, are the ones it
    transcribes (the lines themselves are not repeated here)"""
    import linesearch64 as l64
    names = lambda s: re.findall(r"[A-Za-z_]\w*|<=", re.sub(r"#.*", "", s))    # noqa: E731
    assert names(_lines("trpo", 423, 423)) == ["if", "kl", "item", "<=", "target_kl", "and", "pi_l_new", "item", "<=", "pi_l_old"]
    assert names(_lines("cpo", 545, 548)) == ["if", "kl", "item", "<=", "target_kl", "and", "pi_l_new", "item", "<=", "pi_l_old",
                                              "if", "optim_case", "else", "True", "and", "surr_cost_new", "surr_cost_old", "<=",
                                              "max", "c", "cost_reduction"]
    assert "trpo.py:423" in l64.accepts.__doc__ and "cpo.py:545-548" in l64.accepts.__doc__
    # the candidate and the step sizes: trpo.py:409 and 419
    assert names(_lines("trpo", 409, 409)) == ["new_param", "get_net_param_np_vec", "ac", "pi", "step", "x_direction"]
    assert {"set_and_eval", "backtrack_coeff", "j"} <= set(names(_lines("trpo", 419, 419)))
    # and the rule itself, on rows of four: kl, pi_l, surr_cost, approx_kl
    old = [0.0, 1.0, 5.0, 0.0]
    assert l64.accepts([0.01, 1.0, 5.0, 0], old, 0.01, 0.0, 1, True)
    assert not l64.accepts([0.0100001, 1.0, 5.0, 0], old, 0.01, 0.0, 1, True)
    assert not l64.accepts([0.01, 1.0000001, 5.0, 0], old, 0.01, 0.0, 1, True)
    assert l64.accepts([0.01, 2.0, 5.0, 0], old, 0.01, 0.0, 0, True)
    assert not l64.accepts([0.01, 1.0, 5.1, 0], old, 0.01, 0.05, 1, True) and l64.accepts([0.01, 1.0, 5.1, 0], old, 0.01, 0.05, 1, False)
    for i in range(3):
        m = [0.0, 0.0, 0.0, 0.0]
        m[i] = float("nan")
        assert not l64.accepts(m, old, 0.01, 10.0, 1, True)


def test_the_lagrangian_term_is_linear_in_ratio():
    """trpolag.py:380-394: loss_pi = -(ratio adv).mean() + ac.lmd (ratio adc).mean(), so adv - lmd adc serves as adv"""
    text = re.sub(r"#.*", "", _lines("trpolag", 380, 394))
    stmts = {m.group(1): re.findall(r"[A-Za-z_][\w.]*", m.group(2)) for m in re.finditer(r"^\s*(\w+) = (.*)$", text, flags=re.M)}
    assert stmts["loss_pi_reward"] == ["ratio", "adv", "mean"] and stmts["surr_cost"] == ["ratio", "adc", "mean"]
    assert stmts["lag_term"] == ["ac.lmd", "surr_cost"] and stmts["loss_pi"] == ["loss_pi_reward", "lag_term"]
