"""tests/linesearch64.py on the CPU: the float64 oracle against the learners' formulation in torch float64 (a deep-copied
actor with assigned flat parameters, Normal(mu, exp(log_std)).log_prob(act).sum(-1), diagonal_gaussian_kl), four planted
mistakes it must catch, the plain numpy float32 statement of include/guardx_linesearch.h within 2 x the yardstick (the
device is allowed 4 x: tests/test_gpu_linesearch.py), and the decidability of every search case the GPU tests use.

Measured: the oracle against torch float64, worst difference over the shapes 1.4e-14 (asserted: 1e-12); the planted
mistakes, 8.7e-4 (EPS dropped) to 1.1e3; the float32 statement, worst ratio to the yardstick 1.31 (pi_l, saturated; kl
below 0.3 everywhere); the search cases' smallest margin, 6.0e4 x the yardstick's error (asserted: 100 x)."""
import numpy as np
import pytest
import torch

import fisher64 as f64
import linesearch64 as l64

SHAPES = [("default", 43, 2, 1), ("default", 43, 2, 65), ("default", 64, 8, 257), ("trained", 43, 2, 257),
          ("saturated", 43, 2, 257), ("wide_log_std", 17, 16, 130)]
TOL = 1e-12


def rel(got, want, scales):
    """the largest of the four errors of linesearch64.errors: the measure the device is held to"""
    return l64.errors(got, want, scales)


@pytest.mark.parametrize("regime,D,A,B", SHAPES)
def test_the_oracle_is_the_learners_formulation(regime, D, A, B):
    """1e-12 in the errors the device is measured by (relative L2 over the steps; relative to mean |ratio adv|).  Value by
    value it cannot hold for either side: at t = 0.8^20 the KL is a 1e-6 remainder of O(1) terms, so two float64 evaluations
    that round differently differ by 1e-10 of it (3.9e-11 measured, saturated)."""
    c = l64.evaluate_case(regime, D, A, B, 0)
    got = l64.learners_evaluate(c["pi"], c["theta"], c["d"], c["batch"], c["steps"], torch.float64)
    worst = rel(got, c["want"], c["scales"]).max()
    print(f"{regime} D={D} A={A} B={B}: worst relative difference {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("mistake", [dict(variance=False), dict(eps=0.0), dict(swap=True), dict(log_std_last=True)])
def test_a_planted_mistake_is_caught(mistake):
    c = l64.evaluate_case("wide_log_std", 17, 16, 130, 0)
    steps = [1.0, 0.8 ** 4]
    want, scales = l64.evaluate64(c["theta"], c["d"], c["batch"], steps)
    wrong, _ = l64.evaluate64(c["theta"], c["d"], c["batch"], steps, **mistake)
    got = l64.learners_evaluate(c["pi"], c["theta"], c["d"], c["batch"], steps, torch.float64)
    assert rel(got, want, scales).max() <= TOL
    worst = rel(got, wrong, scales).max()
    print(f"{mistake}: relative difference {worst:.2e}")
    assert worst > 1000 * TOL


def test_the_candidate_is_numpys_float32_minus_float64_times_float64():
    c = l64.evaluate_case("default", 43, 2, 65, 0)
    theta, d = c["theta"], c["d"]
    for t in (1.0, 0.8 ** 4, 0.8 ** 20):
        flat = theta - t * d.astype(np.float64)               # get_net_param_np_vec(ac.pi) - step * x_direction
        assert flat.dtype == np.float64
        pi = f64.make_actor(43, 2)
        l64.assign_flat(pi, flat)                              # the assignment rounds to the parameters' float32
        assert f64.flat(pi).numpy().view(np.int32).tolist() == l64.candidate(theta, d, t).view(np.int32).tolist()
    assert l64.candidate(theta, np.full_like(d, np.nan), 0.0).view(np.int32).tolist() == theta.view(np.int32).tolist()


@pytest.mark.parametrize("regime,D,A,B", SHAPES)
def test_the_float32_statement_is_within_twice_the_yardstick(regime, D, A, B):
    cases = [l64.evaluate_case(regime, D, A, B, s) for s in l64.SEEDS]
    yard = l64.pooled([c["yard"] for c in cases])
    err = l64.pooled([l64.errors(l64.evaluate32(c["theta"], c["d"], c["batch"], c["steps"]), c["want"], c["scales"]) for c in cases])
    print(f"{regime} D={D} A={A} B={B}: " + "  ".join(f"{e:.2e} / {y:.2e} = {e / y:.2f}" for e, y in zip(err, yard)))
    assert (yard > 0).all() and (err <= 2.0 * yard).all()


@pytest.mark.parametrize("name", l64.SEARCH_CASES)
def test_every_search_case_is_decidable(name):
    c = l64.search_case(name)
    expect = dict(first=0, kl_binds=4, loss_binds=4, loss_not_needed=0, cost_binds=3, none=-1)[name]
    assert c["ref"]["accepted"] == expect
    m = l64.margins(c)
    tested = {j for j, _, _ in m}
    assert tested == set(range(expect + 1 if expect >= 0 else c["kw"]["iters"]))
    worst = min(m, key=lambda x: x[2])
    print(f"{name}: accepted {expect}; smallest margin {worst[2]:.3g} x the yardstick's error ({worst[1]} of candidate {worst[0]})")
    assert worst[2] >= l64.DECIDABLE
    # what binds where: the condition named is the one that rejects the candidate before the accepted one
    trace, kw = c["ref"]["trace"], c["kw"]
    if name == "kl_binds":
        assert trace[expect, 0] > kw["target_kl"] and trace[expect, 1] < trace[0, 1]
    if name == "loss_binds":
        assert trace[expect, 0] < kw["target_kl"] and trace[expect, 1] > trace[0, 1]
    if name == "cost_binds":
        assert trace[expect, 0] < kw["target_kl"] and trace[expect, 1] < trace[0, 1] and trace[expect, 2] - trace[0, 2] > kw["cost_margin"]
    if name == "none":
        assert (trace[1:, 1] > trace[0, 1]).all() and len(trace) == kw["iters"] + 1


def test_search64_and_a_nan():
    c = l64.search_case("first")
    d = np.array(c["d"])
    d[7] = np.nan
    ref = l64.search64(c["theta"], d, c["batch"], **dict(c["kw"], iters=5))
    assert ref["accepted"] == -1 and ref["theta_new"].tolist() == c["theta"].tolist() and np.isfinite(ref["old"]).all()
