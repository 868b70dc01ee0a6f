"""tests/vfit64.py against float64 autograd and torch.optim.Adam on the CPU: the oracle that tests/test_gpu_vfit.py holds
libguardx_vfit.so to is the learners' loss, its gradient and their optimizer.

As these tests print (float64, so the differences are rounding):
    grad64 against autograd         g 2.6e-16 .. 5.3e-16 (relative L2; a block at worst 1.1e-14), loss below 2.1e-16
                                                                                                 asserted at 1e-12
    fit64 against torch.optim.Adam  the displacement after 1, 2, 10 steps and 5 + 5 over two calls: 6.3e-16 .. 4.3e-14; the
                                    loss trace below 2.3e-16                                     asserted at 1e-12
    planted mistakes                no_tanh_slope 4.8e-02 .. 9.4e-01, no_two_over_b 2.5e+00 .. 1.3e+02 (of the gradient);
                                    no_bias_correction 3.2e+00, eps_inside_sqrt 4.6e-02, step_restarts 1.9e-01 (of the
                                    displacement over 5 + 5 steps): each misses 1e-12 by far more than 100 x
Adam's normalisation hides gradient-scale mistakes: with the 2 / B dropped from the gradient the fitted parameters after ten
steps differ by 2.4e-04 of the displacement only (m / sqrt(v) does not change with the gradient's scale; only eps weighs
differently), so that mistake is carried by the gradient tests, here and on the device, and fit64's own test would not be the
place to look for it.

The seeds of the device test: a critic whose first gradients hold an entry near zero makes every float32 method err 100 x
more on that entry's first steps (its m / sqrt(v) is +-1 whatever its size, so the sign of a gradient entry that rounding can
flip moves theta by 2 lr).  Seed 0 at D, B = 43, 257 reads 6.9e-05 where the others read 2.2e-06, and 2.2e-05 with its rows
permuted: such a seed measures the lottery, not the method, and test_the_seeds_are_well_conditioned keeps it out."""
import copy

import numpy as np
import pytest
import torch

import vfit64 as v64

TOL = 1e-12
SHAPES = [(43, 257), (64, 130), (5, 7), (128, 65)]


def _critic64(regime, D, B, seed=0):
    critic, obs, ret, theta, facts = v64.problem(regime, D, B, seed)
    return copy.deepcopy(critic).double(), obs.double(), ret.double(), theta.astype(np.float64), facts


@pytest.mark.parametrize("regime", list(v64.REGIMES))
@pytest.mark.parametrize("D,B", SHAPES)
def test_grad64_is_the_gradient_of_the_learners_loss(regime, D, B):
    critic, obs, ret, theta, _ = _critic64(regime, D, B)
    want, want_loss = v64.autograd_grad(critic, obs, ret)
    g, loss = v64.grad64(theta, obs.numpy(), ret.numpy())
    err, blocks, le = v64.grad_errors(g, loss, want, want_loss, D)
    planted = {m: v64.rel_l2(v64.grad64(theta, obs.numpy(), ret.numpy(), mistake=m)[0], want) for m in ("no_tanh_slope", "no_two_over_b")}
    print(f"{regime} D={D} B={B}: g {err:.2e} (worst block {max(blocks.values()):.2e}) loss {le:.2e}; planted " +
          "  ".join(f"{k} {e:.2e}" for k, e in planted.items()))
    assert err <= TOL and max(blocks.values()) <= TOL and le <= TOL
    for m, e in planted.items():
        assert e >= 100.0 * TOL, m


def test_the_regimes_are_what_their_names_promise():
    """default: hardly a unit past the polynomial's 0.625; trained: a good part above it, on both layers; saturated: part of
    |z| above 9, where tanh_f returns 1 and 1 - h^2 is 0"""
    share = {}
    for regime in v64.REGIMES:
        f = v64.problem(regime, 43, 257)[4]
        share[regime] = [(float(np.mean(np.abs(f[z]) > v64.SMALL)), float(np.mean(np.abs(f[z]) > v64.SAT))) for z in ("z1", "z2")]
        print(regime, " ".join("|%s| > 0.625: %.3f, > 9: %.3f" % (z, a, b) for z, (a, b) in zip(("z1", "z2"), share[regime])))
    assert all(a < 0.5 and b == 0.0 for a, b in share["default"])
    assert all(a > 0.5 for a, _ in share["trained"]) and share["trained"][0][1] > 0.0
    assert share["saturated"][0][1] > 0.1 and share["saturated"][1][1] > 0.01


def _adam_run(regime, D, B, calls, mistake=None):
    """(relative L2 of the displacement, worst relative error of the loss trace) of fit64 against torch.optim.Adam in
    float64, the steps taken as the consecutive calls `calls`"""
    critic, obs, ret, theta, _ = _critic64(regime, D, B)
    thetas, losses, opt = [], [], None
    for n in calls:
        ts, ls, opt = v64.learners_loop(critic, obs, ret, n, optimizer=opt)
        thetas, losses = ts, losses + list(ls)
    mine, state, mine_losses = theta, None, []
    for n in calls:
        ts, ls, state = v64.fit64(mine, obs.numpy(), ret.numpy(), n, state=state, mistake=mistake)
        mine, mine_losses = ts[-1], mine_losses + list(ls)
    assert state["step"] == (calls[-1] if mistake == "step_restarts" else sum(calls))
    return (v64.rel_l2(mine - theta, thetas[-1] - theta), max(v64.rel_err(a, b) for a, b in zip(mine_losses, losses)))


@pytest.mark.parametrize("regime", list(v64.REGIMES))
@pytest.mark.parametrize("calls", [(1,), (2,), (10,), (5, 5)])
def test_fit64_is_the_learners_loop(regime, calls):
    for D, B in SHAPES[:2]:
        err, le = _adam_run(regime, D, B, calls)
        print(f"{regime} D={D} B={B} steps {calls}: displacement {err:.2e}  loss trace {le:.2e}")
        assert err <= TOL and le <= TOL


@pytest.mark.parametrize("mistake", ["no_bias_correction", "eps_inside_sqrt", "step_restarts"])
def test_a_planted_mistake_in_adam_misses_by_far(mistake):
    err, _ = _adam_run("default", 43, 257, (5, 5), mistake=mistake)
    print(f"{mistake}: displacement {err:.2e}")
    assert err >= 100.0 * TOL


def test_adams_normalisation_hides_the_gradients_scale():
    """the module docstring's remark, measured: fit64 with the 2 / B dropped lands within 1e-3 of the right displacement"""
    err, _ = _adam_run("default", 43, 257, (10,), mistake="no_two_over_b")
    print(f"no_two_over_b through ten steps of Adam: displacement {err:.2e}")
    assert 100.0 * TOL <= err <= 1e-3


def test_the_stored_form_rounds_once():
    rng = np.random.default_rng(0)
    theta, m, g = (rng.standard_normal(50).astype(np.float32) for _ in range(3))
    v = (rng.standard_normal(50) ** 2).astype(np.float32)
    full = v64.adam64(theta, m, v, g, 3)
    stored = v64.adam64(theta, m, v, g, 3, store=np.float32)
    for a, b in zip(full, stored):
        assert b.dtype == np.float32 and (a.astype(np.float32) == b).all()


@pytest.mark.parametrize("D,B", v64.FIT_SHAPES)
def test_the_seeds_are_well_conditioned(D, B):
    """for every shape and seed tests/test_gpu_vfit.py uses: the learners' float32 loop, in row order and with its rows
    permuted, errs on the displacement within 2 x of the median over the seeds, at every k"""
    seeds = v64.FIT_SEEDS[D, B]
    assert len(seeds) == 4 and len(set(seeds)) == 4
    plain = {s: v64.float32_loop_errors(D, B, s) for s in seeds}
    perm = {s: v64.float32_loop_errors(D, B, s, np.random.default_rng(s).permutation(B)) for s in seeds}
    for k in v64.FIT_KS:
        med = float(np.median([plain[s]["theta", k] for s in seeds]))
        print(f"D={D} B={B} k={k}: median {med:.2e}  " +
              "  ".join(f"seed {s} {plain[s]['theta', k]:.2e} / permuted {perm[s]['theta', k]:.2e}" for s in seeds))
        for s in seeds:
            for e in (plain[s]["theta", k], perm[s]["theta", k]):
                assert med / 2.0 <= e <= 2.0 * med, (s, k)
    yard = v64.fit_yardstick(D, B)
    assert all(yard["theta", k] == v64.pooled([plain[s]["theta", k] for s in seeds]) for k in v64.FIT_KS)


def test_seed_zero_is_the_kind_of_seed_the_condition_keeps_out():
    e = v64.float32_loop_errors(43, 257, 0)
    med = np.median([v64.float32_loop_errors(43, 257, s)["theta", 1] for s in v64.FIT_SEEDS[43, 257]])
    print(f"seed 0 at D, B = 43, 257: {e['theta', 1]:.2e} against a median of {med:.2e}")
    assert 0 not in v64.FIT_SEEDS[43, 257] and e["theta", 1] > 10.0 * med
