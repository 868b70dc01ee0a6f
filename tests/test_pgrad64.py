"""tests/pgrad64.py, the float64 oracle of the device's surrogate gradients and CPO direction, against what it restates: float64
autograd of the learners' two losses (grad64, at 1e-12 relative L2: measured 4.9e-15 at worst, 8.8e-15 for a block), five planted mistakes that the
same comparison must catch, and the dual problem that cpo.py:468-525 solves (cpo_direction64) on inputs that reach every
optim_case, both outcomes of the tie rule in cases 1 and 2 and both orders of LA and LB.  The checkout's own lines are run
against cpo_direction64 in tests/test_reference_pgrad.py, live; no line of them is kept here.  CPU only.

The seeds of the GPU comparison: standardised adv makes g a sum with heavy cancellation, so the float32 yardstick (torch's
float32 autograd against grad64) is itself a draw.  The GPU tests pool over the seeds 0 .. 3 less the one a shape keeps out
(pgrad64.KEPT_OUT, fixed lists: the same seeds everywhere).  The rule, test_the_seeds_are_well_conditioned: a kept seed's
yardsticks for g and for b are within 3 x of the median over the four; a seed kept out is outside; at most one in four goes.
Kept out: none.  The widest draws are seed 3 at D, A, B = 1, 2, 130 (7.1e-07 for g against a median of 3.5e-07, 2.0 x) and
seed 2 in the trained regime (2.5e-06 for b against 1.3e-06, 1.95 x); every other seed of every shape is within 1.75 x."""
import math

import numpy as np
import pytest
import torch

import linesearch64 as l64
import pgrad64 as p64

TOL = 1e-12
SHAPES = [("default", 43, 2, 257), ("default", 64, 8, 130), ("trained", 5, 4, 7), ("saturated", 128, 16, 65), ("wide_log_std", 17, 6, 33)]


def _batch(regime, D, A, B):
    """a batch whose logp_old is off the actor's own, so that ratio is not 1"""
    pi, theta, batch = l64.make_batch(regime, D, A, B, seed=1)
    shift = 0.3 * np.random.default_rng(5).standard_normal(B).astype(np.float32)
    return pi, theta, dict(batch, logp=batch["logp"] + shift)


@pytest.mark.parametrize("regime,D,A,B", SHAPES)
def test_grad64_is_the_gradient_of_the_learners_losses(regime, D, A, B):
    pi, theta, batch = _batch(regime, D, A, B)
    for cost in (False, True):
        want = p64.learners_gradient(pi, theta, batch, cost, torch.float64)
        assert want.shape == (p64.f64.param_count(D, A, 64),)
        got, means = p64.grad64(theta, batch, cost=cost)
        err, blocks = p64.grad_errors(got, want, D, A)
        planted = {m: p64.f64.rel_l2(p64.grad64(theta, batch, cost=cost, mistake=m)[0], want) for m in p64.MISTAKES}
        print(f"{regime} D={D} A={A} B={B} {'b' if cost else 'g'}: {err:.2e} (worst block {max(blocks.values()):.2e}); planted " +
              "  ".join(f"{k} {e:.2e}" for k, e in planted.items()))
        assert err <= TOL and max(blocks.values()) <= TOL
        for m, e in planted.items():
            assert e >= 100.0 * TOL, m
    ref = l64.learners_means(pi, theta, batch, torch.float64)
    assert abs(means["pi_l"] - ref[1]) <= TOL * abs(ref[1]) + 1e-15 and abs(means["surr_cost"] - ref[2]) <= TOL * abs(ref[2]) + 1e-15
    assert abs(means["approx_kl"] - ref[3]) <= TOL * abs(ref[3]) + 1e-15
    ent = torch.distributions.Normal(torch.zeros(A, dtype=torch.float64), torch.exp(torch.as_tensor(theta[:A]).double())).entropy().sum()
    assert abs(means["ent"] - float(ent)) <= TOL * abs(float(ent))


def test_log_std_comes_first():
    pi, theta, batch = _batch("default", 43, 2, 65)
    g, _ = p64.grad64(theta, batch)
    sl = p64.block_slices(43, 2)
    assert list(sl) == list(p64.BLOCKS) and sl["log_std"] == slice(0, 2) and sl["b3"].stop == g.size
    assert [tuple(p.shape) for p in pi.parameters()][0] == (2,)


# ---------------------------------------------------------------------------------------------------------------------
# CPO's direction: cpo_direction64 against the problem it solves (tests/test_reference_pgrad.py runs the checkout's own lines)
# ---------------------------------------------------------------------------------------------------------------------
def dual(lam, nu, q, r, s, c, target_kl):
    """The Lagrange dual of CPO's step: minimise g'x over x'Hx / 2 <= target_kl and b'x + c <= 0.  With multipliers lam and
    nu the minimiser is x = -(H^-1 g + nu H^-1 b) / lam (the learners step along -x_direction) and the dual's value is this,
    in q = g'H^-1 g, r = g'H^-1 b and s = b'H^-1 b"""
    return -(q + 2.0 * nu * r + nu * nu * s) / (2.0 * lam) + nu * c - lam * target_kl


def best_nu(lam, r, s, c):
    """the dual is concave in nu: its maximiser over nu >= 0"""
    return np.maximum(0.0, (lam * c - r) / s)


def test_cpo_direction64_solves_the_dual_in_every_situation():
    """the seven situations are reached, and in each the multipliers are the ones the problem asks for: in cases 1 to 3 the
    pair (lam, nu) maximises the dual over a fine grid of lam with nu at its best for each; in case 4 (no constraint) lam is
    the trust region's own; in case 0 (nothing feasible) the step along H^-1 b ends on the trust region's boundary"""
    reached = set()
    for name in p64.SITUATIONS:
        i = p64.direction_inputs(name)
        got = p64.cpo_direction64(**i)
        case, lam, nu, q, r, s, c, tkl = [got[k] for k in ("optim_case", "lam", "nu", "q", "r", "s")] + [i["c"], i["target_kl"]]
        print(f"{name}: optim_case {case} lam {lam:.6g} nu {nu:.6g} f_a_wins {got['f_a_wins']} "
              f"la_first {got['la_first']} q {q:.4g} r {r:.4g} s {s:.4g} A {got['A']:.4g} B {got['B']:.4g}")
        assert case == int(name[4]) and np.isfinite(got["x"]).all()
        Hg, Hb = (np.asarray(i[k], dtype=np.float64) for k in ("Hinv_g", "Hinv_b"))
        reached.add(("case", case))
        if case in (1, 2, 3):
            grid = np.geomspace(lam / 100.0, lam * 100.0, 40001)
            values = dual(grid, best_nu(grid, r, s, c), q, r, s, c, tkl)
            mine = dual(lam, nu, q, r, s, c, tkl)
            at = grid[np.argmax(values)]
            print(f"    dual at (lam, nu) {mine:.9g}; the grid's best {values.max():.9g} at lam {at:.6g}")
            assert mine >= values.max() - 1e-9 * abs(mine) and abs(at / lam - 1.0) <= 1e-3
            assert math.isclose(nu, float(best_nu(lam, r, s, c)), rel_tol=1e-9, abs_tol=0.0)
            assert np.linalg.norm(got["x"] - (Hg + nu * Hb) / lam) <= 1e-9 * np.linalg.norm(got["x"])
        if case in (1, 2):
            assert got["f_a_wins"] == name.endswith("_fa") and got["la_first"] == (case == 2)
            assert (nu > 0.0) == got["f_a_wins"]                     # the constraint binds exactly where its branch wins
            reached.add((case, got["f_a_wins"]))
            reached.add(("la_first", got["la_first"]))
        if case == 4:
            assert (got["r"], got["s"], got["A"], got["B"], nu) == (0.0, 0.0, 0.0, 0.0, 0.0)
            assert math.isclose(lam, math.sqrt(q / (2.0 * tkl)), rel_tol=1e-15)
            assert np.linalg.norm(got["x"] - Hg / lam) <= 1e-9 * np.linalg.norm(got["x"])
        if case == 0:
            assert lam == 0.0 and math.isclose(0.5 * nu * nu * s, tkl, rel_tol=1e-9)
            assert np.array_equal(got["x"], nu * Hb)
    # the seven situations: every case, both outcomes of f_a >= f_b in cases 1 and 2, both orders of LA and LB
    assert {("case", k) for k in range(5)} <= reached
    assert {(1, True), (1, False), (2, True), (2, False), ("la_first", True), ("la_first", False)} <= reached


# ---------------------------------------------------------------------------------------------------------------------
# the seeds of the GPU comparison
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,D,A,B", p64.SHAPES)
def test_the_seeds_are_well_conditioned(regime, D, A, B):
    """for every shape and seed tests/test_gpu_pgrad.py uses: the float32 yardsticks of g and of b are within 3 x of the median
    over the seeds 0 .. 3; the seed a shape keeps out is not; and no shape keeps out more than one in four"""
    kept, spread = p64.kept_seeds(regime, D, A, B), p64.seed_spread(regime, D, A, B)
    cases = {s: p64.gradient_case(regime, D, A, B, s) for s in p64.CANDIDATE_SEEDS}
    print(f"{regime} D={D} A={A} B={B}: kept {kept}; yardsticks g | b (x from the median)  " +
          "  ".join(f"seed {s} {c['yard_g'][0]:.2e} | {c['yard_b'][0]:.2e} ({spread[s]:.2f})" for s, c in cases.items()))
    assert len(p64.CANDIDATE_SEEDS) == 4 and len(kept) >= 3 and set(kept) <= set(p64.CANDIDATE_SEEDS)
    if B > 1:                                                    # one row: nothing to cancel, and an error of an ulp or none
        for s in p64.CANDIDATE_SEEDS:
            assert (spread[s] <= p64.SPREAD) == (s in kept), s
    (yg, _), (yb, _) = p64.yardstick(regime, D, A, B)
    assert 0.0 < yg < 1e-4 and 0.0 < yb < 1e-4


def test_every_shape_kept_out_of_is_a_shape_compared_at():
    assert set(p64.KEPT_OUT) <= set(p64.SHAPES) and all(s in p64.CANDIDATE_SEEDS for s in p64.KEPT_OUT.values())
