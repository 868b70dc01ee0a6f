"""tests/pifit64.py, the float64 oracle of the policy fit, against the learners' formulation: grad64 against float64 autograd of
the three actor losses (torch.min of the two branches, the unclipped surrogate, -(logp adv).mean()), fit64 against a float64
transcription of the learners' loop around torch.optim.Adam with its `break`; that the comparison catches each planted
mistake by 10 x the tolerance or more; and the conditions on the inputs that tests/test_gpu_pifit.py relies on: the shares of
the rows on either side of the clip range, the distance of every ratio from its edges, the margins of every target_kl, and the
seeds kept out by name.  CPU only."""
import numpy as np
import pytest
import torch

import pgrad64 as p64
import pifit64 as a64

TOL = 1e-12
SHAPES = [("default", 43, 2, 257), ("default", 64, 2, 130), ("default", 43, 8, 130), ("trained", 43, 2, 257), ("saturated", 43, 2, 65)]


# ---------------------------------------------------------------------------------------------------------------------
# the gradient
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loss,clip_ratio", a64.LOSSES)
@pytest.mark.parametrize("regime,D,A,B", SHAPES)
def test_grad64_is_float64_autograd_of_the_learners_loss(regime, D, A, B, loss, clip_ratio):
    c = a64.gradient_case(regime, D, A, B, 1, clip_ratio, loss)
    want, wl, wk, wc = a64.learners_gradient(c["pi"], c["theta"], c["batch"], clip_ratio, loss, torch.float64)
    err = p64.f64.rel_l2(c["g"], want)
    means = max(abs(c["info"]["loss"] - wl), abs(c["info"]["kl"] - wk))
    print(f"{regime} D={D} A={A} B={B} {loss} clip={clip_ratio}: g {err:.2e}, loss and kl {means:.2e}")
    assert err <= TOL and means <= TOL
    assert abs(c["info"]["cf"] - wc) <= 1e-7                      # the learners' cf is a float32 mean
    ls = c["theta"][:A].astype(np.float64)
    assert abs(c["info"]["ent"] - float((ls + 0.5 + p64.HALF_LOG_2PI).sum())) <= 1e-14


@pytest.mark.parametrize("regime,D,A,B", SHAPES)
def test_clipping_by_ratio_alone_is_caught(regime, D, A, B):
    """the planted mistake cuts every row outside the range, whatever the sign of adv: half of the cut rows are wrong"""
    c = a64.gradient_case(regime, D, A, B, 1)
    want = a64.learners_gradient(c["pi"], c["theta"], c["batch"], a64.CLIP, "ratio", torch.float64)[0]
    wrong = a64.grad64(c["theta"], c["batch"], mistake="clip_by_ratio_alone")[0]
    assert p64.f64.rel_l2(wrong, want) >= 10.0 * TOL
    assert p64.f64.rel_l2(wrong, want) >= 0.1                     # and not by a hair: a quarter of the rows change sides


def test_the_row_weight_is_what_autograd_gives_torch_min():
    """per row, on hand-made ratios: d/d ratio of min(ratio adv, clamp(ratio) adv) is adv times pifit64's `active`, a tie
    inside the range included (the two halves add to the whole)"""
    ratio = torch.tensor([0.5, 0.5, 0.79, 0.81, 1.0, 1.19, 1.21, 1.21, 2.0, 2.0, 1.0], dtype=torch.float64, requires_grad=True)
    adv = torch.tensor([1.0, -1.0, -2.0, -2.0, 3.0, 1.0, 1.0, -1.0, 2.0, -2.0, 0.0], dtype=torch.float64)
    torch.min(ratio * adv, torch.clamp(ratio, 0.8, 1.2) * adv).sum().backward()
    r, a = ratio.detach().numpy(), adv.numpy()
    cut = ((a > 0) & (r > 1.2)) | ((a < 0) & (r < 0.8))
    assert ratio.grad.numpy().tolist() == (a * np.where(cut, 0.0, 1.0)).tolist()
    assert cut.tolist() == [False, True, True, False, False, False, True, False, True, False, False]


# ---------------------------------------------------------------------------------------------------------------------
# the loop
# ---------------------------------------------------------------------------------------------------------------------
def _case():
    return a64.fit_case(43, 257, 0)


def _both(c, calls, targets, **kw):
    """consecutive calls of `calls` iterations with `targets`: [(fit64's result, the learners' float64 loop's)]"""
    out, state, carry, theta = [], None, None, c["theta"]
    for n, tkl in zip(calls, targets):
        mine = a64.fit64(theta, c["batch"], n, tkl, state=state, **kw)
        theirs, carry = a64.learners_loop(c["pi"], c["theta"], c["batch"], n, tkl, carry=carry, **{k: v for k, v in kw.items() if k != "mistake"})
        state, theta = mine["state"], mine["theta"]
        out.append((mine, theirs))
    return out


@pytest.mark.parametrize("loss,clip_ratio", a64.LOSSES)
@pytest.mark.parametrize("calls", [(1,), (2,), (3,), (10,), (5, 5)])
def test_fit64_is_the_learners_loop(calls, loss, clip_ratio):
    c = _case()
    worst = 0.0
    for mine, theirs in _both(c, calls, [None] * len(calls), clip_ratio=clip_ratio, loss=loss):
        worst = max(worst, a64.loop_difference(mine, theirs))
        assert mine["stop_iter"] == theirs["stop_iter"] and mine["steps"] == theirs["steps"] == len(mine["thetas"]) - 1
    print(f"calls {calls} {loss} clip={clip_ratio}: largest difference {worst:.2e}")
    assert worst <= TOL


@pytest.mark.parametrize("where", [0, a64.MID, None])
def test_fit64_stops_where_the_learners_stop(where):
    c = _case()
    (mine, theirs), = _both(c, (10,), (c["targets"][where],))
    assert mine["stop_iter"] == theirs["stop_iter"] == (9 if where is None else where)
    assert mine["steps"] == theirs["steps"] == (10 if where is None else where)
    assert a64.loop_difference(mine, theirs) <= TOL
    evaluated = mine["steps"] + (where is not None)
    for k in a64.TRACES:
        assert np.isnan(mine[k][evaluated:]).all() and not np.isnan(mine[k][:evaluated]).any()
    assert mine["state"]["step"] == mine["steps"]
    # a stop, then the optimizer goes on: the second call equals the learners' second epoch
    again = _both(c, (10, 4), (c["targets"][where], None))
    assert a64.loop_difference(*again[1]) <= TOL and again[1][0]["state"]["step"] == mine["steps"] + 4


def test_a_nan_kl_does_not_stop():
    c = _case()
    batch = dict(c["batch"], logp=np.full_like(c["batch"]["logp"], np.nan))
    mine = a64.fit64(c["theta"], batch, 2, 0.01)
    assert mine["steps"] == 2 and mine["stop_iter"] == 1 and np.isnan(mine["kl"]).all()
    assert not (float("nan") > 0.01)


@pytest.mark.parametrize("mistake", a64.LOOP_MISTAKES)
def test_each_planted_mistake_in_the_loop_is_caught(mistake):
    """the scenario in which the mistake shows, compared as test_fit64_stops_where_the_learners_stop compares"""
    c = _case()
    mid = c["targets"][a64.MID]
    if mistake == "threshold_1p5":
        calls, targets = (10,), (mid,)                            # 1.5 x the target is passed later, or never
        assert c["ref"]["kl"][a64.MID] < 1.5 * mid
    elif mistake in ("stop_after_step", "trace_past_stop"):
        calls, targets = (10,), (mid,)
    else:
        calls, targets = (10, 3), (mid, None)                     # what the stop left in the count shows in the next call
    worst = 0.0
    state, carry, theta = None, None, c["theta"]
    wrong_state, wrong_theta = None, c["theta"]                   # the mistaken optimizer carries its own state on
    for n, tkl in zip(calls, targets):
        wrong = a64.fit64(wrong_theta, c["batch"], n, tkl, state=wrong_state, mistake=mistake)
        right = a64.fit64(theta, c["batch"], n, tkl, state=state)
        theirs, carry = a64.learners_loop(c["pi"], c["theta"], c["batch"], n, tkl, carry=carry)
        assert a64.loop_difference(right, theirs) <= TOL
        worst = max(worst, a64.loop_difference(wrong, theirs))
        state, theta = right["state"], right["theta"]
        wrong_state, wrong_theta = wrong["state"], wrong["theta"]
    print(f"{mistake}: difference {worst:.2e}")
    assert worst >= 10.0 * TOL and worst >= 1e-6


# ---------------------------------------------------------------------------------------------------------------------
# the conditions on the inputs
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime,D,A,B", [s for s in a64.SHAPES if s[3] >= 63])
def test_every_group_of_rows_is_populated(regime, D, A, B):
    for seed in a64.grad_seeds(regime, D, A, B):
        c = a64.gradient_case(regime, D, A, B, seed)
        sh = a64.shares(c["ratio"], c["batch"]["adv"])
        assert all(sh[k] >= a64.GROUP_SHARE for k in ("up_pos", "up_neg", "down_pos", "down_neg")) and sh["inside"] >= a64.INSIDE_SHARE, (seed, sh)


@pytest.mark.parametrize("regime,D,A,B", a64.SHAPES)
def test_no_gradient_case_has_a_ratio_at_an_edge(regime, D, A, B):
    assert len(a64.grad_seeds(regime, D, A, B)) >= 3
    for seed in a64.GRAD_CANDIDATES:
        c = a64.gradient_case(regime, D, A, B, seed)
        assert (c["edge"] >= a64.EDGE) == (seed in a64.grad_seeds(regime, D, A, B)), (seed, c["edge"])
        if seed in a64.grad_seeds(regime, D, A, B):
            assert abs(c["learners"]["cf"] - c["info"]["cf"]) <= 1e-7     # float32 counts the same rows


@pytest.mark.parametrize("D,B", a64.FIT_SHAPES)
def test_the_fit_seeds_are_decidable(D, B):
    """every kept seed passes the three conditions at every compared iteration; every seed kept out fails the one it is kept
    out for"""
    seeds = a64.fit_seeds(D, B)
    assert len(seeds) >= 3 and set(a64.FIT_KEPT_OUT[D, B]) <= set(a64.FIT_CANDIDATES)
    spread = a64.fit_spread(D, B)
    for seed in a64.FIT_CANDIDATES:
        c = a64.fit_case(D, B, seed)
        margins = {w: a64.stop_margin(c, w) for w in (0, a64.MID, None)}
        facts = dict(edge=c["edge"] >= a64.EDGE, spread=spread[seed] <= a64.SPREAD,
                     margin=all(min(m) >= a64.DECIDABLE for m in margins.values()))
        print(f"D={D} B={B} seed {seed}: edge {c['edge']:.1e} spread {spread[seed]:.1f} margins "
              f"{ {w: round(min(m)) for w, m in margins.items()} } kl error {c['kl_err']:.1e}")
        if seed in seeds:
            assert all(facts.values()), (seed, facts)
            sh = a64.shares(a64.forward64(c["theta"], c["batch"])[1], c["batch"]["adv"])
            assert all(sh[k] >= a64.GROUP_SHARE for k in ("up_pos", "up_neg", "down_pos", "down_neg")) and sh["inside"] >= a64.INSIDE_SHARE
            # the oracle's own run under each target stops where the test says
            for w in (0, a64.MID, None):
                assert a64.fit64(c["theta"], c["batch"], 10, c["targets"][w])["stop_iter"] == (9 if w is None else w)
            # and cf is what float32 counts, at every compared iteration
            assert np.abs(c["f32"]["cf"] - c["ref"]["cf"][:10]).max() <= 1e-7
        else:
            assert not facts[a64.FIT_KEPT_OUT[D, B][seed]], (seed, facts)


def test_the_states_on_record_are_the_single_call():
    c = _case()
    assert [s["step"] for s in c["states"]] == list(range(11))
    whole = a64.fit64(c["theta"], c["batch"], 10)
    assert np.array_equal(whole["theta"], c["ref"]["thetas"][10]) and np.array_equal(whole["state"]["m"], c["states"][10]["m"])
