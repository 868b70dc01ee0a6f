"""tests/update64.py, the float64 oracle of a whole TRPO or CPO epoch, on the CPU: against the learners' formulation in torch
float64 (autograd for g, b and Hx, the learners' cg, the ladder, learners_means, autograd with torch.optim.Adam), for every
epoch of every sequence; that every decision of every epoch is decidable (the ladder's and the search's thresholds at least
DECIDABLE = 100 x the float32 learners' error away, and the float32 learners decide as the oracle does); that the yardstick
is well conditioned where the Fisher matrix is damped; and eight planted mistakes at the seams between the stages, each a
keyword of the oracle.  CPU only; no reference checkout is read.

The bound of the float64 comparison.  The pieces are held to the same formulation one by one at 1e-12 (test_pgrad64.py: g and
b; test_fisher64.py: H x; test_vfit64.py: the fit's displacement and loss trace).  The critics are one piece: 1e-12.  x_direction
is the end of a chain (g -> ten CG steps -> the ladder) that amplifies a relative perturbation; how much is measured by the
float32 learners, whose per-operation error of 2^-24 ends as the yardstick of x, so a piece's 1e-12 ends as at most
1e-12 x (the sequence's largest yardstick of x) / 2^-24.  Each stage of the formulation goes on from the oracle's rounded g, b
and x_direction (its own g and b are compared first), so that no entry's rounding to float32 can differ between the two: a
stage is compared on the input the oracle's stage had, theta_new bit for bit and the displacement as coeff^accepted x before
the rounding.  Measured (relative L2, the worst epoch of each sequence; bound):
    trpo_default   x 6.5e-13 (2.8e-09)   v 1.0e-15
    trpo_trained   x 2.5e-14 (4.1e-11)   v 1.6e-15
    cpo_default    x 2.4e-13 (1.4e-09)   v 8.7e-16   vc 7.9e-16
    cpo_trained    x 3.2e-14 (8.8e-11)   v 1.6e-15   vc 1.6e-15
    cpo_wide       x 1.9e-15 (2.1e-11)   v 5.4e-15   vc 1.0e-15

Margins (the smallest of each sequence, ladder | search): cpo_default 1.4e+04 | 1.1e+04, cpo_trained 975 | 3.0e+03, cpo_wide
8.0e+04 | 3.8e+04, cpo_trained_257 1.5e+03 | 8.4e+03, trpo_default 5.6e+03, trpo_trained 3.4e+03.  The yardsticks and their
spreads are recorded in tests/update64.py beside the sequences.

Planted mistakes (x the pooled yardstick, the smallest over the epochs each can show in): the Fisher product at the previous
epoch's theta 8.3e+03 (x_direction); the search from the previous epoch's theta 1.2e+04 (the displacement); Adam's moments zeroed
1.6e+05; its step count restarted 8.7e+04; the second solve on g 9.2e+02; ret in cost_ret's place 1.4e+05.  need_loss taken as 1
in cases 0 and 1 moves nothing else in these sequences (the loss falls along every accepted step), so it shows as need_loss
itself, which tests/test_gpu_update.py compares; cost_margin = -c without the max rejects every candidate where c > 0 in
cpo_wide (both epochs) and binds in neither cpo_default nor cpo_trained, where the step lowers the surrogate cost by more than c."""
import copy
import math

import numpy as np
import pytest
import torch

import fisher64 as f64
import pgrad64 as p64
import update64 as u64
import vfit64 as v64

TOL = 1e-12                                     # the bound each piece is held to against the same formulation
DECISIONS = ("accepted", "optim_case", "f_a_wins", "need_loss")


def decisions(r):
    return {k: r.get(k) for k in DECISIONS}


@pytest.mark.parametrize("name", u64.COMPARED)
def test_the_oracle_is_the_learners_formulation_in_float64(name):
    seq = u64.sequence(name)
    spec, cpo = seq["spec"], seq["spec"]["learner"] == "cpo"
    amp = max(e["yard"]["x"] for e in seq["epochs"]) / 2.0 ** -24
    bound = TOL * max(amp, 1.0)
    critics = {k: copy.deepcopy(seq[k]).double() for k in ("v", "vc") if seq[k] is not None}
    opts = {k: torch.optim.Adam(c.parameters(), lr=v64.LR) for k, c in critics.items()}
    for i, e in enumerate(seq["epochs"]):
        ref = e["ref"]
        form = u64.learners_update32(e["pi"], e["theta"], e["batch"], e["c"], u64.COST_REDUCTION, damping=spec["damping"],
                                     dtype=torch.float64, given={k: ref[k] for k in ("g", "b", "x") if k in ref}, **u64.HYPER)
        assert decisions(form) == decisions(ref), (i, decisions(form), decisions(ref))
        assert form["theta_new"].view(np.int32).tolist() == ref["theta_new"].view(np.int32).tolist()
        for k in ("g", "b"):
            if k in ref:
                assert f64.rel_l2(form[k], ref[k]) <= 2.0 ** -23       # float64 autograd against the oracle's, rounded to float32
        t = u64.COEFF ** ref["accepted"]
        ex, ed = f64.rel_l2(form["x"], ref["x64"]), f64.rel_l2(t * form["x"], t * ref["x64"])
        line = f"{name} epoch {i}: x {ex:.2e}  coeff^j x {ed:.2e} (bound {bound:.2e})"
        assert ex <= bound and ed <= bound
        assert f64.rel_l2(form["trace"], ref["trace"]) <= 1e-9          # the means the search decided on
        if cpo:
            for k in ("lam", "nu"):
                assert abs(form[k] - ref[k]) <= bound * abs(ref[k]) + 1e-300, k
        for k, ret in (("v", "ret"), ("vc", "cost_ret")):
            if k in critics:
                th, losses = u64.learners_fit(critics[k], opts[k], e["theta_" + k], e["state_" + k], e["batch"]["obs"], e["batch"][ret])
                dv = u64.displacement_errors(e["theta_" + k], th, e["crit"][k]["theta"])
                dl = u64.loss_errors(losses, e["crit"][k]["losses"])
                line += f"  {k} {dv:.2e} loss {dl:.2e} (bound {TOL:.0e})"
                assert dv <= TOL and dl <= TOL, k
        print(line)


@pytest.mark.parametrize("name", tuple(u64.SEQUENCES))
def test_every_decision_is_decidable(name):
    """a condition on the inputs: the seeds of update64.SEQUENCES are chosen so that it holds"""
    seq = u64.sequence(name)
    cpo = seq["spec"]["learner"] == "cpo"
    assert len(seq["epochs"]) == 3 and [e["B"] for e in seq["epochs"]] == list(seq["spec"]["rows"])
    for i, e in enumerate(seq["epochs"]):
        ref, learn = e["ref"], e["learn"]
        search = u64.search_margins(e)
        worst = min(search, key=lambda m: m[2])
        line = f"{name} epoch {i} B={e['B']} c={e['c']}: accepted {ref['accepted']}; search's smallest margin {worst[2]:.3g} (j = {worst[0]}, {worst[1]})"
        assert worst[2] >= u64.DECIDABLE and ref["accepted"] >= 0
        if cpo:
            ladder = u64.ladder_margins(ref, learn)
            line += f"; optim_case {ref['optim_case']} f_a_wins {ref['f_a_wins']}; ladder " + ", ".join(f"{k} {v:.3g}" for k, v in ladder)
            assert min(v for _, v in ladder) >= u64.DECIDABLE
            assert ref["optim_case"] == u64.EXPECTED_CASES[name][i]
            assert ref["cost_margin"] == max(-e["c"], -u64.COST_REDUCTION) and ref["need_loss"] == int(ref["optim_case"] > 1)
        print(line)
        assert decisions(learn) == decisions(ref), (i, decisions(learn), decisions(ref))
        assert not np.array_equal(ref["theta_new"], e["theta"])
    assert all(np.array_equal(a["ref"]["theta_new"], b["theta"]) for a, b in zip(seq["epochs"], seq["epochs"][1:]))


def test_the_sequences_reach_what_they_are_for():
    cases = {e["ref"]["optim_case"] for n in u64.COMPARED for e in u64.sequence(n)["epochs"] if e["c"] is not None}
    accepted = {e["ref"]["accepted"] for n in u64.COMPARED for e in u64.sequence(n)["epochs"]}
    wins = {e["ref"]["f_a_wins"] for n in u64.COMPARED for e in u64.sequence(n)["epochs"] if e["c"] is not None}
    print(f"optim_case {sorted(cases)}  accepted {sorted(accepted)}  f_a_wins {wins}")
    assert cases == {0, 1, 2, 3} and {0, 1, 2} <= accepted and {True, False, None} <= wins
    seq = u64.sequence("cpo_trained")["epochs"]
    assert [e["B"] for e in seq] == [257, 130, 321] and u64.sequence("cpo_wide")["spec"]["D"] == 96
    for e in seq:                                                            # read-only, and fresh obs every epoch
        assert not any(v.flags.writeable for v in e["batch"].values() if v is not None)
    assert not np.array_equal(seq[0]["batch"]["obs"][:130], seq[1]["batch"]["obs"])


@pytest.mark.parametrize("name", u64.COMPARED)
def test_the_yardstick_is_well_conditioned(name):
    """damped: every epoch's float32 yardstick for x_direction and for the displacement within pgrad64.SPREAD of the median over
    the sequence's epochs.  Undamped: a ten-step float32 CG on an undamped Fisher matrix is a lottery the reference shares;
    the spread is printed and recorded beside update64.SEQUENCES, and asserted finite only."""
    seq, yard = u64.sequence(name), u64.yardstick(name)
    sx, sd = u64.spread(name, "x"), u64.spread(name, "disp")
    print(f"{name}: pooled " + "  ".join(f"{k} {v:.2e}" for k, v in yard.items()) + f"; x per epoch " +
          " ".join(f"{e['yard']['x']:.2e}" for e in seq["epochs"]) + f" (spread {sx:.2f}); displacement " +
          " ".join(f"{e['yard']['disp']:.2e}" for e in seq["epochs"]) + f" (spread {sd:.2f})")
    assert all(math.isfinite(v) and v > 0.0 for v in yard.values()) and math.isfinite(sx) and math.isfinite(sd)
    if seq["spec"]["damping"] > 0.0:
        assert sx <= p64.SPREAD and sd <= p64.SPREAD
    assert yard["x"] < 1e-2 and yard["v"] < 1e-4


# ---------------------------------------------------------------------------------------------------------------------
# planted mistakes: name -> (the epochs it can show in, whether it must show in every one of them)
# ---------------------------------------------------------------------------------------------------------------------
def _applies(mistake, i, e):
    cpo = e["c"] is not None
    return dict(fisher_at_previous_theta=i > 0, search_from_previous_theta=i > 0, moments_zeroed=i > 0, step_restarts=i > 0,
                need_loss_always=cpo and e["ref"].get("optim_case") in (0, 1), margin_without_max=cpo and e["c"] > -u64.COST_REDUCTION,
                second_solve_on_g=cpo and e["ref"].get("optim_case") in (0, 1, 2), ret_for_cost_ret=cpo)[mistake]


# where c > 0 the smaller margin binds only if the step lowers the surrogate cost by less than c: it does not in cpo_trained
EVERY = {m: m != "margin_without_max" for m in u64.MISTAKES}
# what a mistake of the policy half moves (the critics' mistakes move the critics they touch): the search from another theta
# is given the right x_direction, and the two criteria of the search can only flip `accepted` or need_loss itself
MOVES = dict(fisher_at_previous_theta=("x",), second_solve_on_g=("x",), search_from_previous_theta=("disp",),
             need_loss_always=("disp",), margin_without_max=("disp",))


@pytest.mark.parametrize("mistake", u64.MISTAKES)
def test_a_planted_mistake_is_caught(mistake):
    """each mistake against the oracle without it: a decision flips, or the quantity the mistake moves (x_direction, the
    displacement, a critic's displacement) is off by more than ALLOWED x the sequence's pooled yardstick, which is what
    tests/test_gpu_update.py allows the device"""
    shown = tried = 0
    for name in u64.COMPARED:
        seq, yard = u64.sequence(name), u64.yardstick(name)
        eps, spec = seq["epochs"], seq["spec"]
        for i, e in enumerate(eps):
            if not _applies(mistake, i, e):
                continue
            tried += 1
            prev, ref, sizes = (eps[i - 1] if i else None), e["ref"], {}
            if mistake in ("moments_zeroed", "step_restarts", "ret_for_cost_ret"):
                got = u64.critics64(e["theta_v"], e["state_v"], e["theta_vc"], e["state_vc"], e["batch"], **{mistake: True})
                for k in ("v", "vc"):
                    if got[k] is not None and not (mistake == "ret_for_cost_ret" and k == "v"):
                        sizes[k] = u64.displacement_errors(e["theta_" + k], got[k]["theta"], e["crit"][k]["theta"]) / yard[k]
                flips = []
            else:
                kw = {"fisher_at_previous_theta": dict(fisher_theta=prev and prev["theta"]),
                      "search_from_previous_theta": dict(search_theta=prev and prev["theta"])}.get(mistake, {mistake: True})
                got = u64.oracle_epoch(spec, e["theta"], e["batch"], e["c"], **kw)
                flips = [k for k in DECISIONS if got.get(k) != ref.get(k)]
                sizes["x"] = f64.rel_l2(got["x"], ref["x"]) / yard["x"]
                sizes["disp"] = u64.displacement_errors(e["theta"], got["theta_new"], ref["theta_new"]) / yard["disp"]
            held = [sizes[k] for k in MOVES.get(mistake, sizes)]                 # the quantities the mistake moves
            caught = bool(flips) or min(held) > u64.ALLOWED
            print(f"{mistake} {name} epoch {i}: " + "  ".join(f"{k} {v:.3g} x the yardstick" for k, v in sizes.items()) +
                  (f"  flips {flips}" if flips else "") + ("" if caught else "  NOT SHOWN"))
            shown += caught
            if EVERY[mistake]:
                assert caught, (name, i)
    assert tried >= 2 and shown >= 2, (tried, shown)
