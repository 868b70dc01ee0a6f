"""tests/pifit64.py against the reference learners' OWN code, run on the CPU live from a checkout of the reference
(tests/reflearn.py), in the manner of tests/test_reference_vfit.py: the reference's MLPActorCritic and its compute_loss_pi of
ppo_one_episode, espo_one_episode and a2c, in float64, against grad64, its loss, kl and cf.  CPU only; the whole file skips where
the checkout is absent, and nothing of it is recorded here.

compute_loss_pi is a closure inside the learner's main function (it reads `ac` and `clip_ratio` from there), so it cannot be
imported: its definition is taken from the parsed file and compiled over an `ac` of this test's.  The loop lives inside
update() and cannot be run: the lines guardx_amd/pifit.py cites are read off the checkout and their names compared.

The largest difference observed is written down (MEASURED) and asserted at 10 x that; a planted mistake in the oracle (clipping
by ratio alone) must miss the same tolerance by 10 x or more.
"""
import ast
import copy
import os
import re

import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

# learner -> (one_episode, loss, clip_ratio, the largest difference measured)
LEARNERS = {"ppo": (True, "ratio", 0.2, 5.1e-16), "espo": (True, "ratio", None, 5.4e-16), "a2c": (False, "logp", None, 4.5e-16)}


def _path(learner):
    return os.path.join(reflearn._dir(learner, LEARNERS[learner][0]), learner + ".py")


def _lines(learner, first, last):
    return "".join(open(_path(learner)).readlines()[first - 1:last])


def _actor_critic(learner, D, A, seed):
    """the learner's MLPActorCritic.  a2c_core.py imports a package this project does not depend on; its actor is, node for
    node, ppo_core.py's (asserted here), so a2c's loss is compiled over ppo's actor-critic"""
    import ast as _ast
    one_episode = LEARNERS[learner][0]
    if learner == "a2c":
        mine = os.path.join(reflearn._dir("a2c"), "a2c_core.py")
        theirs = os.path.join(reflearn._dir("ppo", True), "ppo_core.py")
        names = ["mlp", "Actor", "MLPGaussianActor"]
        assert [_ast.dump(x) for x in reflearn._nodes(mine, names)] == [_ast.dump(x) for x in reflearn._nodes(theirs, names)]
        learner, one_episode = "ppo", True
    return reflearn.actor_critic(learner, D, A, 64, seed=seed, one_episode=one_episode)


def _closure(learner, name, **ns):
    """the function `name` defined inside the learner's main function, compiled over the names in `ns`"""
    import torch
    import warnings
    with open(_path(learner)) as f, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tree = ast.parse(f.read(), filename=_path(learner))
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1
    ns = dict(ns, torch=torch, np=np)
    exec(compile(ast.Module(body=found, type_ignores=[]), _path(learner), "exec"), ns)
    return ns[name]


@pytest.mark.parametrize("learner", list(LEARNERS))
def test_grad64_is_the_gradient_of_the_references_loss(learner):
    import torch
    import linesearch64 as l64
    import pifit64 as a64
    one_episode, loss, clip_ratio, measured_before = LEARNERS[learner]
    D, A, B = 43, 2, 257
    ac = copy.deepcopy(_actor_critic(learner, D, A, 5)).double()
    assert type(ac.pi).__name__ == "MLPGaussianActor"
    pi32 = copy.deepcopy(ac.pi).float()
    gen = torch.Generator().manual_seed(9)
    batch = a64.shifted(l64.batch_of(pi32, torch.randn(B, D, generator=gen), seed=9, adc=False), 9)
    sh = a64.shares(a64.forward64(torch.cat([p.detach().reshape(-1) for p in ac.pi.parameters()]).numpy(), batch)[1], batch["adv"])
    assert min(sh.values()) >= a64.GROUP_SHARE
    data = {k: torch.from_numpy(np.array(batch[k])).double() for k in ("obs", "act", "adv", "logp")}
    loss_pi, pi_info = _closure(learner, "compute_loss_pi", ac=ac, clip_ratio=clip_ratio)(data)
    got = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss_pi, list(ac.pi.parameters()))]).numpy()
    theta = torch.cat([p.detach().reshape(-1) for p in ac.pi.parameters()]).numpy()
    g, info, _ = a64.grad64(theta, batch, clip_ratio, loss)
    measured = max(a64.f64.rel_l2(g, got), abs(info["loss"] - loss_pi.item()), abs(info["kl"] - pi_info["kl"]),
                   abs(info["ent"] / A - pi_info["ent"]))           # the reference logs the mean over the A dimensions, ent / A
    tol = 10.0 * measured_before
    line = f"reference vs grad64 ({learner}): largest difference {measured:.3e} (recorded {measured_before:.1e}, asserted at {tol:.1e})"
    if clip_ratio is not None:
        assert abs(info["cf"] - pi_info["cf"]) <= 1e-7            # the reference's is a float32 mean
        planted = a64.f64.rel_l2(a64.grad64(theta, batch, clip_ratio, loss, mistake="clip_by_ratio_alone")[0], got)
        line += f"; planted mistake {planted:.3e}"
        assert planted >= 10.0 * tol
    print(line)
    assert measured <= tol
    # the first entries of the traces are these values, and one step of fit64 is one step of torch.optim.Adam on that gradient
    run = a64.fit64(theta, batch, 2, None, clip_ratio, loss)
    assert (run["loss"][0], run["kl"][0], run["cf"][0]) == (info["loss"], info["kl"], info["cf"])
    opt = torch.optim.Adam(ac.pi.parameters(), lr=a64.LR)
    opt.zero_grad()
    loss_pi, _ = _closure(learner, "compute_loss_pi", ac=ac, clip_ratio=clip_ratio)(data)
    loss_pi.backward()
    opt.step()
    after = torch.cat([p.detach().reshape(-1) for p in ac.pi.parameters()]).numpy()
    assert a64.f64.rel_l2(run["thetas"][1] - theta, after - theta) <= 1e-9
    loss2, info2 = _closure(learner, "compute_loss_pi", ac=ac, clip_ratio=clip_ratio)(data)
    assert abs(run["loss"][1] - loss2.item()) <= 1e-12 and abs(run["kl"][1] - info2["kl"]) <= 1e-12


def test_policy_fit_takes_the_references_actor():
    from guardx_amd import pifit
    for learner in LEARNERS:
        ac = _actor_critic(learner, 43, 2, 5)
        PF = pifit.PolicyFit(ac.pi, lr=3e-4)
        assert (PF.D, PF.A) == (43, 2) and PF.P == sum(p.numel() for p in ac.pi.parameters())


def test_the_cited_lines_are_the_loop():
    """ppo.py:307-316, espo.py:292-301 (the loop) and a2c.py:303-307 (its one step), cited by guardx_amd/pifit.py and
    include/guardx_pifit.h: the names there, in their order (the lines themselves are not repeated here; the line that logs the
    stop is left out)"""
    def names(text):
        kept = [ln for ln in text.splitlines() if "logger.log" not in ln]
        return re.findall(r"[A-Za-z_]\w*", re.sub(r"#.*", "", "\n".join(kept)))
    loop = lambda var, bound: ["for", "i", "in", "range", "train_pi_iters", "pi_optimizer", "zero_grad", "loss_pi", "pi_info",   # noqa: E731
                               "compute_loss_pi", "data", var, "mpi_avg", "pi_info", "kl", "if", var, bound, "break", "loss_pi",
                               "backward", "mpi_avg_grads", "ac", "pi", "pi_optimizer", "step"]
    assert names(_lines("ppo", 307, 316)) == loop("kl", "target_kl")
    assert names(_lines("espo", 292, 301)) == loop("dev", "delta")
    assert names(_lines("a2c", 303, 307)) == ["pi_optimizer", "zero_grad", "loss_pi", "pi_info", "compute_loss_pi", "data", "loss_pi",
                                              "backward", "mpi_avg_grads", "ac", "pi", "pi_optimizer", "step"]
    assert names(_lines("ppo", 318, 318)) == ["logger", "store", "StopIter", "i"]
    assert names(_lines("ppo", 292, 292)) == ["pi_optimizer", "Adam", "ac", "pi", "parameters", "lr", "pi_lr"]
    for path in ("guardx_amd/pifit.py", "include/guardx_pifit.h"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)).read()
        assert "ppo.py:307-316" in text and "espo.py:292-301" in text and "a2c.py:303-307" in text, path
