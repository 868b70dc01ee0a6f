"""tests/cfit64.py against the reference learners' OWN code, run on the CPU live from a checkout of the reference
(tests/reflearn.py), in the manner of tests/test_reference_vfit.py: the reference's C_Critic (usl, lpg, safelayer) under its
compute_loss_ccritic and its MLPMaxCostCritic (scpo) under its compute_loss_vc, in float64, against grad64 and its loss under
the 0 / 1 weights of the same selection.  CPU only; the whole file skips where the checkout is absent, and nothing of it is
recorded here.

The loss functions are closures inside the learners' main functions (they read `ac` from there), so they cannot be imported:
each definition is taken from the parsed file and compiled over an `ac` of this test's.  The random choice of the
down-sampling (safelayer's `downsample_rand.choice`, scpo's `np.random.choice`) is a stand-in that checks what it is asked for
(the population, the size int(len * frac), replace=False) and hands out supplied indices.

The largest difference observed is written down (MEASURED) and asserted at 10 x that; a planted mistake in the oracle (the
division by B in place of W where rows are selected out, the dropped f' elsewhere) must miss the same tolerance by 10 x or
more.
"""
import ast
import copy
import os
import types

import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

MEASURED = {"usl": 5e-16, "lpg": 5e-16, "safelayer": 5e-16, "scpo": 5e-16}
D, A, B = 43, 2, 257


def _path(learner):
    return os.path.join(reflearn.LIBX, learner, learner + ".py")


def _closure(learner, name, ns):
    """the function `name` defined inside the learner's main function, compiled over the namespace `ns`"""
    import warnings
    with open(_path(learner)) as f, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tree = ast.parse(f.read(), filename=_path(learner))
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1
    exec(compile(ast.Module(body=found, type_ignores=[]), _path(learner), "exec"), ns)
    return ns[name]


class _Choice:
    """the random choice, supplied: records the call and returns the first `size` entries of a fixed permutation"""

    def __init__(self, seed):
        self.seed, self.calls, self.given = seed, [], None

    def choice(self, n, size=None, replace=True):
        self.calls.append((n, size, replace))
        self.given = np.random.default_rng(self.seed).permutation(n)[:size]
        return self.given


def _targets(gen, sparse):
    import torch
    y = torch.rand(B, generator=gen, dtype=torch.float64) * 3.0 + 0.1
    if sparse:
        y = torch.where(torch.rand(B, generator=gen, dtype=torch.float64) < 0.8, torch.zeros((), dtype=torch.float64), y)
    return y


@pytest.mark.parametrize("sparse", [False, True])
@pytest.mark.parametrize("learner", list(MEASURED))
def test_grad64_is_the_gradient_of_the_references_loss(learner, sparse):
    import torch
    import torch.nn.functional as F
    import cfit64 as c64
    gen = torch.Generator().manual_seed(9)
    obs = torch.randn(B, D, generator=gen, dtype=torch.float64)
    act_safe = torch.randn(B, A, generator=gen, dtype=torch.float64).clamp(-1, 1)
    y = _targets(gen, sparse)
    pick = _Choice(3)
    if learner == "scpo":
        ac = copy.deepcopy(reflearn.actor_critic("scpo", D - 1, A, 64, seed=5)).double()     # its networks see obs and M
        critic, head, name = ac.vc, "softplus", "compute_loss_vc"
        assert type(critic).__name__ == "MLPMaxCostCritic" and critic.v_net[0].in_features == D
        data, x, act, off = dict(obs=obs, cost_ret=y), obs, None, None
        ns = dict(ac=ac, torch=torch, F=F, np=types.SimpleNamespace(random=pick))
    else:
        critic = copy.deepcopy(reflearn.c_critic(learner, D, A, 64, seed=5)).double()
        ac = types.SimpleNamespace(ccritic=critic)
        name = "compute_loss_ccritic"
        ns = dict(ac=ac, torch=torch, F=F, np=np, downsample_rand=pick)
        if learner == "safelayer":
            prev = torch.rand(B, generator=gen, dtype=torch.float64)
            head, data, x, act, off = "dot", dict(obs=obs, act_safe=act_safe, cost=y, prev_cost=prev), obs, act_safe, prev
        else:
            head, x, act, off = "softplus", torch.cat((obs, act_safe), dim=1), None, None
            data = dict(obs=obs, act_safe=act_safe, targetc=y)
    loss = _closure(learner, name, ns)(data)
    got = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, list(critic.parameters()))]).numpy()
    # the weights of what the reference selected
    down = learner in ("safelayer", "scpo") and sparse
    if down:
        n_pos, n_zero = int((y > 0).sum()), int((y == 0).sum())
        assert n_pos < n_zero and pick.calls == [(n_zero, int(n_zero * (n_pos / n_zero)), False)]
        assert pick.calls[0][1] == c64.downsample_count(n_pos, n_zero)
        w = c64.keep_to_weights(y.numpy(), pick.given)
        assert 0 < w.sum() < B
    else:
        assert pick.calls == []                                 # usl and lpg never down-sample; the others keep a dense batch whole
        w = None
    from guardx_amd import cfit
    assert cfit.CostCriticFit(critic.float(), lr=1e-3).head == head
    critic.double()
    theta = c64.flat(critic).numpy()
    np_ = lambda t: None if t is None else t.numpy()             # noqa: E731
    g, l64, W = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off))
    mistake = "over_b" if down else ("no_fprime" if head == "softplus" else "no_offset")
    wrong, _, _ = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off), mistake=mistake)
    measured = max(c64.rel_l2(g, got), c64.rel_err(l64, loss.item()))
    planted = c64.rel_l2(wrong, got)
    tol = 10.0 * MEASURED[learner]
    print(f"reference vs grad64 ({learner}, {'down-sampled' if down else 'whole batch'}): largest difference {measured:.3e} "
          f"(recorded {MEASURED[learner]:.1e}, asserted at {tol:.1e}); planted {mistake} {planted:.3e}")
    assert measured <= tol and planted >= 10.0 * tol


def test_the_cited_lines_hold_the_loops():
    """the lines guardx_amd/cfit.py cites name what it says they do"""
    text = lambda learner, a, b: "".join(open(_path(learner)).readlines()[a - 1:b])    # noqa: E731
    for learner, a, b, words in (("usl", 378, 383, ("compute_loss_ccritic", "act_safe", "targetc")),
                                 ("usl", 449, 454, ("train_ccritic_iters", "ccritic_optimizer", "compute_loss_ccritic")),
                                 ("lpg", 386, 391, ("compute_loss_ccritic", "act_safe", "targetc")),
                                 ("lpg", 457, 462, ("train_ccritic_iters", "ccritic_optimizer", "compute_loss_ccritic")),
                                 ("safelayer", 384, 418, ("compute_loss_ccritic", "prev_cost", "downsample_rand", "mse_loss")),
                                 ("safelayer", 483, 488, ("train_ccritic_iters", "ccritic_optimizer")),
                                 ("scpo", 419, 450, ("compute_loss_vc", "cost_ret", "choice"))):
        for word in words:
            assert word in text(learner, a, b), (learner, a, b, word)
