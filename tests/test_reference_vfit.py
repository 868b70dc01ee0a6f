"""tests/vfit64.py against the reference learners' OWN code, run on the CPU live from a checkout of the reference
(tests/reflearn.py), in the manner of tests/test_reference_linesearch.py: the reference's MLPCritic and its compute_loss_v
(compute_loss_vc for CPO's cost critic), in float64, against grad64 and its loss.  CPU only; the whole file skips where the
checkout is absent, and nothing of it is recorded here.

compute_loss_v is a closure inside the learner's main function (it reads `ac` from there), so it cannot be imported: its
definition is taken from the parsed file and compiled over an `ac` of this test's.  The loop and the optimizer's construction
live inside update() and cannot be run: the lines guardx_amd/vfit.py cites are read off the checkout and their names compared.

The largest difference observed is written down (MEASURED) and asserted at 10 x that; a planted mistake in the oracle (the
dropped 1 - h^2) must miss the same tolerance by 10 x or more.
"""
import ast
import copy
import os
import re

import numpy as np
import pytest

import reflearn

pytestmark = pytest.mark.skipif(not reflearn.available(), reason="no reference checkout (GUARDX_REFERENCE)")

MEASURED = {("trpo", "v"): 4.1e-16, ("cpo", "v"): 4.1e-16, ("cpo", "vc"): 3.0e-16}


def _path(learner):
    return os.path.join(reflearn.LIBX, learner, learner + ".py")


def _lines(learner, first, last):
    return "".join(open(_path(learner)).readlines()[first - 1:last])


def _closure(learner, name, ac):
    """the function `name` defined inside the learner's main function, compiled over `ac`"""
    import torch
    import warnings
    with open(_path(learner)) as f, warnings.catch_warnings():
        warnings.simplefilter("ignore")
        tree = ast.parse(f.read(), filename=_path(learner))
    found = [n for n in ast.walk(tree) if isinstance(n, ast.FunctionDef) and n.name == name]
    assert len(found) == 1
    ns = dict(ac=ac, torch=torch, np=np)
    exec(compile(ast.Module(body=found, type_ignores=[]), _path(learner), "exec"), ns)
    return ns[name]


@pytest.mark.parametrize("learner,which", list(MEASURED))
def test_grad64_is_the_gradient_of_the_references_loss(learner, which):
    import torch
    import vfit64 as v64
    D, B = 43, 257
    ac = copy.deepcopy(reflearn.actor_critic(learner, D, 2, 64, seed=5)).double()
    critic = getattr(ac, which)
    assert type(critic).__name__ == "MLPCritic"
    gen = torch.Generator().manual_seed(9)
    obs = torch.randn(B, D, generator=gen, dtype=torch.float64)
    data = dict(obs=obs, ret=1.0 + 2.0 * torch.randn(B, generator=gen, dtype=torch.float64),
                cost_ret=torch.rand(B, generator=gen, dtype=torch.float64) * 3.0)
    loss_fn, key = (("compute_loss_v", "ret") if which == "v" else ("compute_loss_vc", "cost_ret"))
    loss = _closure(learner, loss_fn, ac)(data)
    got = torch.cat([g.reshape(-1) for g in torch.autograd.grad(loss, list(critic.parameters()))]).numpy()
    theta = v64.flat(critic).numpy()
    g, l64 = v64.grad64(theta, obs.numpy(), data[key].numpy())
    wrong, _ = v64.grad64(theta, obs.numpy(), data[key].numpy(), mistake="no_tanh_slope")
    measured = max(v64.rel_l2(g, got), v64.rel_err(l64, loss.item()))
    planted = v64.rel_l2(wrong, got)
    tol = 10.0 * MEASURED[learner, which]
    print(f"reference vs grad64 ({learner}.{which}): largest difference {measured:.3e} (recorded {MEASURED[learner, which]:.1e}, "
          f"asserted at {tol:.1e}); planted mistake {planted:.3e}")
    assert measured <= tol and planted >= 10.0 * tol


def test_the_references_critics_and_value_fit():
    """ValueFit takes the reference's MLPCritic as it is (its parameters() are W1 b1 W2 b2 W3 b3) and refuses SCPO's cost
    critic, whose output goes through a softplus"""
    import torch
    from guardx_amd import vfit
    ac = reflearn.actor_critic("cpo", 43, 2, 64, seed=5)
    for critic in (ac.v, ac.vc):
        VF = vfit.ValueFit(critic, lr=1e-3)
        assert VF.D == 43 and VF.P == sum(p.numel() for p in critic.parameters())
        assert [tuple(p.shape) for p in critic.parameters()] == [(64, 43), (64,), (64, 64), (64,), (1, 64), (1,)]
    scpo = reflearn.actor_critic("scpo", 43, 2, 64, seed=5)
    assert any(isinstance(m, torch.nn.Softplus) for m in scpo.vc.v_net)
    assert vfit.ValueFit(scpo.v, lr=1e-3).D == scpo.v.v_net[0].in_features
    with pytest.raises(NotImplementedError, match="a linear output only"):
        vfit.ValueFit(scpo.vc, lr=1e-3)


def test_the_cited_lines_are_the_loop():
    """trpo.py:434-439 and cpo.py:563-576 (the loop, cited by guardx_amd/vfit.py and include/guardx_vfit.h), trpo.py:375-380
    (the loss and the optimizer): the names there, in their order (the lines themselves are not repeated here)"""
    names = lambda s: re.findall(r"[A-Za-z_]\w*", re.sub(r"#.*", "", s))    # noqa: E731
    loop = lambda opt, fn, loss, net: ["for", "i", "in", "range", "train_%s_iters" % net, opt, "zero_grad", loss, fn, "data",   # noqa: E731
                                       loss, "backward", "mpi_avg_grads", "ac", net, opt, "step"]
    assert names(_lines("trpo", 434, 439)) == loop("vf_optimizer", "compute_loss_v", "loss_v", "v")
    assert names(_lines("cpo", 563, 568)) == loop("vf_optimizer", "compute_loss_v", "loss_v", "v")
    assert names(_lines("cpo", 571, 576)) == loop("vcf_optimizer", "compute_loss_vc", "loss_vc", "vc")
    assert names(_lines("trpo", 375, 377)) == ["def", "compute_loss_v", "data", "obs", "ret", "data", "obs", "data", "ret", "return",
                                               "ac", "v", "obs", "ret", "mean"]
    assert names(_lines("trpo", 380, 380)) == ["vf_optimizer", "Adam", "ac", "v", "parameters", "lr", "vf_lr"]
    for path in ("guardx_amd/vfit.py", "include/guardx_vfit.h"):
        text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), path)).read()
        assert "trpo.py:434-439" in text and "cpo.py:563-576" in text, path
