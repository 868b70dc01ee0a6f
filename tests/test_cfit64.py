"""tests/cfit64.py (the float64 statement of include/guardx_cfit.h) against float64 autograd of the learners' own expressions,
the down-sampled ones with supplied indices among them; the planted mistakes; guardx_amd.cfit.downsample_weights on the CPU;
and the float32 yardsticks tests/test_gpu_cfit.py holds the kernel to.  No GPU."""
import copy

import numpy as np
import pytest
import torch

import cfit64 as c64
from guardx_amd import cfit

TOL = 1e-12          # tests/test_pgrad64.py's figure for a closed form against float64 autograd
SHAPES = (("softplus", 45, 1, 257), ("softplus", 1, 1, 5), ("dot", 43, 2, 130), ("dot", 17, 16, 65), ("identity", 64, 1, 63))


def _double(c, head, D, A, seed, regime):
    mod = c64.make_module(head, D, A, seed=seed, scale=c64.REGIMES[regime]["scale"], dtype=torch.float64)
    d = lambda t: None if t is None else t.double()              # noqa: E731
    return mod, d(c["x"]), d(c["y"]), d(c["act"]), d(c["offset"])


def _keep(y, seed):
    """indices among the rows with y == 0, as the reference's choice would supply them"""
    n_zero, n_pos = int((y == 0).sum()), int((y > 0).sum())
    k = c64.downsample_count(n_pos, n_zero)
    return None if k is None else np.random.default_rng(seed).choice(n_zero, size=k, replace=False)


@pytest.mark.parametrize("regime", list(c64.REGIMES))
@pytest.mark.parametrize("head,D,A,B", SHAPES)
def test_grad64_is_float64_autograd_of_the_learners_expressions(head, D, A, B, regime):
    c = c64.problem(head, regime, D, A, B, seed=1)
    mod, x, y, act, off = _double(c, head, D, A, 1, regime)
    theta = c64.flat(mod).numpy()
    np_ = lambda t: None if t is None else t.numpy()             # noqa: E731
    # the plain form
    want_g, want_l = c64.autograd_grad(c64.learners_loss(mod, head, x, y, None, act, off), mod)
    g, loss, W = c64.grad64(head, theta, x.numpy(), y.numpy(), None, np_(act), np_(off))
    assert W == B and c64.rel_l2(g, want_g) < TOL and c64.rel_err(loss, want_l) < TOL
    # fractional weights: the weighted expression
    w = c64.make_weights("fractional", B, 1)
    want_g, want_l = c64.autograd_grad(c64.weighted_loss(mod, head, x, y, torch.from_numpy(w).double(), act, off), mod)
    g, loss, W = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off))
    assert abs(W - w.astype(np.float64).sum()) < 1e-9 and c64.rel_l2(g, want_g) < TOL and c64.rel_err(loss, want_l) < TOL
    # the down-sampled form (boolean index, cat, mse_loss) with supplied indices is the weighted form under 0 / 1 weights
    keep = _keep(y.numpy(), 7)
    if regime == "sparse" and B > 5:
        assert keep is not None and 0 < len(keep) < int((y == 0).sum())
    if keep is not None:
        want_g, want_l = c64.autograd_grad(c64.learners_loss(mod, head, x, y, torch.from_numpy(keep), act, off), mod)
        w = c64.keep_to_weights(y.numpy(), keep)
        g, loss, W = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off))
        assert W == int((y > 0).sum()) + len(keep) and c64.rel_l2(g, want_g) < TOL and c64.rel_err(loss, want_l) < TOL
        # and the dead rows may hold anything
        xn, yn = x.numpy().copy(), y.numpy().copy()
        xn[w == 0], yn[w == 0] = np.nan, np.inf
        g2, loss2, _ = c64.grad64(head, theta, xn, yn, w, np_(act), np_(off))
        assert (g2 == g).all() and loss2 == loss


def test_the_regimes_are_what_their_names_say():
    for seed in c64.GRAD_SEEDS:
        c = c64.problem("softplus", "z20", c64.SOFT_D, 1, 257, seed)
        _, z, _, _ = c64.forward64("softplus", c["theta"], c["x"].numpy())
        assert z.max() > 20.5 and z.min() < -20.5 and ((z > -20) & (z < 20)).mean() > 0.3
        c = c64.problem("softplus", "sparse", c64.SOFT_D, 1, 257, seed)
        share = float((c["y"] == 0).float().mean())
        assert 0.85 < share < 0.95 and (c["y"] >= 0).all()
        c = c64.problem("softplus", "default", c64.SOFT_D, 1, 257, seed)
        assert (c["y"] > 0).all()


def test_softplus64_is_torchs():
    z = torch.cat([torch.linspace(-110, 95, 4001, dtype=torch.float64), torch.tensor([20.0, -20.0, 0.0, 19.999999, 20.000001], dtype=torch.float64)])
    z.requires_grad_(True)
    f = torch.nn.Softplus()(z)
    f.sum().backward()
    assert np.abs(c64.softplus64(z.detach().numpy()) - f.detach().numpy()).max() < 1e-13
    assert np.abs(c64.softplus_grad64(z.detach().numpy()) - z.grad.numpy()).max() < 1e-13


@pytest.mark.parametrize("mistake", c64.MISTAKES)
def test_planted_mistakes_are_caught(mistake):
    head = "softplus" if mistake in ("no_fprime",) else "dot"
    D, A, B = (45, 1, 130) if head == "softplus" else (43, 2, 130)
    c = c64.problem(head, "sparse", D, A, B, seed=2)
    mod, x, y, act, off = _double(c, head, D, A, 2, "sparse")
    w = c64.make_weights("fractional", B, 2)
    w[::3] = 0.0
    np_ = lambda t: None if t is None else t.numpy()             # noqa: E731
    live = torch.from_numpy(w != 0)
    pick = lambda t: None if t is None else t[live]              # noqa: E731
    want_g, want_l = c64.autograd_grad(c64.weighted_loss(mod, head, x[live], y[live], torch.from_numpy(w).double()[live], pick(act), pick(off)), mod)
    theta = c64.flat(mod).numpy()
    wrong_act = np.random.default_rng(5).standard_normal((B, A)) if head == "dot" else None
    right = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off))
    wrong = c64.grad64(head, theta, x.numpy(), y.numpy(), w, np_(act), np_(off), mistake=mistake, wrong_act=wrong_act)
    assert c64.rel_l2(right[0], want_g) < TOL and c64.rel_err(right[1], want_l) < TOL
    assert c64.rel_l2(wrong[0], want_g) > 1e-3, mistake


def test_fit64_is_the_learners_loop_in_float64():
    for head, D, A, B in c64.FIT_SHAPES:
        c = c64.fit_case(head, D, A, B, 0)
        mod, x, y, act, off = _double(c, head, D, A, 0, "default")
        opt = torch.optim.Adam(mod.parameters(), lr=c64.LR)
        for i in range(c64.FIT_ITERS):
            live = torch.from_numpy(c["w"][i] != 0)
            pick = lambda t: None if t is None else t[live]      # noqa: E731
            opt.zero_grad()
            loss = c64.weighted_loss(mod, head, x[live], y[live], None, pick(act), pick(off))
            loss.backward()
            opt.step()
            assert c64.rel_err(c["losses"][i], loss.item()) < 1e-9 and c["Ws"][i] == int(live.sum())
        moved = c64.flat(mod).numpy() - c["theta"]
        assert c64.rel_l2(c["thetas"][-1] - c["theta"], moved) < 1e-7      # float32 theta_0 against float64 steps
        assert (c["w"][0] != c["w"][1]).any()


def test_an_empty_selection_is_nan():
    c = c64.problem("softplus", "default", 45, 1, 65, 0)
    g, loss, W = c64.grad64("softplus", c["theta"], c["x"].numpy(), c["y"].numpy(), np.zeros(65, np.float32))
    assert W == 0.0 and np.isnan(loss) and np.isnan(g).all()
    assert torch.isnan(((torch.zeros(0) - torch.zeros(0)) ** 2).mean())         # the reference's mean of nothing


# ---------------------------------------------------------------------------------------------------------------------
# downsample_weights
# ---------------------------------------------------------------------------------------------------------------------
def _targets(n_pos, n_zero, extra=()):
    y = np.concatenate([np.linspace(0.5, 2.0, n_pos), np.zeros(n_zero), np.asarray(extra, dtype=np.float64)]).astype(np.float32)
    return torch.from_numpy(y[np.random.default_rng(n_pos * 41 + n_zero).permutation(y.size)].copy())


def test_the_count_is_the_references_for_every_pair_up_to_forty():
    gen = torch.Generator().manual_seed(0)
    for n_pos in range(41):
        for n_zero in range(41):
            if n_pos + n_zero == 0:
                continue
            y = _targets(n_pos, n_zero)
            w = cfit.downsample_weights(y, 2, generator=gen)
            assert w.dtype == torch.float32 and tuple(w.shape) == (2, n_pos + n_zero) and set(w.unique().tolist()) <= {0.0, 1.0}
            assert (w[:, y > 0] == 1).all(), (n_pos, n_zero)
            kept = w[:, y == 0].sum(1).tolist()
            if n_zero == 0 or n_pos / n_zero >= 1:
                assert (w == 1).all(), (n_pos, n_zero)
            else:
                want = int(n_zero * (n_pos / n_zero))
                assert kept == [want, want] and want == c64.downsample_count(n_pos, n_zero), (n_pos, n_zero)
    assert int(49 * (7 / 49)) == 7 and any(int(z * (p / z)) == p - 1 for p in range(1, 41) for z in range(p + 1, 41))


def test_negative_and_nan_targets():
    nan = float("nan")
    y = _targets(3, 20, extra=(-1.0, nan, -0.0))                  # -0.0 == 0: a zero row
    w = cfit.downsample_weights(y, 4, generator=torch.Generator().manual_seed(1))
    odd = (y < 0) | torch.isnan(y)
    assert int(odd.sum()) == 2 and (w[:, odd] == 0).all() and (w[:, y > 0] == 1).all()
    assert w[:, y == 0].sum(1).tolist() == [int(21 * (3 / 21))] * 4
    y = _targets(20, 3, extra=(-1.0, nan))
    w = cfit.downsample_weights(y, 4)
    assert (w == 1).all()                                        # the reference keeps the whole batch, these rows included
    assert tuple(cfit.downsample_weights(y, 0).shape) == (0, 25)
    for bad in (torch.zeros(2, 2), np.zeros(3)):
        with pytest.raises(ValueError, match="target must be a"):
            cfit.downsample_weights(bad, 1)
    with pytest.raises(ValueError, match="iters must be a non-negative integer"):
        cfit.downsample_weights(torch.zeros(3), -1)


def test_two_iterations_differ_and_a_seed_repeats():
    y = _targets(10, 50)
    w = cfit.downsample_weights(y, 2, generator=torch.Generator().manual_seed(3))
    assert (w[0] != w[1]).any()
    again = cfit.downsample_weights(y, 2, generator=torch.Generator().manual_seed(3))
    assert (w == again).all()


def test_tied_keys_keep_the_count_exact(monkeypatch):
    y = _targets(5, 30)
    monkeypatch.setattr(torch, "rand", lambda size, **kw: torch.full(size, 0.5, dtype=kw.get("dtype", torch.float32)))
    w = cfit.downsample_weights(y, 3)
    assert w[:, y == 0].sum(1).tolist() == [5, 5, 5] and (w[:, y > 0] == 1).all()


def test_every_zero_row_is_kept_equally_often():
    n_zero, k, iters = 50, 10, 2000
    y = _targets(k, n_zero)
    w = cfit.downsample_weights(y, iters, generator=torch.Generator().manual_seed(12345))
    counts = w[:, y == 0].sum(0).numpy()
    p = k / n_zero
    sigma = np.sqrt(iters * p * (1 - p))
    assert counts.sum() == iters * k and np.abs(counts - iters * p).max() < 5 * sigma


# ---------------------------------------------------------------------------------------------------------------------
# the float32 yardsticks of tests/test_gpu_cfit.py
# ---------------------------------------------------------------------------------------------------------------------
def _gpu_gradient_shapes():
    import test_gpu_cfit as t
    return sorted(set(t.gradient_shapes()))


def test_the_yardsticks_are_steady_over_the_seeds():
    """the whole vector's and the top block's yardstick: each seed's within 3 x of the median over seeds 0..3 at every shape
    the GPU test compares (the loss is one float32 number, whose error is anything between nothing and half an ulp: its
    yardstick is pooled over the seeds and floored at half an ulp, cfit64.pool_grads); and the fit's displacement"""
    worst = 0.0
    for head, regime, weighting, D, A, B in _gpu_gradient_shapes():
        yards = [c64.gradient_case(head, regime, weighting, D, A, B, s)["yard"] for s in c64.GRAD_SEEDS]
        for name, vals in (("g", [y[0] for y in yards]), ("block", [max(y[1].values()) for y in yards])):
            med = float(np.median(vals))
            for v in vals:
                worst = max(worst, v / med, med / v)
                assert med / 3 <= v <= 3 * med, (head, regime, weighting, D, A, B, name, vals)
    print(f"the yardsticks' worst distance from their median: {worst:.2f} x")
    for head, D, A, B in c64.FIT_SHAPES:
        yard = c64.fit_yardstick(head, D, A, B)
        each = []
        for s in c64.FIT_SEEDS:
            c = c64.fit_case(head, D, A, B, s)
            thetas, losses = c64.learners_loop(c, head)
            each.append(c64.fit_errors(thetas[-1], losses, c)[0])
        med = float(np.median(each))
        assert all(med / 3 <= v <= 3 * med for v in each), (head, D, A, B, each)
        assert yard[0] > 0 and yard[1] >= c64.HALF_ULP
