"""tests/fisher64.py, the float64 oracle of the Fisher-vector product, against the learners' own method in float64 (a
double backward through autograd of the KL as they write it), its parameter order, the shape of the matrix it applies,
and whether such a comparison would notice a mistake.  No GPU."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import fisher64 as f64

SHAPES = [(43, 2, 2000), (64, 8, 2000), (44, 2, 65)]      # D, A, B
HERE = os.path.dirname(os.path.abspath(__file__))


def _problem(D, A, B, h, seed=0):
    pi = f64.make_actor(D, A, h, seed=seed, dtype=torch.float64)
    gen = torch.Generator().manual_seed(seed + 1)
    obs = torch.randn(B, D, generator=gen, dtype=torch.float64)
    x = torch.randn(f64.param_count(D, A, h), generator=gen, dtype=torch.float64)
    return pi, obs, x


@pytest.mark.parametrize("h", [8, 64])
@pytest.mark.parametrize("D,A,B", SHAPES)
def test_the_closed_form_is_the_double_backward(D, A, B, h):
    pi, obs, x = _problem(D, A, B, h)
    want = f64.autograd_fvp(pi, obs, x).numpy()
    got = f64.fvp64(f64.flat(pi).numpy(), x.numpy(), obs.numpy(), A, h)
    err = f64.rel_l2(got, want)
    print(f"D={D} A={A} B={B} h={h}: relative L2 {err:.3e}")
    assert err <= 1e-12


def test_damping_adds_damping_x():
    pi, obs, x = _problem(44, 2, 65, 8)
    th = f64.flat(pi).numpy()
    np.testing.assert_allclose(f64.fvp64(th, x.numpy(), obs.numpy(), 2, 8, damping=0.25),
                               f64.fvp64(th, x.numpy(), obs.numpy(), 2, 8) + 0.25 * x.numpy(), rtol=0, atol=1e-15)


@pytest.mark.parametrize("D,A,h", [(43, 2, 64), (64, 8, 64), (5, 4, 8)])
def test_the_order_is_that_of_the_actors_parameters(D, A, h):
    pi = f64.make_actor(D, A, h, dtype=torch.float64)
    names = [n for n, _ in pi.named_parameters()]
    assert names == ["log_std", "mu_net.0.weight", "mu_net.0.bias", "mu_net.2.weight", "mu_net.2.bias", "mu_net.4.weight",
                     "mu_net.4.bias"]
    flat = torch.cat([p.flatten() for p in pi.parameters()]).detach().numpy()
    assert flat.shape == (f64.param_count(D, A, h),)
    ls, W1, b1, W2, b2, W3, b3 = f64.unpack(flat, D, A, h)
    lin = [m for m in pi.mu_net if isinstance(m, torch.nn.Linear)]
    for got, want in zip((ls, W1, b1, W2, b2, W3, b3), [pi.log_std] + [t for m in lin for t in (m.weight, m.bias)]):
        np.testing.assert_array_equal(got, want.detach().numpy())
    np.testing.assert_array_equal(f64.pack((ls, W1, b1, W2, b2, W3, b3)), flat)
    from guardx_amd import fisher
    assert fisher.param_count(D, A, h) == flat.size
    np.testing.assert_array_equal(fisher.flat_params(pi).numpy(), flat.astype(np.float32))


def test_the_dense_matrix_of_a_tiny_net_is_symmetric_and_positive_semidefinite():
    D, A, B, h = 3, 2, 40, 4
    pi, obs, _ = _problem(D, A, B, h)
    H = f64.dense64(f64.flat(pi).numpy(), obs.numpy(), A, h)
    scale = np.abs(H).max()
    assert np.abs(H - H.T).max() <= 1e-14 * scale
    eig = np.linalg.eigvalsh(0.5 * (H + H.T))
    assert eig.min() >= -1e-13 * eig.max() and eig.max() > 0
    # no cross terms between log_std and the net; the log_std block is diagonal
    assert not H[:A, A:].any() and not H[A:, :A].any()
    np.testing.assert_array_equal(H[:A, :A], np.diag(f64.log_std_curvature(pi.log_std.detach().numpy())))


# planted mistakes: (what the source says, what the copy says instead)
MISTAKES = {
    "the W2 dh1 term dropped": ("(h1 @ dW2.T + dh1 @ W2.T + db2)", "(h1 @ dW2.T + db2)"),
    "eps dropped": ("u = dmu / (np.exp(2.0 * ls) + eps) / B", "u = dmu / np.exp(2.0 * ls) / B"),
    "log_std placed last": ('sizes = [("ls", (A,)), ("W1", (h, D)), ("b1", (h,)), ("W2", (h, h)), ("b2", (h,)), ("W3", (A, h)), ("b3", (A,))]',
                            'sizes = [("W1", (h, D)), ("b1", (h,)), ("W2", (h, h)), ("b2", (h,)), ("W3", (A, h)), ("b3", (A,)), ("ls", (A,))]'),
}


@pytest.mark.parametrize("name", list(MISTAKES))
def test_a_planted_mistake_is_caught(name, tmp_path):
    old, new = MISTAKES[name]
    src = open(os.path.join(HERE, "fisher64.py")).read()
    assert src.count(old) == 1
    if name == "log_std placed last":          # unpack() then returns the parts in that order: name them accordingly
        first = "    return out\n"
        assert src.count(first) == 1
        src = src.replace(first, "    return [out[-1]] + out[:-1]\n")
    path = tmp_path / "fisher64_mistaken.py"
    path.write_text(src.replace(old, new))
    spec = importlib.util.spec_from_file_location("fisher64_mistaken", str(path))
    bad = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bad)
    # eps = 1e-2 for this check alone, so that dropping it is far above rounding
    eps = 1e-2
    D, A, B, h = 44, 2, 65, 8
    pi, obs, x = _problem(D, A, B, h)
    want = f64.autograd_fvp(pi, obs, x, eps=eps).numpy()
    th = f64.flat(pi).numpy()
    assert f64.rel_l2(f64.fvp64(th, x.numpy(), obs.numpy(), A, h, eps=eps), want) <= 1e-12
    err = f64.rel_l2(bad.fvp64(th, x.numpy(), obs.numpy(), A, h, eps=eps), want)
    print(f"{name}: relative L2 {err:.3e}")
    assert err > 1e-6


def test_cg64_solves_and_stops():
    D, A, B, h = 5, 2, 200, 4
    pi, obs, g = _problem(D, A, B, h)
    th = f64.flat(pi).numpy()
    Hx = lambda v: f64.fvp64(th, v, obs.numpy(), A, h, damping=1.0)   # noqa: E731  (well conditioned)
    x, done, rr = f64.cg64(Hx, g.numpy(), iters=200)
    print("iterations", done, "residual", np.linalg.norm(Hx(x) - g.numpy()) / np.linalg.norm(g.numpy()))
    # the learners' alpha = rr / (p.z + eps) stops shrinking the residual once p.z is of the order of eps, i.e. (the
    # eigenvalues are >= 1 here) once |r| is of the order of sqrt(eps): that is the floor this loop reaches, not zero
    assert 0 < done <= 200 and np.linalg.norm(Hx(x) - g.numpy()) <= np.sqrt(f64.EPS)
    x0, done0, rr0 = f64.cg64(Hx, np.zeros_like(th), iters=10)
    assert not x0.any() and done0 == 0 and rr0 == 0.0
