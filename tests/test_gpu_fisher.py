"""guardx_amd.fisher on the device (libguardx_fisher.so) against tests/fisher64.py: the product at the tile, row and grid
edges, measured by its relative L2 error against float64 and held to 4x the same error of the learners' own method (a
float32 double backward through autograd, computed here on the CPU on the same inputs); its exact properties; and the
solve against the learners' float32 loop on the same problem."""
import functools

import numpy as np
import pytest
import torch

import fisher64 as f64

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 64, 65, 257, 4099]
NETS = [(43, 2), (44, 2), (46, 2), (64, 8)]
ALLOWED = 4.0            # x the yardstick: another order of the sum over rows, another tanh


@functools.lru_cache(maxsize=None)
def problem(D, A, B, seed=0):
    """actor, obs, x (float32, on the CPU), H64 x and the yardstick: the error of the float32 double backward"""
    pi = f64.make_actor(D, A, 64, seed=seed)
    gen = torch.Generator().manual_seed(100 + seed)
    obs = torch.randn(B, D, generator=gen)
    x = torch.randn(f64.param_count(D, A, 64), generator=gen)
    theta = f64.flat(pi).numpy()
    want = f64.fvp64(theta, x.numpy(), obs.numpy(), A, 64)
    yard = f64.rel_l2(f64.autograd_fvp(pi, obs, x).numpy(), want)
    return pi, obs, x, want, yard


def operator(pi, obs, **kw):
    from guardx_amd import fisher
    return fisher.FisherOperator(pi, obs.cuda(), **kw)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).tolist()


@pytest.mark.parametrize("B", ROWS)
@pytest.mark.parametrize("D,A", NETS)
def test_the_product_against_float64(D, A, B):
    pi, obs, x, want, yard = problem(D, A, B)
    tiles = -(-B // 64)
    for wg in (1, 3, tiles + 3, 0):
        y = operator(pi, obs, workgroups=wg)(x.cuda())
        assert y.is_cuda and y.dtype == torch.float32 and tuple(y.shape) == tuple(x.shape)
        err = f64.rel_l2(y.cpu().numpy(), want)
        print(f"D={D} A={A} B={B} workgroups={wg}: kernel {err:.3e}  float32 autograd {yard:.3e}  ratio {err / yard:.2f}")
        assert err <= ALLOWED * yard


# one width per first-layer instantiation of the kernel (pad4(D) / 4 k-steps rounded up to 4, 8, 11, 12, 16, 18, 24, 32;
# 11, 12 and 16 are NETS' above), at its edges, with the widest action block: the obs tile's LDS stride, the number of
# W1 column tiles and the registers a lane keeps all change with it
WIDTHS = [(1, 2), (16, 4), (17, 2), (32, 6), (65, 2), (70, 10), (72, 2), (73, 12), (96, 14), (97, 2), (128, 16)]


@pytest.mark.parametrize("D,A", WIDTHS)
def test_every_first_layer_width(D, A):
    B = 130                                                   # two full tiles and two rows
    pi, obs, x, want, yard = problem(D, A, B)
    for wg in (0, 2):
        err = f64.rel_l2(operator(pi, obs, workgroups=wg)(x.cuda()).cpu().numpy(), want)
        print(f"D={D} A={A} B={B} workgroups={wg}: kernel {err:.3e}  float32 autograd {yard:.3e}  ratio {err / yard:.2f}")
        assert err <= ALLOWED * yard


def test_numpy_in_numpy_out():
    pi, obs, x, want, yard = problem(43, 2, 257)
    F = operator(pi, obs)
    y = F(x.numpy())
    assert isinstance(y, np.ndarray) and y.dtype == np.float32
    assert bits(torch.from_numpy(y)) == bits(F(x.cuda()))


@pytest.mark.parametrize("D,A,B", [(43, 2, 257), (64, 8, 4099)])
def test_two_calls_are_bit_identical(D, A, B):
    pi, obs, x, _, _ = problem(D, A, B)
    for wg in (0, 3):
        F = operator(pi, obs, workgroups=wg)
        first = bits(F(x.cuda()))
        assert first == bits(F(x.cuda())) == bits(operator(pi, obs, workgroups=wg)(x.cuda()))


@pytest.mark.parametrize("D,A,B", [(43, 2, 65), (64, 8, 257)])
def test_zero_gives_zero_and_log_std_stands_alone(D, A, B):
    pi, obs, x, _, _ = problem(D, A, B)
    F = operator(pi, obs, workgroups=3)
    assert bits(F(torch.zeros_like(x).cuda())) == [0] * x.numel()
    only = torch.zeros_like(x)
    only[:A] = x[:A]
    y = F(only.cuda()).cpu().numpy()
    assert not y[A:].any()
    c = f64.log_std_curvature(pi.log_std.detach().numpy())
    # c is evaluated in float64 and rounded once on the device; its exp need not be numpy's to the last bit: one ulp
    np.testing.assert_allclose(y[:A], c * only[:A].numpy().astype(np.float64), rtol=2.0 ** -23, atol=0)


def test_damping_adds_exactly_damping_x():
    pi, obs, x, _, _ = problem(46, 2, 257)
    y0 = operator(pi, obs)(x.cuda()).cpu().numpy()
    yd = operator(pi, obs, damping=0.1)(x.cuda()).cpu().numpy()
    want = y0 + np.float32(0.1) * x.numpy()                   # float32 throughout: one product, one sum
    assert want.dtype == np.float32 and yd.view(np.int32).tolist() == want.view(np.int32).tolist()


@pytest.mark.parametrize("D,A,B", [(43, 2, 65), (46, 2, 1), (64, 8, 63)])
def test_nothing_around_obs_is_read(D, A, B):
    """obs inside a larger buffer of NaN: neither the rows after row B - 1 of the last tile nor the columns a row is
    padded with in LDS come from memory"""
    from guardx_amd import fisher
    pi, obs, x, _, _ = problem(D, A, B)
    pad = 4096
    parent = torch.full((2 * pad + B * D,), float('nan'))
    parent[pad:pad + B * D] = obs.reshape(-1)
    parent = parent.cuda()
    inside = parent[pad:pad + B * D].view(B, D)
    assert inside.is_contiguous() and torch.isnan(parent[pad - 1]) and torch.isnan(parent[pad + B * D])
    for wg in (0, 2):
        plain = operator(pi, obs, workgroups=wg)(x.cuda())
        assert bits(fisher.FisherOperator(pi, inside, workgroups=wg)(x.cuda())) == bits(plain)
        assert np.isfinite(plain.cpu().numpy()).all()


# ---------------------------------------------------------------------------------------------------------------------
# the solve
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def solve_problem():
    D, A, B = 43, 2, 4099
    pi, obs, _, _, _ = problem(D, A, B)
    gen = torch.Generator().manual_seed(7)
    g = torch.randn(f64.param_count(D, A, 64), generator=gen)
    theta = f64.flat(pi).numpy()
    H64 = lambda v: f64.fvp64(theta, v, obs.numpy(), A, 64)    # noqa: E731
    return pi, obs, g, H64


@pytest.mark.parametrize("iters", [10, 100])
def test_the_solve_against_the_learners_loop(iters):
    pi, obs, g, H64 = solve_problem()
    F = operator(pi, obs)
    x_hat, s, info = F.solve(g.cuda(), iters=iters)
    assert all(t.is_cuda for t in (x_hat, s, info['iters'], info['r_dot']))
    assert s.dtype == torch.float32 and info['iters'].dtype == torch.int32 and int(info['iters']) == iters
    xh = x_hat.cpu().numpy().astype(np.float64)
    gn = g.numpy().astype(np.float64)
    res = np.linalg.norm(H64(xh) - gn) / np.linalg.norm(gn)
    Hx32 = lambda v: f64.autograd_fvp(pi, obs, torch.from_numpy(v)).numpy()    # noqa: E731
    x_ref = f64.learners_cg32(Hx32, g.numpy(), iters).astype(np.float64)
    res_ref = np.linalg.norm(H64(x_ref) - gn) / np.linalg.norm(gn)
    print(f"iters={iters}: |H64 x - g| / |g| device {res:.4e}  learners' float32 loop {res_ref:.4e}  ratio {res / res_ref:.3f}")
    assert res <= 2.0 * res_ref
    # s = x' H x to the product's tolerance: an error e (relative L2) in H x moves x . (H x) by at most e |x| |H x|;
    # s itself is rounded once to float32
    hx = H64(xh)
    yard = f64.rel_l2(Hx32(x_hat.cpu().numpy()), hx)
    s64 = float(xh @ hx)
    print(f"iters={iters}: s device {float(s):.8e}  float64 {s64:.8e}  float32 autograd product error {yard:.3e}")
    assert abs(float(s) - s64) <= ALLOWED * yard * np.linalg.norm(xh) * np.linalg.norm(hx) + 2.0 ** -24 * abs(s64)
    assert np.isfinite(float(info['r_dot'])) and float(info['r_dot']) >= 0


def test_zero_gradient_gives_zero():
    pi, obs, g, _ = solve_problem()
    x_hat, s, info = operator(pi, obs).solve(torch.zeros_like(g).cuda(), iters=10)
    assert bits(x_hat) == [0] * g.numel() and float(s) == 0.0 and float(info['r_dot']) == 0.0 and int(info['iters']) == 0


def test_the_early_stop_freezes_the_solution():
    """g along one log_std axis is an eigenvector (H is diagonal there, and nothing couples log_std to the net): one
    step solves it, |p| falls below eps, and later iterations leave x_hat as it is"""
    pi, obs, g, _ = solve_problem()
    e = torch.zeros_like(g)
    e[0] = 1.0
    F = operator(pi, obs)
    x3, s3, i3 = F.solve(e.cuda(), iters=3)
    x50, s50, i50 = F.solve(e.cuda(), iters=50)
    c0 = f64.log_std_curvature(pi.log_std.detach().numpy())[0]
    assert int(i3['iters']) == int(i50['iters']) < 3
    assert bits(x3) == bits(x50) and bits(s3) == bits(s50) and bits(i3['r_dot']) == bits(i50['r_dot'])
    got = x3.cpu().numpy()
    assert not got[1:].any() and abs(got[0] - 1.0 / c0) <= 1e-6 / c0
