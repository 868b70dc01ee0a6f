"""guardx_amd.fisher on the device (libguardx_fisher.so) against tests/fisher64.py: the product at the tile, row and grid
edges, measured by its relative L2 error against float64 and held to 4x the same error of the learners' own method (a
float32 double backward through autograd, computed here on the CPU on the same inputs); its exact properties; and the
solve against the learners' float32 loop on the same problem.

Beyond the default-init actor (fisher64.REGIMES: default, trained, saturated, wide_log_std; tests/test_fisher64.py asserts
where each sits on tanh and that a plain numpy float32 evaluation meets every bound below at 2 x): the product pooled over 8
tangents (the root-mean-square of their errors), (a) the whole vector against its yardstick and (b) each of W1, b1, W2, b2,
W3, b3 against the largest of the six blocks' yardsticks; the learners' grid (256 workgroups that loop); properties that
hold to the bit (a repeated tile, F(2 x), F(-x)); symmetry; tanh_act by itself (gxf_tanh_act, the set and checks of
tests/math64.py); the solve's x_hat, s and r_dot after 1, 2, 3 and 10 iterations against cg64; its edges.

As these tests print on an MI355X (x the yardstick, ALLOWED = 4; the worst of workgroups = 0 and 2):
    D, A, B          default         trained         saturated       wide_log_std        (a) whole | (b) worst block
    43, 2, 1         1.31 | 1.22 W1  0.33 | 0.42 W1  0.60 | 0.74 W1  2.18 | 1.88 W1
    43, 2, 65        0.91 | 0.94 W1  0.92 | 0.90 W1  0.90 | 0.88 W1  0.98 | 0.87 b1
    64, 8, 130       0.59 | 0.74 W1  0.78 | 0.81 W1  0.77 | 0.91 b1  0.73 | 0.76 W1
    17, 16, 130      0.50 | 0.66 W1  0.68 | 0.81 W1  0.72 | 0.97 b1  0.70 | 0.68 W1
    43, 2, 16384 and 16385, default, the default grid: (a) 0.02 and 0.03 (yardstick 1.2e-06)
  B = 1 was 7.08 (default) and 10.74 (wide_log_std) while every sum of stages 1 to 3 was one chain: one row, two actions, and
  one tangent of the eight whose dmu is 1/50 of the sum of its terms' sizes; gx_fisher.hip:sum_acc is the remedy.
    tanh_act, ulp of the result     |x| < 0.625: 0.664 at x = 0.4553      from 0.625: 1.286 at x = 0.62522      stated: 2.3
    (8552462 inputs; -0 gave +0 before the copysignf in tanh_act; denormals are kept, tanh_act(x) = x there)
    the solve, worst of 3 regimes x 2 shapes x 2 grids      x_hat    s      r_dot
      1 iteration                                            0.65     0.42   0.46
      2                                                      0.46     0.29   0.50
      3                                                      0.53     0.45   0.60
      10                                                     0.64     0.25   0.64"""
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


# ---------------------------------------------------------------------------------------------------------------------
# the product beyond the default-init actor: the regimes of fisher64.REGIMES, pooled over 8 tangents, whole and per block
# ---------------------------------------------------------------------------------------------------------------------
REGIMES = list(f64.REGIMES)
EXACT_NETS = [(43, 2), (64, 8)]


def device_products(c, **kw):
    """F(x) for the tangents of a fisher64 case -> list of numpy float32"""
    F = operator(c["pi"], c["obs"], **kw)
    return [F(torch.from_numpy(x).cuda()).cpu().numpy() for x in c["xs"]]


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D,A,B", f64.PRODUCT_SHAPES)
def test_every_regime_whole_and_per_block(regime, D, A, B):
    """(a) the pooled whole-vector error within ALLOWED x the pooled yardstick; (b) each block's pooled error within
    ALLOWED x the largest of the six blocks' pooled yardsticks (the autograd bias gradients are pairwise sums and almost
    exact: a block's own yardstick is a noisy denominator)"""
    c = f64.product_case(regime, D, A, B)
    top = max(c["yard_blocks"].values())
    for wg in (0, 2):
        whole, blocks = f64.pool_products(device_products(c, workgroups=wg), c["wants"], D, A)
        print(f"{regime} D={D} A={A} B={B} workgroups={wg}: whole {whole / c['yard']:.2f}  " +
              "  ".join(f"{k} {blocks[k] / top:.2f}" for k in f64.BLOCKS) + f"   (yardsticks {c['yard']:.2e}, {top:.2e})")
        assert whole <= ALLOWED * c["yard"]
        for k in f64.BLOCKS:
            assert blocks[k] <= ALLOWED * top, k


@pytest.mark.parametrize("value", [-10.0, 2.0])
def test_the_log_std_block_at_its_ends(value):
    """log_std = -10: v = 2e-9 lies below eps = 1e-8, which then decides c (and makes it negative); +2: v = 55"""
    D, A, B = 43, 2, 65
    pi = f64.make_actor(D, A, 64, log_std=np.full(A, value))
    _, obs, x, _, _ = problem(D, A, B)
    only = torch.zeros_like(x)
    only[:A] = x[:A]
    y = operator(pi, obs, workgroups=3)(only.cuda()).cpu().numpy()
    assert not y[A:].any()
    c = f64.log_std_curvature(pi.log_std.detach().numpy())
    assert (c < 0).all() if value < 0 else (c > 0).all()
    np.testing.assert_allclose(y[:A], c * only[:A].numpy().astype(np.float64), rtol=2.0 ** -23, atol=0)


@pytest.mark.parametrize("B", [256 * 64, 256 * 64 + 1])
def test_the_learners_grid_loops(B):
    """workgroups = 0 is 256 workgroups from 16384 rows on; at 16385 workgroup 0 walks a second tile, of one row"""
    from guardx_amd import _fisher_native, fisher
    D, A = 43, 2
    assert _fisher_native.load().gxf_default_workgroups(B) == 256 and -(-B // 64) == 256 + B % 64
    c = f64.product_case("default", D, A, B)
    F = operator(c["pi"], c["obs"])
    xs = [torch.from_numpy(x).cuda() for x in c["xs"]]
    ys = [F(x) for x in xs]
    whole, _ = f64.pool_products([y.cpu().numpy() for y in ys], c["wants"], D, A)
    print(f"default D={D} A={A} B={B} workgroups=0: whole {whole / c['yard']:.2f}   (yardstick {c['yard']:.2e})")
    assert whole <= ALLOWED * c["yard"]
    assert bits(F(xs[0])) == bits(ys[0]) == bits(operator(c["pi"], c["obs"])(xs[0]))
    pad = 4096
    parent = torch.full((2 * pad + B * D,), float('nan'))
    parent[pad:pad + B * D] = c["obs"].reshape(-1)
    parent = parent.cuda()
    inside = parent[pad:pad + B * D].view(B, D)
    assert inside.is_contiguous() and torch.isnan(parent[pad - 1]) and torch.isnan(parent[pad + B * D])
    assert bits(fisher.FisherOperator(c["pi"], inside)(xs[0])) == bits(ys[0])
    assert np.isfinite(ys[0].cpu().numpy()).all()


@pytest.mark.parametrize("regime", ["default", "trained", "saturated"])
@pytest.mark.parametrize("D,A", EXACT_NETS)
def test_a_repeated_tile_gives_the_bits_of_one_tile(D, A, regime):
    """obs = one 64-row tile stacked k times: 1 / ((v + eps) k B) is the one tile's scaled by a power of two, everything
    after u is linear in u, t / 2 + t / 2 and t / 4 + t / 4 are exact in float32 and equal partials add exactly in
    float64, so the product has the bits of the one tile's -- unless a tile is read from the wrong rows, or something
    of one tile (LDS, the running sums) leaks into the next.  (k = 4 on one workgroup is not exact: 3 t / 4.)"""
    c = f64.product_case(regime, D, A, 130)
    tile = c["obs"][:64].contiguous()
    x = torch.from_numpy(c["xs"][0]).cuda()
    one = bits(operator(c["pi"], tile, workgroups=1)(x))
    assert any(one[A:])
    for k, grids in ((2, (1, 2)), (4, (2, 4))):
        stacked = tile.repeat(k, 1)
        assert tuple(stacked.shape) == (64 * k, D)
        for wg in grids:
            assert bits(operator(c["pi"], stacked, workgroups=wg)(x)) == one, (k, wg)


@pytest.mark.parametrize("regime", ["default", "trained", "saturated"])
@pytest.mark.parametrize("D,A", EXACT_NETS)
def test_the_product_is_homogeneous_to_the_bit(D, A, regime):
    """F(2 x) = 2 F(x) and F(-x) = -F(x): every operation after the activations is linear in x and rounds alike"""
    c = f64.product_case(regime, D, A, 130)
    x = torch.from_numpy(c["xs"][0]).cuda()
    for wg in (0, 2):
        F = operator(c["pi"], c["obs"], workgroups=wg)
        y = F(x)
        assert bits(F(2.0 * x)) == bits(2.0 * y)
        assert bits(F(-x)) == bits(-y)


@pytest.mark.parametrize("regime", REGIMES)
@pytest.mark.parametrize("D,A,B", [(43, 2, 65), (64, 8, 130)])
def test_the_operator_is_symmetric_and_positive_within_its_error(regime, D, A, B):
    """an error e (relative L2) in H x moves y . (H x) by at most e |y| |H x|: the argument of the solve's s"""
    c = f64.product_case(regime, D, A, B)
    F = operator(c["pi"], c["obs"])
    x, y = (c["xs"][i].astype(np.float64) for i in (0, 1))
    Hx, Hy = (F(torch.from_numpy(c["xs"][i]).cuda()).cpu().numpy().astype(np.float64) for i in (0, 1))
    bound = ALLOWED * c["yard"] * (np.linalg.norm(x) * np.linalg.norm(Hy) + np.linalg.norm(y) * np.linalg.norm(Hx))
    print(f"{regime} D={D} A={A} B={B}: |x.Hy - y.Hx| {abs(x @ Hy - y @ Hx):.3e}  bound {bound:.3e}  x.Hx {x @ Hx:.3e}  y.Hy {y @ Hy:.3e}")
    assert abs(x @ Hy - y @ Hx) <= bound
    assert x @ Hx >= -ALLOWED * c["yard"] * 2 * np.linalg.norm(x) * np.linalg.norm(Hx)
    assert y @ Hy >= -ALLOWED * c["yard"] * 2 * np.linalg.norm(y) * np.linalg.norm(Hy)


# ---------------------------------------------------------------------------------------------------------------------
# tanh_act by itself (gxf_tanh_act)
# ---------------------------------------------------------------------------------------------------------------------
def test_tanh_act_over_its_domain():
    """the set, the checks and the bound (2.3 ulp, the figure gx_fisher.hip states) of tests/test_math64.py's numpy
    restatement; this build keeps denormals (tests/test_gpu_math64.py (c)), so tanh_act(denormal) is the denormal"""
    import math64 as m
    from guardx_amd import _fisher_native as n
    x = m.tanh_act_set()
    xd = torch.from_numpy(np.array(x)).cuda()
    yd = torch.full_like(xd, float('nan'))
    n.check(n.load().gxf_tanh_act(x.size, xd.data_ptr(), yd.data_ptr(), None))
    torch.cuda.synchronize()
    m.check_tanh_act(x, yd.cpu().numpy(), "HIP")
    assert n.load().gxf_tanh_act(0, xd.data_ptr(), yd.data_ptr(), None) == n.GXF_OK


# ---------------------------------------------------------------------------------------------------------------------
# the solve, iterate by iterate
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("regime", list(f64.SOLVE_REGIMES))
@pytest.mark.parametrize("D,A,B", f64.SOLVE_SHAPES)
def test_the_iterates_against_cg64(regime, D, A, B):
    """x_hat (relative L2), s and r_dot (relative error) after 1, 2, 3 and 10 iterations against cg64 (and x' H64 x),
    pooled over 8 right-hand sides, within ALLOWED x the same errors of the learners' float32 loop around their float32
    double backward.  One iteration shows alpha, two show beta; `trained` is solved with damping = 0.1"""
    c = f64.solve_case(regime, D, A, B)
    for wg in (0, 2):
        F = operator(c["pi"], c["obs"], damping=c["damping"], workgroups=wg)
        xs, ss, rrs = [], [], []
        for g in c["gs"]:
            gd = torch.from_numpy(g).cuda()
            xk, sk, rk = {}, {}, {}
            for k in f64.SOLVE_ITERS:
                x_hat, s, info = F.solve(gd, iters=k)
                assert int(info['iters']) == k
                xk[k], sk[k], rk[k] = x_hat.cpu().numpy(), float(s), float(info['r_dot'])
            xs.append(xk)
            ss.append(sk)
            rrs.append(rk)
        got = f64.solve_errors(xs, ss, rrs, c)
        for k in f64.SOLVE_ITERS:
            print(f"{regime} D={D} A={A} B={B} workgroups={wg} iters={k}: " +
                  "  ".join(f"{w} {got[w, k] / c['yard'][w, k]:.2f} ({c['yard'][w, k]:.1e})" for w in ("x", "s", "r_dot")))
        for key, v in got.items():
            assert v <= ALLOWED * c["yard"][key], (wg, key)


def test_zero_iterations():
    pi, obs, g, _ = solve_problem()
    x_hat, s, info = operator(pi, obs).solve(g.cuda(), iters=0)
    assert bits(x_hat) == [0] * g.numel() and float(s) == 0.0 and int(info['iters']) == 0
    g64 = g.numpy().astype(np.float64)
    assert float(info['r_dot']) == float(np.float32(g64 @ g64))           # g . g in float64, rounded once


@pytest.mark.parametrize("bad", [float('nan'), float('inf')])
def test_a_gradient_that_is_not_finite_stops_at_once_and_leaves_nothing_behind(bad):
    pi, obs, g, _ = solve_problem()
    poisoned = g.clone()
    poisoned[1234] = bad
    F = operator(pi, obs)
    x_hat, s, info = F.solve(poisoned.cuda(), iters=10)
    assert int(info['iters']) == 0 and bits(x_hat) == [0] * g.numel() and float(s) == 0.0
    assert not np.isfinite(float(info['r_dot']))
    after = F.solve(g.cuda(), iters=5)
    fresh = operator(pi, obs).solve(g.cuda(), iters=5)
    for a, b in ((after[0], fresh[0]), (after[1], fresh[1]), (after[2]['r_dot'], fresh[2]['r_dot']), (after[2]['iters'], fresh[2]['iters'])):
        assert bits(a) == bits(b)
    assert int(after[2]['iters']) == 5 and np.isfinite(after[0].cpu().numpy()).all()


def test_a_product_after_a_stopped_solve():
    """the solve that stops early leaves the workspace's stop flag set; the product does not look at it"""
    pi, obs, g, _ = solve_problem()
    e = torch.zeros_like(g)
    e[0] = 1.0
    F = operator(pi, obs)
    before = bits(F(g.cuda()))
    _, _, info = F.solve(e.cuda(), iters=50)
    assert int(info['iters']) < 3
    assert bits(F(g.cuda())) == before and any(before)


def test_a_side_stream_gives_the_same_bits():
    pi, obs, g, _ = solve_problem()
    gd = g.cuda()
    F = operator(pi, obs)
    y = bits(F(gd))
    x_hat, s, info = F.solve(gd, iters=5)
    want = (y, bits(x_hat), bits(s), bits(info['r_dot']), bits(info['iters']))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        y2 = F(gd)
        x2, s2, info2 = F.solve(gd, iters=5)
    side.synchronize()
    assert (bits(y2), bits(x2), bits(s2), bits(info2['r_dot']), bits(info2['iters'])) == want


def test_two_solves_are_bit_identical():
    pi, obs, g, _ = solve_problem()
    runs = []
    for F in (operator(pi, obs, workgroups=3),) * 2 + (operator(pi, obs, workgroups=3),):
        x_hat, s, info = F.solve(g.cuda(), iters=10)
        runs.append((bits(x_hat), bits(s), bits(info['r_dot']), bits(info['iters'])))
    assert runs[0] == runs[1] == runs[2] and int(info['iters']) == 10
