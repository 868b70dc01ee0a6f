"""guardx_amd.vfit on the device (libguardx_vfit.so) against tests/vfit64.py: `gradient` at the tile, row, width and grid
edges, held to 4 x the error of the learners' own float32 backward (torch autograd on the CPU, on the same inputs); its exact
properties; tanh_act by itself; one Adam step against adam64 to the ulp; `fit` against fit64, held to 4 x the error of the
learners' float32 loop (autograd + torch.optim.Adam on the CPU).

The gradient's errors (vfit64.grad_errors): the relative L2 of the whole vector and of each of W1, b1, W2, b2, W3, b3, and the
relative error of the loss, each pooled over three seeds (root-mean-square).  The whole vector and the loss are held to their
own yardsticks; a block to the largest of the six blocks' yardsticks, as tests/test_gpu_fisher.py holds its blocks (b3 is one
number, whose float32 error is anything between nothing and an ulp).  The fit's (vfit64.fit_errors): the relative L2 of the
displacement theta_k - theta_0 and the largest relative error of the first k losses, pooled over four seeds that
tests/test_vfit64.py shows to be well conditioned.

As these tests print on an MI355X (x the yardstick, ALLOWED = 4; the worst of the grids workgroups = 1, 3, tiles + 3, 0):
    gradient, default regime        g | worst block | loss
    D, B = 43, 1                    0.92 | 1.04 W1 | 0.57        44, 1      1.00 | 1.00 W1 | 1.00        64, 1      1.00 | 1.15 W1 | 0.87
           43, 63                   0.95 | 0.92 W1 | 0.10        44, 63     1.09 | 0.94 W1 | 0.62        64, 63     0.86 | 0.97 W1 | 0.40
           43, 64                   1.05 | 0.96 W1 | 0.13        44, 64     1.16 | 0.96 W1 | 0.36        64, 64     1.14 | 0.96 W1 | 0.35
           43, 65                   0.93 | 0.95 W1 | 1.00        44, 65     1.03 | 1.01 W1 | 1.18        64, 65     1.04 | 0.97 W1 | 0.54
           43, 257                  0.63 | 0.80 W1 | 0.31        44, 257    0.62 | 0.84 W1 | 1.00        64, 257    0.64 | 0.82 W1 | 0.29
           43, 4099                 0.28 | 0.22 W1 | 0.32        44, 4099   0.26 | 0.26 W1 | 0.33        64, 4099   0.40 | 0.30 W1 | 0.41
    B = 130, D = 1                  0.61 | 0.88 W1 | 0.34        D = 16     0.79 | 0.88 W1 | 0.21        D = 17     0.93 | 0.83 W1 | 0.22
             D = 32                 0.82 | 0.80 W1 | 0.44        D = 65     1.10 | 0.86 W1 | 0.31        D = 72     0.84 | 0.80 W1 | 0.39
             D = 73                 0.82 | 0.84 W1 | 0.30        D = 96     0.71 | 0.82 W1 | 0.59        D = 97     0.93 | 0.82 W1 | 0.51
             D = 128                0.99 | 0.83 W1 | 0.26
    D, B = 43, 257: trained         0.65 | 0.77 W1 | 0.64        saturated  0.72 | 0.85 W1 | 0.52
    D, B = 43, 16385, default grid  0.03 | 0.07 W1 | 0.73        (yardstick 9.0e-07: torch's float32 sums grow with B, the tiles' do not)
    tanh_act, ulp of the result     |x| < 0.625: 0.664 at x = 0.4553      from 0.625: 1.286 at x = 0.62522      stated: 2.3
    gxv_adam_step at t = 1, 2, 1000 0 of 10007 stored values of theta, m and v differ from adam64's
    fit, displacement | loss trace  k = 1          k = 2          k = 3          k = 10         5 + 5
    D, B = 43, 257                  1.02 | 0.47    0.90 | 0.51    0.92 | 0.42    0.95 | 0.53    0.95 | 0.53
    D, B = 64, 130                  0.99 | 0.36    0.98 | 0.51    0.98 | 0.55    0.99 | 0.48    0.99 | 0.48
  (the worst of workgroups = 0 and 2; the displacement's yardstick is 2.2e-06 at one step and 8.6e-07 at ten: the float32
  rounding of theta against steps of size lr, which the kernel shares, hence ratios near 1)"""
import copy

import numpy as np
import pytest
import torch

import vfit64 as v64

pytestmark = pytest.mark.gpu

ALLOWED = v64.ALLOWED


def fitter(critic, **kw):
    """a ValueFit around a copy of `critic` on the device (the case's own critic is shared and never written to)"""
    from guardx_amd import vfit
    kw.setdefault("lr", v64.LR)
    return vfit.ValueFit(copy.deepcopy(critic).cuda(), **kw)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).reshape(-1).tolist()


def check_gradient(regime, D, B, grids):
    cases = [v64.gradient_case(regime, D, B, s) for s in v64.GRAD_SEEDS]
    yard, yard_blocks, yard_loss = v64.pool_grads([c["yard"] for c in cases])
    top = max(yard_blocks.values())
    for wg in grids:
        errs = []
        for c in cases:
            g, loss = fitter(c["critic"], workgroups=wg).gradient(c["obs"].cuda(), c["ret"].cuda())
            assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (v64.param_count(D),)
            assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0
            errs.append(v64.grad_errors(g.cpu().numpy(), float(loss), c["g"], c["loss"], D))
        whole, blocks, le = v64.pool_grads(errs)
        worst = max(blocks, key=blocks.get)
        print(f"{regime} D={D} B={B} workgroups={wg}: g {whole:.2e} / {yard:.2e} = {whole / yard:.2f}  worst block {worst} "
              f"{blocks[worst]:.2e} / {top:.2e} = {blocks[worst] / top:.2f}  loss {le:.2e} / {yard_loss:.2e} = {le / yard_loss:.2f}")
        assert whole <= ALLOWED * yard, wg
        for k in v64.BLOCKS:
            assert blocks[k] <= ALLOWED * top, (wg, k)
        assert le <= ALLOWED * yard_loss, wg


@pytest.mark.parametrize("B", v64.GRAD_ROWS)
@pytest.mark.parametrize("D", v64.GRAD_WIDTHS)
def test_gradient_against_grad64(D, B):
    tiles = -(-B // 64)
    check_gradient("default", D, B, (1, 3, tiles + 3, 0))


@pytest.mark.parametrize("D", v64.EDGE_WIDTHS)
def test_every_first_layer_instantiation_at_its_edges(D):
    check_gradient("default", D, v64.EDGE_ROWS, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("regime", list(v64.REGIMES))
def test_every_regime(regime):
    check_gradient(regime, 43, 257, (1, 3, 5 + 3, 0))


def test_a_workgroup_walks_a_second_tile_at_the_default_grid():
    """workgroups = 0 is 256 workgroups from 16384 rows on; at 16385 workgroup 0 walks a second tile, of one row"""
    from guardx_amd import _vfit_native
    assert _vfit_native.load().gxv_default_workgroups(16385) == 256 and -(-16385 // 64) == 257
    check_gradient("default", 43, 16385, (0,))


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("D,B", [(43, 257), (64, 4099)])
def test_two_calls_give_the_same_bits(D, B):
    c = v64.gradient_case("default", D, B, 0)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    for wg in (0, 3):
        VF = fitter(c["critic"], workgroups=wg)
        first = [bits(t) for t in VF.gradient(obs, ret)]
        assert first == [bits(t) for t in VF.gradient(obs, ret)] == [bits(t) for t in fitter(c["critic"], workgroups=wg).gradient(obs, ret)]
        assert np.isfinite(VF.gradient(obs, ret)[0].cpu().numpy()).all()
        a, b = fitter(c["critic"], workgroups=wg), fitter(c["critic"], workgroups=wg)
        ia, ib = a.fit(obs, ret, iters=3), b.fit(obs, ret, iters=3)
        assert bits(ia["theta"]) == bits(ib["theta"]) and bits(ia["loss"]) == bits(ib["loss"]) and bits(a.m) == bits(b.m) and bits(a.v) == bits(b.v)


@pytest.mark.parametrize("D,B", [(43, 257), (64, 63)])
def test_idle_workgroups_add_exact_zeros(D, B):
    c = v64.gradient_case("default", D, B, 0)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    tiles = -(-B // 64)
    want = [bits(t) for t in fitter(c["critic"], workgroups=tiles).gradient(obs, ret)]
    for extra in (1, 5, 300):
        assert [bits(t) for t in fitter(c["critic"], workgroups=tiles + extra).gradient(obs, ret)] == want, extra


@pytest.mark.parametrize("D,B", [(43, 65), (64, 63), (43, 1)])
def test_rows_inside_a_larger_buffer(D, B):
    """obs and ret inside larger buffers whose other entries are NaN: neither the rows past B - 1 of the last tile nor the
    columns a row is padded with in LDS come from memory"""
    c = v64.gradient_case("default", D, B, 0)
    tight = {"obs": c["obs"].cuda(), "ret": c["ret"].cuda()}
    pad, inside = 4096, {}
    for k, t in tight.items():
        parent = torch.full((2 * pad + t.numel(),), float('nan'), device="cuda")
        parent[pad:pad + t.numel()] = t.reshape(-1)
        inside[k] = parent[pad:pad + t.numel()].view(t.shape)
        assert inside[k].is_contiguous()
    for wg in (0, 2):
        plain = fitter(c["critic"], workgroups=wg).gradient(tight["obs"], tight["ret"])
        got = fitter(c["critic"], workgroups=wg).gradient(inside["obs"], inside["ret"])
        assert [bits(t) for t in got] == [bits(t) for t in plain] and np.isfinite(plain[0].cpu().numpy()).all()


def test_tanh_act_over_its_domain():
    """the set, the checks and the bound (2.3 ulp, the figure gx_vfit.hip states) of tests/math64.py"""
    import math64 as m
    from guardx_amd import _vfit_native as n
    x = m.tanh_act_set()
    xd = torch.from_numpy(np.array(x)).cuda()
    yd = torch.full_like(xd, float('nan'))
    n.check(n.load().gxv_tanh_act(x.size, xd.data_ptr(), yd.data_ptr(), None))
    torch.cuda.synchronize()
    m.check_tanh_act(x, yd.cpu().numpy(), "HIP vfit")
    assert n.load().gxv_tanh_act(0, xd.data_ptr(), yd.data_ptr(), None) == n.GXV_OK


# ---------------------------------------------------------------------------------------------------------------------
# one Adam step (gxv_adam_step)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t", [1, 2, 1000])
def test_adam_step_against_adam64(t):
    """random g, m, v, theta with g = 0, v = 0 and denormal m among them: each stored value within 1 float32 ulp of adam64's
    (the float64 evaluation is the same operations in the same order, so it can differ from numpy's only where a library
    function does, and the stored value only at a rounding tie)"""
    import ctypes as C
    from guardx_amd import _vfit_native as n
    rng = np.random.default_rng(t)
    P = 10007
    theta = rng.standard_normal(P).astype(np.float32)
    g = (rng.standard_normal(P) * 10.0 ** rng.uniform(-8, 2, P)).astype(np.float32)
    m = (rng.standard_normal(P) * 10.0 ** rng.uniform(-8, 2, P)).astype(np.float32)
    v = ((rng.standard_normal(P) * 10.0 ** rng.uniform(-8, 2, P)) ** 2).astype(np.float32)
    g[::7] = 0.0
    v[::11] = 0.0
    m[::13] = (rng.standard_normal(m[::13].size) * 1e-40).astype(np.float32)
    m[::77] = 0.0                                                 # with g = 0 and v = 0 among them: 0 / (0 + eps)
    assert ((g == 0) & (v == 0) & (m == 0)).any() and ((np.abs(m) > 0) & (np.abs(m) < 1.2e-38)).any()
    b1, b2 = v64.BETAS
    want = v64.adam64(theta, m, v, g, t, v64.LR, v64.BETAS, v64.EPS, store=np.float32)
    dev = [torch.from_numpy(x.copy()).cuda() for x in (theta, m, v, g)]
    hyper = (C.c_double * 6)(v64.LR, b1, b2, v64.EPS, b1 ** t, b2 ** t)
    n.check(n.load().gxv_adam_step(P, *[x.data_ptr() for x in dev], C.cast(hyper, C.c_void_p), None))
    torch.cuda.synchronize()
    assert bits(dev[3]) == bits(torch.from_numpy(g))              # the gradient is read only
    for name, got, w in zip(("theta", "m", "v"), dev, want):
        got = got.cpu().numpy()
        differ = int((got.view(np.int32) != w.view(np.int32)).sum())
        print(f"t={t} {name}: {differ} of {P} stored values differ from adam64's")
        assert np.isfinite(got).all()
        assert (np.abs(got.astype(np.float64) - w.astype(np.float64)) <= np.spacing(np.abs(w)).astype(np.float64)).all(), name


# ---------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------
def _run(c, calls, wg):
    """(theta after the calls, the loss trace, the ValueFit) of consecutive fit calls of `calls` iterations"""
    VF = fitter(c["critic"], workgroups=wg)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    losses = []
    for n in calls:
        info = VF.fit(obs, ret, iters=n)
        losses.append(info["loss"])
    return info["theta"].cpu().numpy(), torch.cat(losses).cpu().numpy(), VF


@pytest.mark.parametrize("wg", [0, 2])
@pytest.mark.parametrize("D,B", v64.FIT_SHAPES)
def test_fit_against_fit64(D, B, wg):
    yard = v64.fit_yardstick(D, B)
    errs, split = [], []
    for seed in v64.FIT_SEEDS[D, B]:
        c = v64.fit_case(D, B, seed)
        thetas, losses = {}, None
        for k in v64.FIT_KS:
            thetas[k], losses, VF = _run(c, (k,), wg)
            assert VF.step == k
        errs.append(v64.fit_errors(thetas, losses, c))
        theta, trace, VF = _run(c, (5, 5), wg)                    # the moments and the step count carry over
        assert VF.step == 10
        split.append(dict(theta=v64.rel_l2(theta.astype(np.float64) - c["theta"], c["thetas"][10] - c["theta"]),
                          loss=max(v64.rel_err(trace[i], c["losses"][i]) for i in range(10))))
        assert theta.view(np.int32).tolist() == thetas[10].view(np.int32).tolist() and bits(torch.from_numpy(trace)) == bits(torch.from_numpy(losses))
    err = v64.pool_fits(errs)
    for k in v64.FIT_KS:
        print(f"D={D} B={B} workgroups={wg} k={k}: displacement {err['theta', k]:.2e} / {yard['theta', k]:.2e} = "
              f"{err['theta', k] / yard['theta', k]:.2f}  loss trace {err['loss', k]:.2e} / {yard['loss', k]:.2e} = "
              f"{err['loss', k] / yard['loss', k]:.2f}")
    st, sl = v64.pooled([s["theta"] for s in split]), v64.pooled([s["loss"] for s in split])
    print(f"D={D} B={B} workgroups={wg} 5 + 5: displacement {st:.2e} / {yard['theta', 10]:.2e} = {st / yard['theta', 10]:.2f}  "
          f"loss trace {sl:.2e} / {yard['loss', 10]:.2e} = {sl / yard['loss', 10]:.2f}")
    for k in v64.FIT_KS:
        assert err["theta", k] <= ALLOWED * yard["theta", k], k
        assert err["loss", k] <= ALLOWED * yard["loss", k], k
    assert st <= ALLOWED * yard["theta", 10] and sl <= ALLOWED * yard["loss", 10]


def test_the_module_holds_the_flat_result_and_the_first_loss_is_the_gradients():
    c = v64.fit_case(43, 257, 1)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    VF = fitter(c["critic"])
    assert bits(v64.flat(VF.critic)) == bits(torch.from_numpy(c["theta"]))
    _, loss0 = VF.gradient(obs, ret)
    info = VF.fit(obs, ret, iters=4)
    assert all(t.is_cuda for t in info.values()) and info["loss"].dtype == torch.float32 and tuple(info["loss"].shape) == (4,)
    assert int(info["step"]) == VF.step == 4 and info["step"].dtype == torch.int64
    assert bits(v64.flat(VF.critic)) == bits(info["theta"]) != bits(torch.from_numpy(c["theta"]))
    assert bits(info["loss"][0]) == bits(loss0)
    assert all(p.is_cuda for p in VF.critic.parameters())
    # the next gradient is taken at the fitted parameters: its loss is what a fifth iteration would report
    _, loss4 = VF.gradient(obs, ret)
    again = VF.fit(obs, ret, iters=1)
    assert bits(again["loss"][0]) == bits(loss4) and VF.step == 5
    assert float(info["loss"][0]) > float(info["loss"][3]) > float(loss4)      # it descends


def test_zero_iterations_change_nothing():
    c = v64.fit_case(64, 130, 0)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    VF = fitter(c["critic"])
    VF.fit(obs, ret, iters=2)
    before = (bits(v64.flat(VF.critic)), bits(VF.m), bits(VF.v), VF.step)
    info = VF.fit(obs, ret, iters=0)
    assert tuple(info["loss"].shape) == (0,) and int(info["step"]) == 2
    assert (bits(v64.flat(VF.critic)), bits(VF.m), bits(VF.v), VF.step) == before == (bits(info["theta"]),) + before[1:]


def test_a_side_stream_gives_the_same_bits():
    c = v64.fit_case(43, 257, 2)
    obs, ret = c["obs"].cuda(), c["ret"].cuda()
    want = fitter(c["critic"]).fit(obs, ret, iters=3)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = fitter(c["critic"]).fit(obs, ret, iters=3)
    side.synchronize()
    assert bits(got["theta"]) == bits(want["theta"]) and bits(got["loss"]) == bits(want["loss"])
