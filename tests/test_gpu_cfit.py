"""guardx_amd.cfit on the device (libguardx_cfit.so) against tests/cfit64.py: `gradient` under the three heads at the tile, row,
width, action-width and grid edges, without weights, under a 0 / 1 mask with whole tiles dead and under fractional weights,
held to 4 x the error of float32 autograd of the learners' own expression (torch on the CPU, same inputs); its exact
properties (dead rows may hold anything, W == 0, bit stability); `fit` against fit64 under weights that change every round,
held to 4 x the error of the learners' float32 loop; the Softplus pair against the rollout kernels' and a float64 sigmoid; and
the module after a fit in the hands of the rollouts.

The gradient's errors (cfit64.grad_errors): the relative L2 of the whole vector and of each of W1, b1, W2, b2, W3, b3, and the
relative error of the loss, each pooled over four seeds (root-mean-square).  The whole vector and the loss are held to their
own yardsticks (the loss's floored at half a float32 ulp: a float32 loss is closer to its float64 value only by luck); a block
to the largest of the six blocks' yardsticks, as tests/test_gpu_vfit.py holds its blocks.

As these tests print on an MI355X (x the yardstick, ALLOWED = 4; the worst over the grids workgroups = 1, 3, tiles + 3, 0 and
over the cases of each line):
    gradient                                            g              worst block        loss
    softplus D = 45, mask, B = 1 .. 4099                0.92 .. 1.49   0.85 .. 0.98 W1    1.00
    dot D = 43 A = 2, fractional, B = 1 .. 4099         0.24 .. 1.13   0.24 .. 0.99 W1    0.51 .. 1.00
    softplus, none, B = 130, the sixteen widths         0.62 .. 1.15   0.80 .. 0.86       0.59 .. 1.00
    dot A = 2, mask, B = 130, the sixteen widths        0.78 .. 0.98   0.88 .. 1.02 W1    0.57 .. 1.00
    dot D = 43, fractional, B = 130, A = 2, 8, 10, 16   0.77 .. 0.80   0.81 .. 0.84 W1    0.77 .. 1.00
    identity D = 45, B = 257, 3 regimes x 3 weightings  0.60 .. 0.78   0.79 .. 1.02       0.78 .. 1.00
    softplus D = 45, B = 257, the same nine             0.55 .. 1.03   0.72 .. 0.87 W1    0.77 .. 1.28
    dot D = 43 A = 2, B = 257, the same nine            0.59 .. 0.81   0.64 .. 1.21       0.67 .. 1.00   (1.21: b3, z20 under the mask)
    softplus D = 45, mask, B = 16385, default grid      0.28           0.63 W1            1.00
    fit, 10 iterations, displacement | loss trace       softplus 45, 257: 0.77 | 0.51   dot 43 (2), 130: 1.00 | 0.48   identity 64, 257: 0.99 | 0.68
    softplus_grad_f against a float64 sigmoid           1.943 ulp at x = -15.54; the formula in float32 on the CPU 2.394 ulp; bound 3.394
"""
import copy

import numpy as np
import pytest
import torch

import cfit64 as c64

pytestmark = pytest.mark.gpu

ALLOWED = c64.ALLOWED


def gradient_shapes():
    """(head, regime, weighting, D, A, B) of every gradient comparison below; tests/test_cfit64.py checks the yardsticks of
    each"""
    out = []
    for B in c64.GRAD_ROWS:
        out += [("softplus", "default", "mask", c64.SOFT_D, 1, B), ("dot", "default", "fractional", c64.DOT_D, 2, B)]
    for D in c64.EDGE_WIDTHS:
        out += [("softplus", "default", "none", D, 1, c64.EDGE_ROWS), ("dot", "default", "mask", D, 2, c64.EDGE_ROWS)]
    for A in c64.DOT_AS:
        out.append(("dot", "default", "fractional", c64.DOT_D, A, c64.EDGE_ROWS))
    for head in c64.HEADS:
        for regime in c64.REGIMES:
            for weighting in c64.WEIGHTINGS:
                out.append((head, regime, weighting, c64.DOT_D if head == "dot" else c64.SOFT_D, 2 if head == "dot" else 1, 257))
    out.append(("softplus", "default", "mask", c64.SOFT_D, 1, 16385))
    return out


def fitter(mod, **kw):
    """a CostCriticFit around a copy of `mod` on the device (the case's own module is shared and never written to)"""
    from guardx_amd import cfit
    kw.setdefault("lr", c64.LR)
    return cfit.CostCriticFit(copy.deepcopy(mod).cuda(), **kw)


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int64).reshape(-1).tolist()


def dev(t):
    if t is None:
        return None
    return (torch.from_numpy(t) if isinstance(t, np.ndarray) else t).cuda().contiguous()


def call_gradient(QF, c, w="case"):
    w = c["w"] if isinstance(w, str) else w
    return QF.gradient(dev(c["x"]), dev(c["y"]), weight=dev(w), act=dev(c["act"]), offset=dev(c["offset"]))


def check_gradient(head, regime, weighting, D, A, B, grids):
    cases = [c64.gradient_case(head, regime, weighting, D, A, B, s) for s in c64.GRAD_SEEDS]
    yard, yard_blocks, yard_loss = c64.pool_grads([c["yard"] for c in cases])
    top = max(yard_blocks.values())
    for wg in grids:
        errs = []
        for c in cases:
            g, loss, W = call_gradient(fitter(c["mod"], workgroups=wg), c)
            assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (c64.param_count(D, A),)
            assert loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0
            assert W.is_cuda and W.dtype == torch.float64 and W.dim() == 0 and abs(float(W) - c["W"]) <= 1e-12 * c["W"]
            errs.append(c64.grad_errors(g.cpu().numpy(), float(loss), c["g"], c["loss"], D, A))
        whole, blocks, le = c64.pool_grads(errs)
        worst = max(blocks, key=blocks.get)
        print(f"{head} {regime} {weighting} D={D} A={A} B={B} workgroups={wg}: g {whole:.2e} / {yard:.2e} = {whole / yard:.2f}  worst block "
              f"{worst} {blocks[worst]:.2e} / {top:.2e} = {blocks[worst] / top:.2f}  loss {le:.2e} / {yard_loss:.2e} = {le / yard_loss:.2f}")
        assert whole <= ALLOWED * yard, wg
        for k in c64.BLOCKS:
            assert blocks[k] <= ALLOWED * top, (wg, k)
        assert le <= ALLOWED * yard_loss, wg


@pytest.mark.parametrize("B", c64.GRAD_ROWS)
@pytest.mark.parametrize("head,weighting,D,A", [("softplus", "mask", c64.SOFT_D, 1), ("dot", "fractional", c64.DOT_D, 2)])
def test_gradient_against_grad64(head, weighting, D, A, B):
    tiles = -(-B // 64)
    check_gradient(head, "default", weighting, D, A, B, (1, 3, tiles + 3, 0))


@pytest.mark.parametrize("D", c64.EDGE_WIDTHS)
@pytest.mark.parametrize("head,weighting,A", [("softplus", "none", 1), ("dot", "mask", 2)])
def test_every_first_layer_instantiation_at_its_edges(head, weighting, A, D):
    check_gradient(head, "default", weighting, D, A, c64.EDGE_ROWS, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("A", c64.DOT_AS)
def test_every_action_width_of_the_dot_head(A):
    check_gradient("dot", "default", "fractional", c64.DOT_D, A, c64.EDGE_ROWS, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("weighting", c64.WEIGHTINGS)
@pytest.mark.parametrize("regime", list(c64.REGIMES))
@pytest.mark.parametrize("head", c64.HEADS)
def test_every_head_regime_and_weighting(head, regime, weighting):
    check_gradient(head, regime, weighting, c64.DOT_D if head == "dot" else c64.SOFT_D, 2 if head == "dot" else 1, 257, (1, 3, 5 + 3, 0))


def test_a_workgroup_walks_a_second_tile_at_the_default_grid():
    """workgroups = 0 is 256 workgroups from 16384 rows on; at 16385 workgroup 0 walks a second tile, of one row"""
    from guardx_amd import _cfit_native
    assert _cfit_native.load().gxq_default_workgroups(16385) == 256 and -(-16385 // 64) == 257
    check_gradient("softplus", "default", "mask", c64.SOFT_D, 1, 16385, (0,))


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
SHAPES = [("softplus", c64.SOFT_D, 1, 257), ("dot", c64.DOT_D, 2, 257), ("identity", c64.SOFT_D, 1, 257)]


@pytest.mark.parametrize("head,D,A,B", SHAPES)
def test_masked_rows_may_hold_anything(head, D, A, B):
    """NaN and Inf in x, target, act and offset of the rows with weight 0: the same bits as zeros there"""
    c = c64.gradient_case(head, "default", "mask", D, A, B, 0)
    dead = torch.from_numpy(c["w"] == 0)
    assert dead.sum() > 64 and (~dead).sum() > 10

    def planted(value):
        d = {}
        for k in ("x", "y", "act", "offset"):
            if c[k] is not None:
                d[k] = c[k].clone()
                d[k][dead] = value
        return d
    for wg in (0, 2):
        got = {}
        for name, value in (("zeros", 0.0), ("nan", float("nan")), ("inf", float("inf")), ("-inf", float("-inf"))):
            p = planted(value)
            QF = fitter(c["mod"], workgroups=wg)
            got[name] = [bits(t) for t in QF.gradient(dev(p["x"]), dev(p["y"]), weight=dev(c["w"]), act=dev(p.get("act")), offset=dev(p.get("offset")))]
        plain = [bits(t) for t in call_gradient(fitter(c["mod"], workgroups=wg), c)]
        assert got["nan"] == got["zeros"] and got["inf"] == got["zeros"] and got["-inf"] == got["zeros"]
        assert plain[1:] == got["zeros"][1:] and plain[0] == got["zeros"][0]      # and the rows' own finite values are not factors either
        assert np.isfinite(np.array(got["zeros"][0], np.int32).view(np.float32)).all()


@pytest.mark.parametrize("head,D,A,B", SHAPES)
def test_no_live_row_is_nan_and_returns_normally(head, D, A, B):
    c = c64.gradient_case(head, "default", "none", D, A, B, 0)
    QF = fitter(c["mod"])
    g, loss, W = call_gradient(QF, c, np.zeros(B, np.float32))
    assert float(W) == 0.0 and torch.isnan(loss) and torch.isnan(g).all()
    w = np.ones((3, B), np.float32)
    w[1] = 0.0
    info = QF.fit(dev(c["x"]), dev(c["y"]), iters=3, weight=dev(w), act=dev(c["act"]), offset=dev(c["offset"]))
    torch.cuda.synchronize()
    assert info["weight"].tolist() == [float(B), 0.0, float(B)]
    assert torch.isfinite(info["loss"][0]) and torch.isnan(info["loss"][1:]).all()
    assert torch.isnan(info["theta"]).all() and torch.isnan(c64.flat(QF.critic)).all() and torch.isnan(QF.m).all() and QF.step == 3


@pytest.mark.parametrize("head,D,A,B", [("softplus", c64.SOFT_D, 1, 257), ("dot", 64, 8, 4099)])
def test_two_calls_give_the_same_bits(head, D, A, B):
    c = c64.gradient_case(head, "default", "fractional", D, A, B, 0)
    for wg in (0, 3):
        QF = fitter(c["mod"], workgroups=wg)
        first = [bits(t) for t in call_gradient(QF, c)]
        assert first == [bits(t) for t in call_gradient(QF, c)] == [bits(t) for t in call_gradient(fitter(c["mod"], workgroups=wg), c)]
        a, b = fitter(c["mod"], workgroups=wg), fitter(c["mod"], workgroups=wg)
        args = (dev(c["x"]), dev(c["y"]))
        kw = dict(iters=3, weight=dev(c["w"]), act=dev(c["act"]), offset=dev(c["offset"]))
        ia, ib = a.fit(*args, **kw), b.fit(*args, **kw)
        assert all(bits(ia[k]) == bits(ib[k]) for k in ("theta", "loss", "weight")) and bits(a.m) == bits(b.m) and bits(a.v) == bits(b.v)


@pytest.mark.parametrize("head,D,A,B", [("softplus", c64.SOFT_D, 1, 257), ("dot", c64.DOT_D, 2, 63)])
def test_idle_workgroups_add_exact_zeros(head, D, A, B):
    c = c64.gradient_case(head, "default", "mask", D, A, B, 0)
    tiles = -(-B // 64)
    want = [bits(t) for t in call_gradient(fitter(c["mod"], workgroups=tiles), c)]
    for extra in (1, 5, 300):
        assert [bits(t) for t in call_gradient(fitter(c["mod"], workgroups=tiles + extra), c)] == want, extra


@pytest.mark.parametrize("head,D,A,B", [("softplus", c64.SOFT_D, 1, 65), ("dot", c64.DOT_D, 2, 63), ("identity", 64, 1, 1)])
def test_rows_inside_a_larger_buffer(head, D, A, B):
    """every input inside a larger buffer whose other entries are NaN: neither the rows past B - 1 of the last tile nor the
    columns a row is padded with in LDS come from memory"""
    c = c64.gradient_case(head, "default", "fractional", D, A, B, 0)
    tight = {k: dev(c[k]) for k in ("x", "y", "w", "act", "offset") if c[k] is not None}
    pad, inside = 4096, {}
    for k, t in tight.items():
        parent = torch.full((2 * pad + t.numel(),), float('nan'), device="cuda")
        parent[pad:pad + t.numel()] = t.reshape(-1)
        inside[k] = parent[pad:pad + t.numel()].view(t.shape)
        assert inside[k].is_contiguous()
    run = lambda d, wg: fitter(c["mod"], workgroups=wg).gradient(d["x"], d["y"], weight=d["w"], act=d.get("act"), offset=d.get("offset"))   # noqa: E731
    for wg in (0, 2):
        plain, got = run(tight, wg), run(inside, wg)
        assert [bits(t) for t in got] == [bits(t) for t in plain] and np.isfinite(plain[0].cpu().numpy()).all()


def test_a_side_stream_gives_the_same_bits():
    c = c64.fit_case("dot", 43, 2, 130, 2)
    args = (dev(c["x"]), dev(c["y"]))
    kw = dict(iters=3, weight=dev(c["w"][:3]), act=dev(c["act"]), offset=dev(c["offset"]))
    want = fitter(c["mod"]).fit(*args, **kw)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = fitter(c["mod"]).fit(*args, **kw)
    side.synchronize()
    assert all(bits(got[k]) == bits(want[k]) for k in ("theta", "loss", "weight"))


# ---------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------
def _run(c, calls, wg):
    """(theta after the calls, the loss trace, the W trace, the CostCriticFit) of consecutive fit calls of `calls` iterations,
    each under its own rows of the case's weight table"""
    QF = fitter(c["mod"], workgroups=wg)
    losses, Ws, at = [], [], 0
    for n in calls:
        info = QF.fit(dev(c["x"]), dev(c["y"]), iters=n, weight=dev(c["w"][at:at + n]), act=dev(c["act"]), offset=dev(c["offset"]))
        at += n
        losses.append(info["loss"])
        Ws.append(info["weight"])
    return info["theta"].cpu().numpy(), torch.cat(losses).cpu().numpy(), torch.cat(Ws).cpu().numpy(), QF


@pytest.mark.parametrize("wg", [0, 2])
@pytest.mark.parametrize("head,D,A,B", c64.FIT_SHAPES)
def test_fit_against_fit64(head, D, A, B, wg):
    yard_theta, yard_loss = c64.fit_yardstick(head, D, A, B)
    errs = []
    for seed in c64.FIT_SEEDS:
        c = c64.fit_case(head, D, A, B, seed)
        theta, losses, Ws, QF = _run(c, (c64.FIT_ITERS,), wg)
        assert QF.step == c64.FIT_ITERS and Ws.tolist() == c["Ws"].tolist() and len(set(Ws.tolist())) > 1
        errs.append(c64.fit_errors(theta, losses, c))
        theta2, losses2, Ws2, QF2 = _run(c, (5, 5), wg)           # the moments and the step count carry over
        assert QF2.step == 10 and theta2.view(np.int32).tolist() == theta.view(np.int32).tolist()
        assert losses2.view(np.int32).tolist() == losses.view(np.int32).tolist() and Ws2.tolist() == Ws.tolist()
    et, el = c64.pooled([e[0] for e in errs]), c64.pooled([e[1] for e in errs])
    print(f"{head} D={D} A={A} B={B} workgroups={wg} {c64.FIT_ITERS} iterations: displacement {et:.2e} / {yard_theta:.2e} = {et / yard_theta:.2f}  "
          f"loss trace {el:.2e} / {yard_loss:.2e} = {el / yard_loss:.2f}")
    assert et <= ALLOWED * yard_theta and el <= ALLOWED * yard_loss


def test_zero_iterations_change_nothing():
    c = c64.fit_case("softplus", 45, 1, 257, 0)
    QF = fitter(c["mod"])
    QF.fit(dev(c["x"]), dev(c["y"]), iters=2, weight=dev(c["w"][:2]))
    before = (bits(c64.flat(QF.critic)), bits(QF.m), bits(QF.v), QF.step)
    info = QF.fit(dev(c["x"]), dev(c["y"]), iters=0, weight=dev(c["w"][:0]))
    assert tuple(info["loss"].shape) == (0,) and tuple(info["weight"].shape) == (0,) and int(info["step"]) == 2
    assert (bits(c64.flat(QF.critic)), bits(QF.m), bits(QF.v), QF.step) == before == (bits(info["theta"]),) + before[1:]


# ---------------------------------------------------------------------------------------------------------------------
# Softplus and its derivative
# ---------------------------------------------------------------------------------------------------------------------
def softplus_grid():
    near = lambda v: [np.nextafter(np.float32(v), np.float32(-1e9)), np.float32(v), np.nextafter(np.float32(v), np.float32(1e9))]   # noqa: E731
    x = np.concatenate([np.linspace(-30, 30, 6001).astype(np.float32), np.array(near(20) + near(-20) + [-104, 89, 0, -0.0, np.nan], np.float32)])
    return x


def cpu_formula_df(x):
    """gx_qcritic.h:softplus_grad_f's formula in float32 on the CPU: x > 20 ? 1 : e / (e + 1), e = exp(x)"""
    x = np.asarray(x, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):          # exp(89) = inf: inf / inf, selected away
        e = np.exp(x).astype(np.float32)
        return np.where(x > 20, np.float32(1), e / (e + np.float32(1))).astype(np.float32)


def test_the_softplus_pair():
    """f: the bits of statewise.softplus_probe, the rollout kernels' Softplus.  df: against a float64 sigmoid; the bound is the
    worst error of the same formula evaluated in float32 on the CPU over the same grid plus 1 ulp.  As this test prints on an
    MI355X: worst 1.943 ulp at x = -15.54; the CPU's 2.394 ulp; bound 3.394.  Between -103 and -87.3 exp_f flushes to zero where
    the sigmoid is a float32 denormal: df = 0 there, an absolute error below 2^-126; the grid keeps -104 of that range."""
    import math64 as m
    from guardx_amd import cfit, statewise
    x = softplus_grid()
    xd = torch.from_numpy(x).cuda()
    f, df = cfit.softplus_probe(xd)
    assert bits(f) == bits(statewise.softplus_probe(xd))
    assert torch.isnan(f[-1]) and torch.isnan(df[-1])
    fin = ~np.isnan(x)
    ref = 1.0 / (1.0 + np.exp(-x[fin].astype(np.float64)))
    cpu = m.ulp_err(cpu_formula_df(x[fin]), ref).max()
    got = m.ulp_err(df.cpu().numpy()[fin], ref)
    i = int(np.argmax(got))
    print(f"softplus_grad_f: worst {got[i]:.3f} ulp at x = {x[fin][i]!r}; the formula in float32 on the CPU {cpu:.3f} ulp; bound {cpu + 1:.3f}")
    assert got.max() <= cpu + 1.0
    deep = torch.linspace(-103, -87.5, 64, device="cuda")
    assert (cfit.softplus_probe(deep)[1].abs() < 2.0 ** -126).all()
    far = torch.tensor([20.0, 89.0], device="cuda")
    assert cfit.softplus_probe(far)[1].tolist() == [1.0, 1.0]


# ---------------------------------------------------------------------------------------------------------------------
# the module after a fit, in the rollouts' hands
# ---------------------------------------------------------------------------------------------------------------------
def test_the_module_holds_the_result_and_rollout_usl_runs_on_it():
    from guardx_amd import Engine, cfit
    from guardx_amd.rollout_buffer import usl_rollout_batch
    from test_gpu_statewise import _cfg, _engine, COSTLY, SEED
    from test_policy64 import make_ac
    E = _engine(_cfg("point", 16, seed=5, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac = make_ac(D, A, 64, seed=3)
    ccritic = c64.make_module("softplus", D + A, seed=4).cuda()
    p = Engine.pack_actor_critic(ac).cuda()
    out = E.rollout_usl(p, 2, q_critic=Engine.pack_q_critic(ccritic, device='cuda'), noise_seed=SEED)
    data = usl_rollout_batch(out)
    QF = cfit.CostCriticFit(ccritic, lr=1e-3)
    assert QF.head == "softplus" and QF.Din == D + A
    before = bits(c64.flat(ccritic))
    info = QF.fit(torch.cat((data['obs'], data['act_safe']), dim=1), data['targetc'], iters=4)
    assert all(t.is_cuda for t in info.values()) and int(info["step"]) == 4 and info["weight"].tolist() == [32.0] * 4
    qp = Engine.pack_q_critic(ccritic, device='cuda')
    assert bits(qp) == bits(info["theta"]) == bits(c64.flat(ccritic)) != before
    again = E.rollout_usl(p, 2, q_critic=qp, noise_seed=SEED)
    assert all(torch.isfinite(v).all() for v in again.values())
    E.close()


def test_the_safelayer_recipe_runs_as_the_document_writes_it():
    from guardx_amd import Engine, cfit
    from guardx_amd.rollout_buffer import safelayer_rollout_batch
    from test_gpu_statewise import _cfg, _engine, COSTLY, SEED
    from test_policy64 import make_ac
    E = _engine(_cfg("point", 64, seed=5, **COSTLY))
    E.reset()
    D, A = E.obs_flat_size, E.action_space.shape[0]
    ac = make_ac(D, A, 64, seed=3)
    ccritic = c64.make_module("dot", D, A, seed=6).cuda()
    p = Engine.pack_actor_critic(ac).cuda()
    out = E.rollout_safelayer(p, 6, g_net=Engine.pack_g_net(ccritic, device='cuda', act_dim=A), noise_seed=SEED)
    data = safelayer_rollout_batch(out)
    assert (data['cost'] > 0).any() and (data['cost'] == 0).any()           # the inputs: there is something to down-sample
    QF = cfit.CostCriticFit(ccritic, lr=1e-3)
    w = cfit.downsample_weights(data['cost'], 8)
    info = QF.fit(data['obs'], data['cost'], iters=8, weight=w, act=data['act_safe'], offset=data['prev_cost'])
    gp = Engine.pack_g_net(ccritic, device='cuda', act_dim=A)
    assert bits(gp) == bits(info["theta"]) and torch.isfinite(info["theta"]).all() and torch.isfinite(info["loss"]).all()
    n_pos, n_zero = int((data['cost'] > 0).sum()), int((data['cost'] == 0).sum())
    k = c64.downsample_count(n_pos, n_zero)
    assert info["weight"].tolist() == [float(n_pos + n_zero if k is None else n_pos + k)] * 8
    assert torch.isfinite(E.rollout_safelayer(p, 2, g_net=gp, noise_seed=SEED)['act_safe']).all()
    E.close()
