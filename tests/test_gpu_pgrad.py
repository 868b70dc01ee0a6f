"""guardx_amd.pgrad on the device (libguardx_pgrad.so) against tests/pgrad64.py: `gradient` (g and b) at the tile, row, width,
action-width and grid edges, held to 4 x the error of the learners' own float32 backward (torch autograd on the CPU, on the
same inputs); its exact properties; its means against the line search's; gxg_cpo_direction against cpo_direction64 in the
seven situations of tests/test_pgrad64.py; and one chained update, gradient -> cpo_direction -> LineSearch.search ->
assign_flat_params.

The gradient's errors (pgrad64.grad_errors): the relative L2 of the whole vector and of each of log_std, W1, b1, W2, b2, W3,
b3, pooled (root-mean-square) over the seeds pgrad64.kept_seeds lists (tests/test_pgrad64.py: well conditioned, at least three of four).  adv is
standardised and adc centred, as the buffer leaves them.  The whole vector is held to its own yardstick; a block to the
largest of the seven blocks' yardsticks, as tests/test_gpu_vfit.py holds its blocks (log_std and b3 are A numbers each).

As these tests print on an MI355X (x the yardstick, ALLOWED = 4; the worst of the grids workgroups = 1, 3, tiles + 3, 0): see
INTEGRATION.md, "Surrogate gradients and the CPO step on the device path"."""
import copy

import numpy as np
import pytest
import torch

import pgrad64 as p64
import vfit64 as v64

pytestmark = pytest.mark.gpu

ALLOWED = p64.ALLOWED


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).reshape(-1).tolist()


def device_data(batch, adc=True, keys=("obs", "act", "adv", "logp", "mu", "logstd")):
    d = {k: torch.from_numpy(np.array(batch[k])).cuda() for k in keys}
    if adc:
        d["adc"] = torch.from_numpy(np.array(batch["adc"])).cuda()
    return d


def surrogate(case, adc=True, **kw):
    """a SurrogateGradient around a copy of the case's actor on the device (the case's own is shared and never written to)"""
    from guardx_amd import pgrad
    return pgrad.SurrogateGradient(copy.deepcopy(case["pi"]).cuda(), device_data(case["batch"], adc), **kw)


def check_gradient(regime, D, A, B, grids):
    seeds = p64.kept_seeds(regime, D, A, B)
    cases = [p64.gradient_case(regime, D, A, B, s) for s in seeds]
    yards = p64.yardstick(regime, D, A, B)
    P = p64.f64.param_count(D, A, 64)
    for wg in grids:
        errs = ([], [])
        for c in cases:
            g, b, info = surrogate(c, workgroups=wg).gradient()
            for v in (g, b):
                assert v.is_cuda and v.dtype == torch.float32 and tuple(v.shape) == (P,)
            assert all(info[k].is_cuda and info[k].dim() == 0 for k in ("pi_l", "surr_cost", "approx_kl", "ent"))
            errs[0].append(p64.grad_errors(g.cpu().numpy(), c["g"], D, A))
            errs[1].append(p64.grad_errors(b.cpu().numpy(), c["b"], D, A))
            for k in ("pi_l", "surr_cost", "approx_kl", "ent"):
                assert abs(float(info[k]) - c["means"][k]) <= 1e-5 * max(1.0, abs(c["means"][k])), (k, wg)
        for name, e, (yard, yard_blocks) in zip("gb", errs, yards):
            whole, blocks = p64.pool(e)
            top = max(yard_blocks.values())
            worst = max(blocks, key=blocks.get)
            print(f"{regime} D={D} A={A} B={B} seeds={seeds} workgroups={wg}: {name} {whole:.2e} / {yard:.2e} = {whole / yard:.2f}  "
                  f"worst block {worst} {blocks[worst]:.2e} / {top:.2e} = {blocks[worst] / top:.2f}")
            assert whole <= ALLOWED * yard, (name, wg)
            for k in p64.BLOCKS:
                assert blocks[k] <= ALLOWED * top, (name, wg, k)


@pytest.mark.parametrize("B", p64.ROWS)
@pytest.mark.parametrize("D", (43, 64))
def test_gradient_against_grad64(D, B):
    tiles = -(-B // 64)
    check_gradient("default", D, 2, B, (1, 3, tiles + 3, 0))


@pytest.mark.parametrize("A", (8, 10))
def test_action_widths_around_half_the_padded_tile(A):
    """A = 8: both dmu together are the 16 padded action columns; A = 10: they are more"""
    check_gradient("default", 43, A, 130, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("D", p64.EDGE_WIDTHS)
def test_every_first_layer_instantiation_at_its_edges(D):
    """D at both ends of every instantiation's range (1 .. 16, .. 32, .. 44, .. 48, .. 64, .. 72, .. 96, .. 128); from D = 73 on
    the second gradient is a second pass"""
    check_gradient("default", D, 2, v64.EDGE_ROWS, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("regime", ("trained", "saturated"))
def test_every_regime(regime):
    check_gradient(regime, 43, 2, 257, (1, 3, 5 + 3, 0))


def test_a_workgroup_walks_a_second_tile_at_the_default_grid():
    """workgroups = 0 is 256 workgroups from 16384 rows on; at 16385 workgroup 0 walks a second tile, of one row"""
    from guardx_amd import _pgrad_native
    assert _pgrad_native.load().gxg_default_workgroups(16385) == 256 and -(-16385 // 64) == 257
    check_gradient("default", 43, 2, 16385, (0,))


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
def triple(out):
    g, b, info = out
    return [bits(g), bits(b) if b is not None else None] + [bits(info[k].reshape(1).view(torch.int32)) for k in ("pi_l", "surr_cost", "approx_kl", "ent")]


@pytest.mark.parametrize("D,A,B", [(43, 2, 257), (64, 8, 4099), (96, 2, 130)])
def test_g_is_the_same_with_and_without_adc(D, A, B):
    c = p64.gradient_case("default", D, A, B, 0)
    for wg in (0, 3):
        g2, b2, i2 = surrogate(c, workgroups=wg).gradient()
        g1, b1, i1 = surrogate(c, adc=False, workgroups=wg).gradient()
        assert b1 is None and b2 is not None and bits(g1) == bits(g2)
        assert float(i1["pi_l"]) == float(i2["pi_l"]) and float(i1["approx_kl"]) == float(i2["approx_kl"]) and float(i1["surr_cost"]) == 0.0
        assert np.isfinite(g1.cpu().numpy()).all() and np.isfinite(b2.cpu().numpy()).all()


@pytest.mark.parametrize("D,A,B", [(43, 2, 257), (64, 2, 4099), (128, 4, 130)])
def test_two_calls_give_the_same_bits(D, A, B):
    c = p64.gradient_case("default", D, A, B, 0)
    for wg in (0, 3):
        S = surrogate(c, workgroups=wg)
        first = triple(S.gradient())
        assert first == triple(S.gradient()) == triple(surrogate(c, workgroups=wg).gradient())


@pytest.mark.parametrize("D,B", [(43, 257), (64, 63), (97, 65)])
def test_idle_workgroups_add_exact_zeros(D, B):
    c = p64.gradient_case("default", D, 2, B, 0)
    tiles = -(-B // 64)
    want = triple(surrogate(c, workgroups=tiles).gradient())
    for extra in (1, 5, 300):
        assert triple(surrogate(c, workgroups=tiles + extra).gradient()) == want, extra


@pytest.mark.parametrize("D,B", [(43, 65), (64, 63), (43, 1), (100, 65)])
def test_rows_inside_a_larger_buffer(D, B):
    """every tensor of the batch inside a larger buffer whose other entries are NaN: neither the rows past B - 1 of the last
    tile nor the columns a row is padded with in LDS come from memory"""
    from guardx_amd import pgrad
    c = p64.gradient_case("default", D, 2, B, 0)
    tight = device_data(c["batch"], keys=("obs", "act", "adv", "logp"))
    pad, inside = 4096, {}
    for k, t in tight.items():
        parent = torch.full((2 * pad + t.numel(),), float('nan'), device="cuda")
        parent[pad:pad + t.numel()] = t.reshape(-1)
        inside[k] = parent[pad:pad + t.numel()].view(t.shape)
        assert inside[k].is_contiguous()
    pi = copy.deepcopy(c["pi"]).cuda()
    for wg in (0, 2):
        plain = pgrad.SurrogateGradient(pi, tight, workgroups=wg).gradient()
        got = pgrad.SurrogateGradient(pi, inside, workgroups=wg).gradient()
        assert triple(got) == triple(plain) and np.isfinite(plain[0].cpu().numpy()).all() and np.isfinite(plain[1].cpu().numpy()).all()


def test_a_side_stream_gives_the_same_bits():
    c = p64.gradient_case("default", 43, 2, 4099, 0)
    S = surrogate(c)
    want = triple(S.gradient())
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = S.gradient()
    side.synchronize()
    assert triple(got) == want


@pytest.mark.parametrize("D,A,B", [(43, 2, 257), (64, 8, 4099)])
def test_the_means_are_the_line_searchs(D, A, B):
    """pi_l, surr_cost and approx_kl against LineSearch.evaluate(d, [0.0])'s row: the same rows' terms in the same words, so they
    agree to the float32 rounding the search applies to its means"""
    from guardx_amd import linesearch
    c = p64.gradient_case("default", D, A, B, 1)
    pi, data = copy.deepcopy(c["pi"]).cuda(), device_data(c["batch"])
    from guardx_amd import pgrad
    _, _, info = pgrad.SurrogateGradient(pi, data).gradient()
    row = linesearch.LineSearch(pi, data).evaluate(torch.zeros(p64.f64.param_count(D, A, 64), device="cuda"), [0.0])[0].cpu().numpy()
    for k, i in (("pi_l", 1), ("surr_cost", 2), ("approx_kl", 3)):
        mine = float(info[k])
        print(f"D={D} A={A} B={B} {k}: {mine!r} against the line search's {row[i]!r}")
        assert np.float32(mine) == np.float32(row[i]), k
    ls = c["theta"][:A].astype(np.float64)
    assert abs(float(info["ent"]) - float((ls + 0.5 + p64.HALF_LOG_2PI).sum())) <= 1e-14


# ---------------------------------------------------------------------------------------------------------------------
# the directions
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", p64.SITUATIONS)
def test_cpo_direction_against_cpo_direction64(name):
    from guardx_amd import pgrad
    i = p64.direction_inputs(name)
    want = p64.cpo_direction64(**i)
    dev = lambda k: torch.from_numpy(np.array(i[k])).cuda()      # noqa: E731
    for as_tensor in (False, True):
        c, tkl = (torch.tensor(i["c"], dtype=torch.float64, device="cuda"), torch.tensor(i["target_kl"], dtype=torch.float64, device="cuda")) if as_tensor else (i["c"], i["target_kl"])
        x, info = pgrad._direction_from(dev("b"), dev("Hinv_g"), dev("Hinv_b"), dev("approx_g"), torch.tensor([i["s"]], dtype=torch.float32, device="cuda"), c, tkl)
        assert int(info["optim_case"]) == want["optim_case"] and bool(info["need_loss"]) == (want["optim_case"] > 1)
        assert info["optim_case"].dtype == torch.int32 and info["lam"].dtype == torch.float64 and x.dtype == torch.float32
        for k in ("lam", "nu", "q", "r", "s", "A", "B"):
            got = float(info[k])
            print(f"{name} {k}: {got!r} against {want[k]!r}")
            assert abs(got - want[k]) <= 1e-6 * abs(want[k]), k
        xs = x.cpu().numpy().astype(np.float64)
        assert np.isfinite(xs).all()
        assert np.linalg.norm(xs - want["x"]) <= 1e-6 * np.linalg.norm(want["x"])


def test_a_zero_b_below_the_limit_is_case_4_and_finite():
    """through the public call, both solves included: b = 0 and c < 0"""
    from guardx_amd import fisher, pgrad
    c = p64.gradient_case("default", 43, 2, 257, 0)
    pi, data = copy.deepcopy(c["pi"]).cuda(), device_data(c["batch"])
    g, _, _ = pgrad.SurrogateGradient(pi, data).gradient()
    F = fisher.FisherOperator(pi, data["obs"])
    x, info = pgrad.cpo_direction(F, g, torch.zeros_like(g), -0.5, 0.01, cg_iters=10)
    assert int(info["optim_case"]) == 4 and float(info["nu"]) == 0.0 and float(info["r"]) == 0.0 and bool(info["need_loss"])
    xs = x.cpu().numpy()
    assert np.isfinite(xs).all() and np.linalg.norm(xs) > 0.0
    # ... and is trpo's direction: lam = sqrt(q / (2 target_kl)) against sqrt(2 target_kl / s), with q = s up to the solve's residual
    xt, it = pgrad.trpo_direction(F, g, 0.01, cg_iters=10)
    x_hat, s, _ = F.solve(g, iters=10)
    want = np.sqrt(2.0 * 0.01 / (float(s) + 1e-8)) * x_hat.cpu().numpy().astype(np.float64)
    assert np.linalg.norm(xt.cpu().numpy() - want) <= 1e-6 * np.linalg.norm(want) and float(it["s"]) == float(s)
    assert np.linalg.norm(xs - want) <= 1e-2 * np.linalg.norm(want)


def test_one_update_from_gradient_to_assigned_parameters():
    """gradient -> cpo_direction -> LineSearch.search -> assign_flat_params: the plumbing, not the accuracy"""
    from guardx_amd import fisher, linesearch, pgrad
    D, A, B = 43, 2, 257
    c = p64.gradient_case("default", D, A, B, 0)
    pi, data = copy.deepcopy(c["pi"]).cuda(), device_data(c["batch"])
    target_kl = 0.01
    g, b, ginfo = pgrad.SurrogateGradient(pi, data).gradient()
    F = fisher.FisherOperator(pi, data["obs"], damping=0.1)
    cost = torch.tensor(-0.01, dtype=torch.float64, device="cuda")          # c as the device path has it: a 0-dim tensor
    x, dinfo = pgrad.cpo_direction(F, g, b, cost, target_kl, cg_iters=20)
    margin = torch.clamp(-cost, min=0.0)
    theta_new, sinfo = linesearch.LineSearch(pi, data).search(x, target_kl, cost_margin=margin, need_loss=dinfo["need_loss"])
    linesearch.assign_flat_params(pi, theta_new)
    torch.cuda.synchronize()
    flat = fisher.flat_params(pi).cpu().numpy()
    assert np.isfinite(flat).all() and bits(fisher.flat_params(pi)) == bits(theta_new)
    assert int(dinfo["optim_case"]) in (0, 1, 2, 3, 4) and np.isfinite(x.cpu().numpy()).all()
    accepted = int(sinfo["accepted"])
    print(f"optim_case {int(dinfo['optim_case'])} lam {float(dinfo['lam']):.4g} nu {float(dinfo['nu']):.4g} accepted {accepted} "
          f"kl {float(sinfo['kl']):.3e} pi_l {float(sinfo['pi_l']):.4e} (old {float(ginfo['pi_l']):.4e})")
    assert accepted >= 0 and np.float32(float(sinfo["kl"])) <= target_kl
    assert not np.array_equal(flat, c["theta"])
    assert np.float32(float(sinfo["pi_l_old"])) == np.float32(float(ginfo["pi_l"]))
