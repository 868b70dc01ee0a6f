"""guardx_amd.pifit on the device (libguardx_pifit.so) against tests/pifit64.py: `gradient` at the tile, row, width, action-width
and grid edges, in every regime and for the three losses, held to 4 x the error of the learners' own float32 backward (torch
autograd on the CPU, on the same inputs); `fit` against fit64 over 1, 2, 3 and 10 iterations and as 5 + 5, held to 4 x the error
of the learners' float32 loop (autograd + torch.optim.Adam on the CPU, in row order), with stops at iteration 0, mid-loop and
never; and the exact properties.

The inputs are decidable (tests/test_pifit64.py): no row's float64 ratio lies within a relative 1e-5 of 1 +- clip_ratio at any
compared iteration, and each target_kl sits 100 x the float32 loop's kl error or more from the oracle's kl on either side of
the decision.  So stop_iter, steps and cf are compared exactly.  Seeds that fail a condition, and seeds on which the float32
loop's own displacement error is an outlier (one entry of g next to Adam's eps), are kept out by name: pifit64.FIT_KEPT_OUT.

The gradient's errors (pgrad64.grad_errors): the relative L2 of the whole vector and of each of log_std, W1, b1, W2, b2, W3, b3,
pooled over the seeds pifit64.grad_seeds lists; the whole vector is held to its own yardstick, a block to the largest of the
seven blocks' yardsticks, as tests/test_gpu_pgrad.py holds its blocks.  loss and kl are held to float64 at pifit64.MEANS_TOL.
The fit's (pifit64.fit_errors): the relative L2 of the displacement theta_k - theta_0 and the largest errors of the first k
entries of the loss and kl traces, pooled over pifit64.fit_seeds.

As these tests print on an MI355X: see INTEGRATION.md, "Policy fit on the device path"."""
import copy

import numpy as np
import pytest
import torch

import pgrad64 as p64
import pifit64 as a64
import vfit64 as v64

pytestmark = pytest.mark.gpu

ALLOWED = a64.ALLOWED
KEYS = ("obs", "act", "adv", "logp")


def bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(torch.int32).reshape(-1).tolist()


def device_data(batch):
    return {k: torch.from_numpy(np.array(batch[k])).cuda() for k in KEYS}


def fitter(case, **kw):
    """a PolicyFit around a copy of the case's actor on the device (the case's own is shared and never written to)"""
    from guardx_amd import pifit
    kw.setdefault("lr", a64.LR)
    return pifit.PolicyFit(copy.deepcopy(case["pi"]).cuda(), **kw)


def check_gradient(regime, D, A, B, grids, clip_ratio=a64.CLIP, loss="ratio"):
    seeds = a64.grad_seeds(regime, D, A, B)
    cases = [a64.gradient_case(regime, D, A, B, s, clip_ratio, loss) for s in seeds]
    yard, yard_blocks = a64.grad_yardstick(regime, D, A, B, clip_ratio, loss)
    top = max(yard_blocks.values())
    P = p64.f64.param_count(D, A, 64)
    for wg in grids:
        errs = []
        for c in cases:
            g, info = fitter(c, workgroups=wg).gradient(device_data(c["batch"]), clip_ratio=clip_ratio, loss=loss)
            assert g.is_cuda and g.dtype == torch.float32 and tuple(g.shape) == (P,)
            assert all(info[k].is_cuda and info[k].dim() == 0 and info[k].dtype == torch.float64 for k in ("loss", "kl", "cf", "ent"))
            errs.append(p64.grad_errors(g.cpu().numpy(), c["g"], D, A))
            for k in ("loss", "kl"):
                assert abs(float(info[k]) - c["info"][k]) <= a64.MEANS_TOL * max(1.0, abs(c["info"][k])), (k, wg)
            assert float(info["cf"]) == c["info"]["cf"], wg
            assert abs(float(info["ent"]) - c["info"]["ent"]) <= 1e-14
        whole, blocks = p64.pool(errs)
        worst = max(blocks, key=blocks.get)
        print(f"{regime} D={D} A={A} B={B} clip={clip_ratio} loss={loss} seeds={seeds} workgroups={wg}: g {whole:.2e} / {yard:.2e} = "
              f"{whole / yard:.2f}  worst block {worst} {blocks[worst]:.2e} / {top:.2e} = {blocks[worst] / top:.2f}")
        assert whole <= ALLOWED * yard, wg
        for k in p64.BLOCKS:
            assert blocks[k] <= ALLOWED * top, (wg, k)


@pytest.mark.parametrize("B", a64.GRAD_ROWS)
@pytest.mark.parametrize("D", a64.GRAD_WIDTHS)
def test_gradient_against_grad64(D, B):
    tiles = -(-B // 64)
    check_gradient("default", D, 2, B, (1, 3, tiles + 3, 0))


def test_a_workgroup_walks_a_second_tile_at_the_default_grid():
    """workgroups = 0 is 256 workgroups from 16384 rows on; at 16385 workgroup 0 walks a second tile, of one row"""
    from guardx_amd import _pifit_native
    assert _pifit_native.load().gxa_default_workgroups(16385) == 256 and -(-16385 // 64) == 257
    check_gradient("default", 43, 2, 16385, (0,))


@pytest.mark.parametrize("D", p64.EDGE_WIDTHS)
def test_every_first_layer_instantiation_at_its_edges(D):
    check_gradient("default", D, 2, v64.EDGE_ROWS, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("A", (8, 10))
def test_action_widths(A):
    check_gradient("default", 43, A, 130, (1, 3, 3 + 3, 0))


@pytest.mark.parametrize("regime", ("trained", "saturated"))
def test_every_regime(regime):
    check_gradient(regime, 43, 2, 257, (1, 3, 5 + 3, 0))


@pytest.mark.parametrize("loss,clip_ratio", a64.LOSSES[1:])
@pytest.mark.parametrize("D,B", [(43, 257), (64, 65)])
def test_the_unclipped_and_the_logp_loss(D, B, loss, clip_ratio):
    tiles = -(-B // 64)
    check_gradient("default", D, 2, B, (1, 3, tiles + 3, 0), clip_ratio, loss)


# ---------------------------------------------------------------------------------------------------------------------
# the fit
# ---------------------------------------------------------------------------------------------------------------------
def run(c, calls, wg, data=None, **kw):
    """consecutive fit calls of `calls` iterations on one PolicyFit -> (dict(thetas: theta after each call, loss, kl, cf: the
    calls' traces one after the other, infos), the PolicyFit)"""
    PF = fitter(c, workgroups=wg)
    data = data or device_data(c["batch"])
    infos = [PF.fit(data, iters=n, **kw) for n in calls]
    out = {k: torch.cat([i[k] for i in infos]).cpu().numpy() for k in a64.TRACES}
    return dict(out, thetas=[i["theta"].cpu().numpy() for i in infos], infos=infos), PF


def state_bits(PF, info):
    return [bits(info["theta"]), bits(PF.m), bits(PF.v), int(PF.count[0])]


@pytest.mark.parametrize("wg", [0, 2])
@pytest.mark.parametrize("D,B", a64.FIT_SHAPES)
def test_fit_against_fit64(D, B, wg):
    yard = a64.fit_yardstick(D, B)
    errs, split = [], []
    for seed in a64.fit_seeds(D, B):
        c = a64.fit_case(D, B, seed)
        ref, got = c["ref"], dict(thetas={0: c["theta"]})
        for k in a64.FIT_KS:
            r, PF = run(c, (k,), wg)
            i = r["infos"][0]
            assert (int(i["stop_iter"]), int(i["steps"]), int(i["step"]), int(PF.count[0])) == (k - 1, k, k, k)
            assert r["cf"].tolist() == ref["cf"][:k].tolist()                     # decidable: exactly
            got["thetas"][k] = r["thetas"][0]
            got.update(loss=r["loss"], kl=r["kl"])
        errs.append(a64.fit_errors(got, ref, c["scale"]))
        r, PF = run(c, (5, 5), wg)                                # the moments and the device's step count carry over
        assert int(PF.count[0]) == 10 and [int(i["step"]) for i in r["infos"]] == [5, 10]
        assert r["thetas"][1].view(np.int32).tolist() == got["thetas"][10].view(np.int32).tolist()
        for k in a64.TRACES[:2]:
            assert r[k].view(np.int64).tolist() == got[k].view(np.int64).tolist(), k
        assert r["cf"].tolist() == ref["cf"][:10].tolist()
    err = a64.pool_fits(errs)
    for k in a64.FIT_KS:
        print(f"D={D} B={B} workgroups={wg} k={k}: " + "  ".join(
            f"{what} {err[what, k]:.2e} / {yard[what, k]:.2e} = {err[what, k] / yard[what, k]:.2f}" for what in ("theta", "loss", "kl")))
    for k in a64.FIT_KS:
        for what in ("theta", "loss", "kl"):
            assert err[what, k] <= ALLOWED * yard[what, k], (what, k)


@pytest.mark.parametrize("where", [0, a64.MID, None])
@pytest.mark.parametrize("D,B", a64.FIT_SHAPES)
def test_the_stop_is_the_learners(D, B, where):
    """target_kl between the oracle's kl entries: the call stops where fit64 stops, leaves theta, m, v and the count bit-equal
    to those of an unstopped call of that many iterations, and writes nothing past the stop"""
    n = max(a64.FIT_KS)
    for seed in a64.fit_seeds(D, B):
        c = a64.fit_case(D, B, seed)
        want = a64.fit64(c["theta"], c["batch"], n, c["targets"][where])
        assert want["stop_iter"] == (n - 1 if where is None else where) and want["steps"] == (n if where is None else where)
        for wg in (0, 2):
            r, PF = run(c, (n,), wg, target_kl=c["targets"][where])
            i = r["infos"][0]
            assert (int(i["stop_iter"]), int(i["steps"]), int(i["step"])) == (want["stop_iter"], want["steps"], want["steps"])
            assert i["stop_iter"].dtype == i["steps"].dtype == torch.int32 and i["step"].dtype == torch.int64
            evaluated = want["steps"] + (where is not None)
            for k in a64.TRACES:
                assert np.isnan(r[k][evaluated:]).all() and np.isfinite(r[k][:evaluated]).all(), k
            assert r["cf"][:evaluated].tolist() == want["cf"][:evaluated].tolist()
            plain, PG = run(c, (want["steps"],), wg)              # no target: the same iterations, nothing stops
            assert state_bits(PF, i) == state_bits(PG, plain["infos"][0])
            for k in a64.TRACES:
                assert r[k][:want["steps"]].view(np.int64).tolist() == plain[k].view(np.int64).tolist(), k
            last = evaluated - 1
            assert [float(i[k + "_last"]) for k in a64.TRACES] == [float(r[k][last]) for k in a64.TRACES]
            assert abs(float(i["ent"]) - want["ent"]) <= 1e-14
            assert bits(torch.cat([p.detach().reshape(-1) for p in PF.pi.parameters()])) == bits(i["theta"])
            if where == a64.MID and wg == 0:
                # the optimizer goes on from the stop: two more iterations equal an unstopped call of MID + 2
                more = PF.fit(device_data(c["batch"]), iters=2)
                whole, PW = run(c, (a64.MID + 2,), wg)
                assert state_bits(PF, more) == state_bits(PW, whole["infos"][0]) and int(more["step"]) == a64.MID + 2


def test_the_unclipped_loss_stops_on_kl_and_the_logp_loss_takes_one_step():
    """espo: clip_ratio=None with its delta as target_kl; a2c: loss='logp', iters=1"""
    D, B = a64.FIT_SHAPES[0]
    seed = a64.fit_seeds(D, B)[0]
    c = a64.fit_case(D, B, seed)
    data = device_data(c["batch"])
    ref = a64.fit64(c["theta"], c["batch"], 6, None, None, "ratio")
    tkl = 0.5 * (max(ref["kl"][:2]) + ref["kl"][2])
    assert (ref["kl"][2] - tkl) > 1e-4 and (tkl - max(ref["kl"][:2])) > 1e-4     # float32's kl error is some 1e-7
    want = a64.fit64(c["theta"], c["batch"], 6, tkl, None, "ratio")
    info = fitter(c).fit(data, iters=6, target_kl=tkl, clip_ratio=None)
    assert (int(info["stop_iter"]), int(info["steps"])) == (want["stop_iter"], want["steps"]) == (2, 2)
    assert info["cf"].cpu().numpy()[:3].tolist() == [0.0, 0.0, 0.0]
    disp = p64.f64.rel_l2(info["theta"].cpu().numpy().astype(np.float64) - c["theta"], want["theta"] - c["theta"])
    print(f"espo: displacement after two steps {disp:.2e}")
    assert disp <= 1e-3
    want = a64.fit64(c["theta"], c["batch"], 1, None, None, "logp")
    info = fitter(c).fit(data, iters=1, target_kl=None, clip_ratio=None, loss="logp")
    disp = p64.f64.rel_l2(info["theta"].cpu().numpy().astype(np.float64) - c["theta"], want["theta"] - c["theta"])
    print(f"a2c: displacement after one step {disp:.2e}; loss {float(info['loss'][0])!r} against {want['loss'][0]!r}")
    assert disp <= 1e-3 and int(info["steps"]) == 1 and abs(float(info["loss"][0]) - want["loss"][0]) <= a64.MEANS_TOL * max(1.0, abs(want["loss"][0]))


# ---------------------------------------------------------------------------------------------------------------------
# exact properties
# ---------------------------------------------------------------------------------------------------------------------
def pair(out):
    g, info = out
    return [bits(g)] + [bits(info[k].reshape(1).view(torch.int32)) for k in ("loss", "kl", "cf", "ent")]


def fit_bits(info, PF):
    return state_bits(PF, info) + [bits(info[k].view(torch.int32)) for k in a64.TRACES] + [int(info["stop_iter"]), int(info["steps"])]


@pytest.mark.parametrize("D,B", [(43, 257), (64, 130)])
def test_two_calls_give_the_same_bits(D, B):
    c = a64.fit_case(D, B, a64.fit_seeds(D, B)[0])
    data = device_data(c["batch"])
    for wg in (0, 3):
        PF = fitter(c, workgroups=wg)
        first = pair(PF.gradient(data))
        assert first == pair(PF.gradient(data)) == pair(fitter(c, workgroups=wg).gradient(data))
        x, y = fitter(c, workgroups=wg), fitter(c, workgroups=wg)
        tkl = c["targets"][a64.MID]
        assert fit_bits(x.fit(data, iters=6, target_kl=tkl), x) == fit_bits(y.fit(data, iters=6, target_kl=tkl), y)


@pytest.mark.parametrize("D,B", [(43, 257), (64, 63)])
def test_idle_workgroups_add_exact_zeros(D, B):
    c = a64.gradient_case("default", D, 2, B, 0)
    data = device_data(c["batch"])
    tiles = -(-B // 64)
    want = pair(fitter(c, workgroups=tiles).gradient(data))
    PW = fitter(c, workgroups=tiles)
    want_fit = fit_bits(PW.fit(data, iters=3), PW)
    for extra in (1, 5, 300):
        assert pair(fitter(c, workgroups=tiles + extra).gradient(data)) == want, extra
        PF = fitter(c, workgroups=tiles + extra)
        assert fit_bits(PF.fit(data, iters=3), PF) == want_fit, extra


@pytest.mark.parametrize("D,B", [(43, 65), (64, 63), (43, 1)])
def test_rows_inside_a_larger_buffer(D, B):
    """every tensor of the batch inside a larger buffer whose other entries are NaN: neither the rows past B - 1 of the last
    tile nor the columns a row is padded with in LDS come from memory"""
    c = a64.gradient_case("default", D, 2, B, 0)
    tight = device_data(c["batch"])
    pad, inside = 4096, {}
    for k, t in tight.items():
        parent = torch.full((2 * pad + t.numel(),), float('nan'), device="cuda")
        parent[pad:pad + t.numel()] = t.reshape(-1)
        inside[k] = parent[pad:pad + t.numel()].view(t.shape)
        assert inside[k].is_contiguous()
    for wg in (0, 2):
        plain = fitter(c, workgroups=wg).gradient(tight)
        assert pair(fitter(c, workgroups=wg).gradient(inside)) == pair(plain) and np.isfinite(plain[0].cpu().numpy()).all()
        x, y = fitter(c, workgroups=wg), fitter(c, workgroups=wg)
        ix = x.fit(tight, iters=2)
        assert fit_bits(ix, x) == fit_bits(y.fit(inside, iters=2), y) and np.isfinite(ix["theta"].cpu().numpy()).all()


def test_tanh_act_over_its_domain():
    """the set, the checks and the bound (2.3 ulp, the figure gx_pifit.hip states) of tests/math64.py, as tests/test_gpu_vfit.py"""
    import math64 as m
    from guardx_amd import _pifit_native as n
    x = m.tanh_act_set()
    xd = torch.from_numpy(np.array(x)).cuda()
    yd = torch.full_like(xd, float('nan'))
    n.check(n.load().gxa_tanh_act(x.size, xd.data_ptr(), yd.data_ptr(), None))
    torch.cuda.synchronize()
    m.check_tanh_act(x, yd.cpu().numpy(), "HIP pifit")
    assert n.load().gxa_tanh_act(0, xd.data_ptr(), yd.data_ptr(), None) == n.GXA_OK


def test_the_module_holds_the_flat_result_and_the_first_entries_are_the_gradients():
    from guardx_amd import fisher
    c = a64.fit_case(43, 257, 0)
    data = device_data(c["batch"])
    PF = fitter(c)
    assert bits(fisher.flat_params(PF.pi)) == bits(torch.from_numpy(c["theta"]))
    _, g0 = PF.gradient(data)
    info = PF.fit(data, iters=4)
    assert all(t.is_cuda for t in info.values()) and all(info[k].dtype == torch.float64 and tuple(info[k].shape) == (4,) for k in a64.TRACES)
    assert bits(fisher.flat_params(PF.pi)) == bits(info["theta"]) != bits(torch.from_numpy(c["theta"]))
    assert all(p.is_cuda for p in PF.pi.parameters())
    for k in a64.TRACES:
        assert float(info[k][0]) == float(g0[k]), k
    assert float(info["ent"]) == float(g0["ent"])
    _, g4 = PF.gradient(data)                                     # taken at the fitted parameters: what a fifth iteration reports
    again = PF.fit(data, iters=1)
    assert float(again["loss"][0]) == float(g4["loss"]) and int(again["step"]) == 5
    assert float(info["loss"][0]) > float(info["loss"][3]) > float(g4["loss"])      # it descends


def test_zero_iterations_change_nothing():
    from guardx_amd import fisher
    c = a64.fit_case(64, 130, 0)
    data = device_data(c["batch"])
    PF = fitter(c)
    first = PF.fit(data, iters=2)
    before = state_bits(PF, first) + [bits(fisher.flat_params(PF.pi))]
    info = PF.fit(data, iters=0)
    assert tuple(info["loss"].shape) == (0,) and (int(info["step"]), int(info["steps"]), int(info["stop_iter"])) == (2, 0, -1)
    assert state_bits(PF, info) + [bits(fisher.flat_params(PF.pi))] == before
    ent = float((info["theta"][:2].cpu().numpy().astype(np.float64) + 0.5 + p64.HALF_LOG_2PI).sum())
    assert abs(float(info["ent"]) - ent) <= 1e-14 and np.isnan(float(info["loss_last"]))


def test_a_call_queued_behind_other_work_equals_the_synchronised_one():
    c = a64.fit_case(43, 257, 0)
    data = device_data(c["batch"])
    tkl = c["targets"][a64.MID]
    PW = fitter(c)
    want = fit_bits(PW.fit(data, iters=6, target_kl=tkl), PW)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    big = torch.randn(4096, 4096, device="cuda")
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(8):
            big = big @ big * 1e-3                                # the stream is busy when the fit's launches are queued
        PF = fitter(c)
        info = PF.fit(data, iters=6, target_kl=tkl)
        info2 = PF.fit(data, iters=2)                             # and a second call behind the first, unsynchronised
    side.synchronize()
    PS = fitter(c)
    PS.fit(data, iters=6, target_kl=tkl)
    torch.cuda.synchronize()
    want2 = fit_bits(PS.fit(data, iters=2), PS)
    assert [bits(info[k].view(torch.int32)) for k in a64.TRACES] == want[4:7] and int(info["stop_iter"]) == want[7]
    assert fit_bits(info2, PF) == want2
