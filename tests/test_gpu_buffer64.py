"""The kernels that turn a rollout into the learner's batch against the float64 restatement tests/buffer64.py, at the
block and stride edges of their launches: finish_gae_kernel / finish_gather_kernel (gx_episode.hip) through
episode_rollout_batch, and the kernels of gx_gae.hip through the entry points guardx_amd/rollout_buffer.py itself uses.
Synthetic tensors only: no Engine, no robot, no networks.  The same inputs go through the host paths in
tests/test_buffer64.py."""
import ctypes as C

import numpy as np
import pytest

import buffer64 as b64
from buffer64 import FORMS, PARTITION_N

pytestmark = pytest.mark.gpu
GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (who, output), (r, case) in sorted(b64.RATIOS.items()):
        print(f"\nlargest error/bound {who:28s} {output:9s} {r:8.3f}  {case}", end="")


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32 if x.dtype == np.float32 else x.dtype)


def _episode(g, case, out_dev=None, out_host=None):
    """the four assertions of every gxe_finish case: n_valid, the gathered columns exactly and the computed ones within
    the bound (b64.check_episode), and bit-equality with the host path"""
    from guardx_amd.rollout_buffer import episode_rollout_batch
    dev = b64.to_numpy(episode_rollout_batch(out_dev if out_dev is not None else b64.to_torch(g, 'cuda'), GAMMA, LAM))
    host = b64.to_numpy(episode_rollout_batch(out_host if out_host is not None else b64.to_torch(g), GAMMA, LAM))
    ref = b64.episode64(g, GAMMA, LAM)
    T, N = g['rew'].shape
    assert dev['n_valid'] == ref['n_valid'] == int(b64.episode_lengths(g['first_done'], T).sum())
    b64.check_episode(dev, ref, "gxe_finish", case)
    assert set(dev) == set(host)
    for k in dev:
        if k != 'n_valid':
            assert dev[k].dtype == host[k].dtype == np.float32 and dev[k].shape == host[k].shape, k
            assert (_bits(dev[k]) == _bits(host[k])).all(), f"{case}: {k} differs from the host path in its bits"
    return dev


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", PARTITION_N)
def test_finish_block_partition(N, form):
    """N on either side of the 256-env block of launch 1; first_done cycles through 0, 1, T - 1, T, T + 4 (the clamp) with
    period 5, so the lengths on either side of a block boundary differ.  N >= 257: `blk > 0`, and n_valid comes from the
    partly filled last block"""
    g = b64.episode_inputs(**b64.partition_case(N, form))
    _episode(g, f"partition N={N} {form}")


@pytest.mark.parametrize("name,kw", b64.episode_cases(), ids=[c[0] for c in b64.episode_cases()])
def test_finish_cases(name, kw):
    """bsum-stride: N = 256 * 257 + 3, the smallest at which the offset loop of the last envs takes a second turn over the
    block sums.  gather-stride: L in (600, 257, 600) and (600, 1, 600) at T = 600, D + 2 A = 11: three turns of the row
    loops, L W > 256 many times over; -b with rewards of mean 100, deviation 1.  Then L = 1 everywhere, no env finished
    (n_valid == N T), and N = 1."""
    g = b64.episode_inputs(**kw)
    dev = _episode(g, name)
    if name == 'all-unfinished':
        assert dev['n_valid'] == kw['N'] * kw['T']
    if name == 'all-length-1':
        assert dev['n_valid'] == kw['N']


def test_finish_inputs_as_callers_hand_them():
    """the wrapper hands raw pointers to C, so its conversions are part of what is tested: int64 first_done, float64 rew,
    a transposed view as val"""
    import torch
    g = b64.episode_inputs(N=9, T=6, D=5, A=3, first_done=(0, 1, 5, 6, 10, 2, 0, 3, 6), form='cost', seed=8)

    def handed(device):
        out = b64.to_torch(g, device)
        out['first_done'] = out['first_done'].to(torch.int64)
        out['rew'] = out['rew'].to(torch.float64)
        out['val'] = out['val'].t().contiguous().t()
        assert not out['val'].is_contiguous() and out['val'].shape == g['val'].shape
        return out
    _episode(g, "callers' dtypes", handed('cuda'), handed(None))


# ---------------------------------------------------------------------------------------------------------------------
# gx_gae.hip
# ---------------------------------------------------------------------------------------------------------------------
def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.mark.parametrize("T", b64.GAE_T)
@pytest.mark.parametrize("N", b64.GAE_N)
def test_gae_rollout(N, T):
    from guardx_amd.rollout_buffer import gae_rollout
    coef = b64.coef_gae(GAMMA, LAM)
    for kind in b64.GAE_DONE + ('mixed',):
        rew, val, done, lv = b64.gae_inputs(N, T, 'none' if kind == 'mixed' else kind, mixed=kind == 'mixed')
        assert np.abs(lv).min() >= 1
        got = {}
        for name, last in (('none', None), ('given', lv)):
            adv, ret = gae_rollout(_dev(rew), _dev(val), _dev(done), None if last is None else _dev(last), GAMMA, LAM)
            got[name] = adv.cpu().numpy(), ret.cpu().numpy()
            _, (r64, Br), (a64, Ba) = b64.rollout64(rew, val, done, last, coef)
            case = f"N={N} T={T} done={kind} last_val={name}"
            b64.check(got[name][0], (a64, Ba), "gx_gae_rollout", "adv raw", case)
            b64.check(got[name][1], (r64, Br), "gx_gae_rollout", "ret", case)
        same = all((_bits(a) == _bits(b)).all() for a, b in zip(got['none'], got['given']))
        if kind in ('every', 'last'):        # done at step T - 1: the given last_val has no effect
            assert same, (N, T, kind)
        if kind == 'none':
            assert not same


@pytest.mark.parametrize("bootstrap", [False, True])
def test_statewise_and_cost_rollout_batch(bootstrap):
    from guardx_amd.rollout_buffer import cost_rollout_batch, statewise_rollout_batch
    N, T, D, A = 65, 9, 5, 3
    rew, val, done, _ = b64.gae_inputs(N, T, 'none', seed=3, mixed=True)
    done[T - 1, ::2] = 1                                # the bootstrap must skip these
    o = b64.rollout_out(N, T, D, A, rew, val, done, seed=4)
    out = {k: _dev(v) for k, v in o.items()}
    alive = 1.0 - done[T - 1]
    lv, lvc = (o['val_last'] * alive, o['vc_last'] * alive) if bootstrap else (None, None)
    got = b64.to_numpy(statewise_rollout_batch(out, GAMMA, LAM, cgamma=1.0, clam=0.95, bootstrap=bootstrap))
    adv, ret, _ = b64.rollout64(rew, val, done, lv, b64.coef_gae(GAMMA, LAM), 1)
    adc, cret, _ = b64.rollout64(o['cost_inc'], o['vc'], done, lvc, b64.coef_gae(1.0, 0.95), 0)
    who, case = "statewise_rollout_batch", f"N={N} T={T} bootstrap={bootstrap}"

    def batch(got, adv, ret, adc, cret, who, case):
        for k in ('obs', 'act', 'logp', 'mu'):
            np.testing.assert_array_equal(got[k], b64.env_major(o[k]), err_msg=k)
        b64.check(got['adv'], tuple(x.reshape(-1) for x in adv), who, 'adv', case)
        b64.check(got['adc'], tuple(x.reshape(-1) for x in adc), who, 'adc', case)
        b64.check(got['ret'], tuple(b64.env_major(x) for x in ret), who, 'ret', case)
        b64.check(got['cost_ret'], tuple(b64.env_major(x) for x in cret), who, 'cost_ret', case)
    batch(got, adv, ret, adc, cret, who, case)
    if bootstrap:                                       # and the bootstrap is there: without it the returns differ
        plain = b64.rollout64(rew, val, done, None, b64.coef_gae(GAMMA, LAM), 1)
        assert b64.outside(got['ret'], tuple(b64.env_major(x) for x in plain[1])) > b64.FACTOR
    else:                                               # cost_rollout_batch on the same data: CPO's gamma and lambda on cost / vc
        got = b64.to_numpy(cost_rollout_batch(out, GAMMA, LAM))
        adc, cret, _ = b64.rollout64(o['cost'], o['vc'], done, None, b64.coef_gae(GAMMA, LAM), 0)
        batch(got, adv, ret, adc, cret, "cost_rollout_batch", f"N={N} T={T}")


@pytest.mark.parametrize("T", b64.NORM_T)
def test_adv_normalize(T):
    """one wave per env, four envs per block: T on either side of a wave's 64 lanes and far beyond; N on either side of a
    block; rows whose mean dwarfs their deviation; and nothing written outside the N rows"""
    import torch
    from guardx_amd import _native
    lib = _native.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for N in b64.NORM_N:
        for mean100 in (False, True):
            x = b64.norm_rows(N, T, mean100)
            for scale in (0, 1):
                buf = torch.full((8, T), -7.25, dtype=torch.float32, device='cuda')     # rows N .. 7: not the kernel's
                buf[:N] = _dev(x)
                _native.check(lib.gx_adv_normalize(N, T, buf.data_ptr(), scale, stream))
                got = buf.cpu().numpy()
                assert (got[N:] == -7.25).all(), (N, T, scale)
                b64.check(got[:N], b64.normalize64(x, np.zeros((N, T)), scale), "gx_adv_normalize",
                          "adv" if scale else "adc", f"N={N} T={T} scale={scale} " + ("mean 100" if mean100 else "N(0, 1)"))


@pytest.mark.parametrize("closing", ["done=None", "ones"])
@pytest.mark.parametrize("cost", [False, True])
def test_device_buffers_store_finish_get(cost, closing):
    """store / finish_path / get at (N, T) = (65, 9): a finish_path after step 3 that closes some envs, one after step 6
    that closes the rest, the closing one over every env, as done=None and as explicit ones"""
    import torch
    from guardx_amd.rollout_buffer import DeviceCostRolloutBuffer, DeviceRolloutBuffer
    N, T, D, A = 65, 9, 5, 3
    rng = np.random.default_rng(17 + cost)
    r = lambda *s: rng.normal(size=s).astype(np.float32)   # noqa: E731
    rew, val, cst, cval = r(T, N), r(T, N), rng.random((T, N)).astype(np.float32), r(T, N)
    obs, act, mu, ls = b64.encoded(T, N, D, 0), b64.encoded(T, N, A, 1), b64.encoded(T, N, A, 2), b64.encoded(T, N, A, 3)
    logp = r(T, N)
    G = (DeviceCostRolloutBuffer if cost else DeviceRolloutBuffer)(N, T, (D,), (A,), gamma=GAMMA, lam=LAM, device='cuda')
    some = (rng.random(N) < 0.4).astype(np.float32)
    some[0], some[64] = 1, 0
    calls = {3: some, 6: 1 - some, T - 1: np.ones(N, np.float32)}
    close, boot, cboot = np.zeros((T, N), bool), np.zeros((T, N)), np.zeros((T, N))
    start = np.zeros(N, np.int32)
    for t in range(T):
        more = (_dev(cst[t]), _dev(cval[t])) if cost else ()
        G.store(_dev(obs[t]), _dev(act[t]), _dev(rew[t]), _dev(val[t]), _dev(logp[t]), *more, _dev(mu[t]), _dev(ls[t]))
        if t in calls:
            done, lv, lcv = calls[t], r(N), r(N)
            dn = None if (t == T - 1 and closing == "done=None") else _dev(done)
            if cost:
                G.finish_path(_dev(lv), _dev(lcv), dn)
            else:
                G.finish_path(_dev(lv), dn)
            close[t], boot[t], cboot[t] = done == 1, lv, lcv
            start = np.where(done == 1, t + 1, start).astype(np.int32)
            assert G.path_start_idx.dtype == torch.int32
            np.testing.assert_array_equal(G.path_start_idx.cpu().numpy(), start, err_msg=f"after step {t}")
    coef = b64.coef_gae(GAMMA, LAM)
    who = "DeviceCostRolloutBuffer" if cost else "DeviceRolloutBuffer"
    case = f"N={N} T={T} {closing}"
    adv, ret, Ba, Br = b64.gae64(rew, val, close, boot, coef)
    b64.check(G.adv_buf.cpu().numpy(), (adv.T, Ba.T), who, "adv raw", case)
    b64.check(G.ret_buf.cpu().numpy(), (ret.T, Br.T), who, "ret", case)
    if cost:
        adc, cret, Bc, Bcr = b64.gae64(cst, cval, close, cboot, coef)
        b64.check(G.adc_buf.cpu().numpy(), (adc.T, Bc.T), who, "adc raw", case)
        b64.check(G.cost_ret_buf.cpu().numpy(), (cret.T, Bcr.T), who, "cost_ret", case)
    d = b64.to_numpy(G.get())
    for k, x in (('obs', obs), ('act', act), ('mu', mu), ('logstd', ls), ('logp', logp)):
        np.testing.assert_array_equal(d[k], b64.env_major(x), err_msg=k)
    b64.check(d['adv'], tuple(x.reshape(-1) for x in b64.normalize64(adv.T, Ba.T, 1)), who, "adv", case)
    b64.check(d['ret'], (b64.env_major(ret), b64.env_major(Br)), who, "ret", case)
    if cost:
        b64.check(d['adc'], tuple(x.reshape(-1) for x in b64.normalize64(adc.T, Bc.T, 0)), who, "adc", case)
        b64.check(d['cost_ret'], (b64.env_major(cret), b64.env_major(Bcr)), who, "cost_ret", case)
    assert G.ptr == 0 and int(G.path_start_idx.abs().sum()) == 0
