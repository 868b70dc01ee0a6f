"""The host side of guardx_amd.epstats (the learners' EpRet / EpCost / EpLen / EpCostRet / MaxEpLenRet / VVals from a
rollout's (T, N) tensors): its host-tensor path against the independent restatement of the learner loop
(tests/epstats64.py), the fixed order of its float64 sums, and the ninth library's argument checks and device code
(its build identity and ABI: tests/test_build_identity.py)."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import epstats64 as e64

STAT_KEYS = ('EpRet', 'EpCost', 'EpLen', 'EpCostRet', 'MaxEpLenRet', 'VVals')


def make(seed, T, N, density, *, values=(1.0,)):
    """rew ~ N(0, 1), real-valued cost in [0, 1), done = one of `values` with probability `density`, val ~ N(0, 1)"""
    rng = np.random.default_rng(seed)
    f = np.float32
    done = np.where(rng.random((T, N)) < density, rng.choice(np.asarray(values, f), size=(T, N)), f(0)).astype(f)
    return dict(rew=rng.normal(size=(T, N)).astype(f), cost=rng.random((T, N)).astype(f), done=done,
                val=rng.normal(size=(T, N)).astype(f))


def tt(d, *keys):
    return [torch.from_numpy(np.ascontiguousarray(d[k])) for k in keys]


def bits(x):
    return np.asarray(x, dtype=np.float64).reshape(-1).view(np.int64).tolist()


def same_bits(a, b):
    return bits(a) == bits(b)


def check_key(got, xs, name):
    """one key of a result against the entries `xs` the restatement logged: n, min and max exact; S, mean and Q bit-equal to
    the explicit loop over the 256 slots, and within the forward-error bound of a float64 sum against math.fsum"""
    x = e64.logged(xs)
    want = e64.stats64(xs)
    n = len(x)
    assert float(got['n']) == n == want['n'], name
    assert same_bits(got['min'], want['min']) and same_bits(got['max'], want['max']), name
    S = e64.slot_sum_loop(x)
    mean = float(np.float64(S) / np.float64(n)) if n else math.nan
    q = [float((np.float64(v) - np.float64(mean)) * (np.float64(v) - np.float64(mean))) for v in x]
    Q = e64.slot_sum_loop(q)
    assert same_bits(got['S'], S) and same_bits(got['mean'], mean) and same_bits(got['Q'], Q), name
    assert same_bits(got['std'], np.sqrt(np.float64(Q) / np.float64(n)) if n else math.nan), name
    if n == 0 or math.isnan(want['S']):
        return
    # a float64 sum of n terms against the exact one: (n - 1) u sum |x|; the mean adds the division's rounding, u |mean|
    bS = e64.sum_bound(x)
    assert abs(S - want['S']) <= bS, (name, S - want['S'], bS)
    assert abs(mean - want['mean']) <= bS / n + e64.U * abs(want['mean']), name
    # Q: the same terms (deviations from the product's own mean, which the bits above pin) summed exactly
    assert abs(Q - math.fsum(q)) <= e64.sum_bound(q), name
    # and against the deviations from the exact mean: d/dm sum (x - m)^2 = -2 sum (x - m), so a mean off by dm moves Q by
    # at most 2 |dm| sum |x - m| + n dm^2; each term's own rounding (one subtraction, one product) is within 3 u of it
    dm = bS / n + e64.U * abs(want['mean'])
    dev = math.fsum(abs(v - want['mean']) for v in x)
    assert abs(Q - want['Q']) <= e64.sum_bound(q) + 3 * e64.U * math.fsum(q) + 2 * dm * dev + n * dm * dm + e64.U * want['Q'], name


def check_result(got, log, *, gamma, timeout, val):
    from guardx_amd.epstats import KEYS
    assert KEYS == STAT_KEYS
    present = {'EpRet', 'EpCost', 'EpLen'} | ({'EpCostRet'} if gamma is not None else set()) | \
        ({'MaxEpLenRet'} if timeout else set()) | ({'VVals'} if val else set())
    assert {k for k in got if k in STAT_KEYS} == present
    for k in sorted(present):
        check_key(got[k], log[k], k)
    assert int(got['n_episodes']) == len(log['env']) and got['n_episodes'].dtype == torch.int32
    cs = e64.slot_sum_loop(log['cost_env'])
    assert same_bits(got['cost_sum'], cs) and abs(cs - log['cost_sum']) <= e64.sum_bound(log['cost_env'])
    if 'env' in got:
        assert got['env'].tolist() == log['env'] and got['t_end'].tolist() == log['t_end']
        assert got['ep_len'].tolist() == log['EpLen'] and got['ep_len'].dtype == torch.int32
        for k, name in (('ep_ret', 'EpRet'), ('ep_cost', 'EpCost')) + ((('ep_cost_ret', 'EpCostRet'),) if gamma is not None else ()):
            assert got[k].dtype == torch.float64 and same_bits(got[k].numpy(), log[name]), k


# ---------------------------------------------------------------------------------------------------------------------
# the host path against the restatement
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T,N,density,gamma,val", [(1, 1, 1.0, None, False), (7, 5, 0.0, 0.99, True), (33, 70, 0.02, None, True),
                                                    (33, 130, 0.5, 0.99, True), (12, 300, 1.0, 0.9, False)])
def test_host_path_against_the_restatement(T, N, density, gamma, val):
    from guardx_amd.epstats import episode_stats
    d = make(T * 1000 + N, T, N, density)
    log, _ = e64.learner_loop(d['rew'], d['cost'], d['done'], gamma=gamma, val=d['val'] if val else None)
    rew, cost, done, v = tt(d, 'rew', 'cost', 'done', 'val')
    got = episode_stats(rew, cost, done, val=v if val else None, gamma=gamma, episodes=True)
    check_result(got, log, gamma=gamma, timeout=True, val=val)
    if (T, N) == (33, 130):
        assert len(log['env']) > 8 * 256             # the slots hold several entries each and the tree is full
    # the dict form: val is taken from the rollout dict, val=False leaves it out; the static method is the same call
    from guardx_amd import Engine
    out = dict(rew=rew, cost=cost, done=done, val=v, obs=torch.zeros(T, N, 3))
    a, b = Engine.episode_stats(out, gamma=gamma), episode_stats(rew, cost, done, val=v, gamma=gamma)
    assert 'VVals' in a and 'env' not in a and 'VVals' not in episode_stats(out, val=False)
    for k in a:
        if k in STAT_KEYS:
            assert all(same_bits(a[k][f], b[k][f]) for f in a[k]), k
    assert got['carry']['t'] == 0 and not got['carry']['acc'].any() and not got['carry']['len'].any()


def test_an_epoch_longer_than_the_call_has_no_time_out_step():
    from guardx_amd.epstats import episode_stats
    d = make(3, 9, 40, 0.2)
    log, st = e64.learner_loop(d['rew'], d['cost'], d['done'], max_ep_len=20, gamma=0.95)
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'), max_ep_len=20, gamma=0.95, episodes=True)
    check_result(got, log, gamma=0.95, timeout=False, val=False)
    c = got['carry']
    assert c['t'] == 9 and c['len'].tolist() == st['ep_len']
    for i, k in enumerate(('ep_ret', 'ep_cost', 'ep_cost_ret', 'epoch_ret')):
        assert same_bits(c['acc'][i].numpy(), st[k]), k


@pytest.mark.parametrize("split", ["1", "half", "T-1"])
def test_chunked_calls_with_carry_equal_the_single_call(split):
    from guardx_amd.epstats import episode_stats
    T, N = 20, 70
    k = {"1": 1, "half": T // 2, "T-1": T - 1}[split]
    d = make(11, T, N, 0.15)
    rew, cost, done, val = tt(d, 'rew', 'cost', 'done', 'val')
    whole = episode_stats(rew, cost, done, val=val, gamma=0.99, episodes=True)
    first = episode_stats(rew[:k], cost[:k], done[:k], val=val[:k], gamma=0.99, max_ep_len=T, episodes=True)
    assert 'MaxEpLenRet' not in first and first['carry']['t'] == k
    before = [x.clone() for x in (first['carry']['acc'], first['carry']['len'])]
    second = episode_stats(rew[k:], cost[k:], done[k:], val=val[k:], gamma=0.99, carry=first['carry'], episodes=True)
    assert torch.equal(first['carry']['acc'], before[0]) and torch.equal(first['carry']['len'], before[1])
    for key in ('env', 't_end', 'ep_ret', 'ep_cost', 'ep_cost_ret', 'ep_len'):
        both = torch.cat([first[key], second[key]])
        assert both.dtype == whole[key].dtype and bits(both.double().numpy()) == bits(whole[key].double().numpy()), key
    assert all(same_bits(second['MaxEpLenRet'][f], whole['MaxEpLenRet'][f]) for f in whole['MaxEpLenRet'])
    assert int(first['n_episodes']) + int(second['n_episodes']) == int(whole['n_episodes'])
    assert second['carry']['t'] == 0 and not second['carry']['acc'].any() and not second['carry']['len'].any()
    # the statistics of the two calls' lists, taken together, are the single call's
    from guardx_amd.epstats import moments_host
    for key, name in (('ep_ret', 'EpRet'), ('ep_cost', 'EpCost'), ('ep_len', 'EpLen'), ('ep_cost_ret', 'EpCostRet')):
        m = moments_host(torch.cat([first[key], second[key]]).numpy())
        assert same_bits(m, [float(whole[name][f]) for f in ('n', 'S', 'mean', 'Q', 'min', 'max', 'std')]), name
    # a third call of the epoch would run past its end
    with pytest.raises(ValueError, match="max_ep_len"):
        episode_stats(rew[:2], cost[:2], done[:2], carry=dict(first['carry'], t=T - 1))


def test_the_time_out_rule():
    """env 0 is done at step 2 and again on the last step: nothing there (its ep_len is not the epoch's); env 1 is never
    done: one episode of the whole epoch; env 2 is done on the last step only: one episode, by the ep_len rule"""
    from guardx_amd.epstats import episode_stats
    T = 6
    rew = torch.arange(1, 3 * T + 1, dtype=torch.float32).reshape(T, 3)
    cost = torch.ones(T, 3)
    done = torch.zeros(T, 3)
    done[2, 0] = done[T - 1, 0] = done[T - 1, 2] = 1
    got = episode_stats(rew, cost, done, episodes=True)
    assert got['env'].tolist() == [0, 1, 2] and got['t_end'].tolist() == [2, T - 1, T - 1]
    assert got['ep_len'].tolist() == [3, T, T]
    assert got['ep_ret'].tolist() == [float(rew[:3, 0].sum()), float(rew[:, 1].sum()), float(rew[:, 2].sum())]
    assert float(got['MaxEpLenRet']['n']) == 3 and float(got['MaxEpLenRet']['S']) == float(rew.sum())
    assert float(got['MaxEpLenRet']['max']) == float(rew[:, 2].sum())
    assert float(got['cost_sum']) == 3 * T
    log, _ = e64.learner_loop(rew.numpy(), cost.numpy(), done.numpy())
    check_result(got, log, gamma=None, timeout=True, val=False)


def test_done_values_other_than_one_are_not_ends():
    from guardx_amd.epstats import episode_stats
    d = make(5, 10, 30, 0.4, values=(1.0, 0.5, 2.0, -1.0, np.nan, 0.99999994))
    log, _ = e64.learner_loop(d['rew'], d['cost'], d['done'], max_ep_len=11)
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'), max_ep_len=11, episodes=True)
    ones = [(t, e) for t in range(10) for e in range(30) if d['done'][t, e] == 1]
    assert 0 < len(ones) < int((d['done'] != 0).sum()) and list(zip(got['t_end'].tolist(), got['env'].tolist())) == ones
    check_result(got, log, gamma=None, timeout=False, val=False)


def test_no_episode_gives_the_empty_statistics():
    from guardx_amd.epstats import episode_stats
    d = make(6, 5, 9, 0.0)
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'), max_ep_len=8, gamma=0.9, episodes=True)
    assert int(got['n_episodes']) == 0 and got['env'].numel() == 0 and got['ep_ret'].numel() == 0
    for k in ('EpRet', 'EpCost', 'EpLen', 'EpCostRet'):
        s = got[k]
        assert float(s['n']) == 0 and math.isnan(float(s['mean'])) and math.isnan(float(s['std']))
        assert float(s['min']) == math.inf and float(s['max']) == -math.inf
    # N == 0 and T == 0: the same, and nothing to carry
    for shape in ((0, 4), (3, 0)):
        z = torch.zeros(shape)
        e = episode_stats(z, z, z, max_ep_len=5)
        assert int(e['n_episodes']) == 0 and math.isnan(float(e['EpRet']['mean'])) and float(e['cost_sum']) == 0
        assert e['carry']['t'] == shape[0]


def test_a_planted_nan_reaches_mean_std_min_and_max_of_its_key_alone():
    from guardx_amd.epstats import episode_stats
    d = make(7, 12, 20, 0.2)
    d['rew'][4, 3] = np.nan
    log, _ = e64.learner_loop(d['rew'], d['cost'], d['done'])
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'), episodes=True)
    for k in ('EpRet', 'MaxEpLenRet'):
        assert all(math.isnan(float(got[k][f])) for f in ('mean', 'std', 'min', 'max')), k
        assert float(got[k]['n']) == len(log[k])
    assert all(math.isfinite(float(got['EpCost'][f])) for f in ('mean', 'std', 'min', 'max'))
    check_result(got, log, gamma=None, timeout=True, val=False)


def test_the_gamma_table_and_the_epoch_step_discount():
    from guardx_amd.epstats import discount_table, episode_stats
    g = discount_table(0.99, 50)
    assert g.dtype == np.float64 and g.tolist() == [0.99 ** k for k in range(50)]
    # one env, done at step 1: its second episode's first cost is discounted by gamma ** 2, the epoch's step
    cost = torch.tensor([[1.0], [1.0], [1.0], [1.0]])
    done = torch.tensor([[0.0], [1.0], [0.0], [0.0]])
    got = episode_stats(torch.zeros(4, 1), cost, done, gamma=0.5, max_ep_len=5, episodes=True)
    assert got['ep_cost_ret'].tolist() == [1.5] and got['carry']['acc'][2].tolist() == [0.25 + 0.125]
    assert 'EpCostRet' not in episode_stats(torch.zeros(4, 1), cost, done)


def test_the_one_episode_form():
    from guardx_amd.epstats import episode_stats
    rng = np.random.default_rng(2)
    N, T, t0 = 300, 7, 5
    out = dict(ep_ret=torch.from_numpy(rng.normal(size=N).astype(np.float32)), ep_cost=torch.from_numpy(rng.random(N).astype(np.float32)),
               first_done=torch.from_numpy(rng.integers(0, 13, N).astype(np.int32)), rew=torch.zeros(T, N), t0=t0)
    got = episode_stats(out)
    L = t0 + T
    lens = [int(v) if v > 0 else L for v in out['first_done']]
    assert 0 in out['first_done'].tolist()
    check_key(got['EpRet'], out['ep_ret'].tolist(), 'EpRet')
    check_key(got['EpCost'], out['ep_cost'].tolist(), 'EpCost')
    check_key(got['EpLen'], lens, 'EpLen')
    assert int(got['n_episodes']) == N and 'carry' not in got
    y = [float(np.float64(v) / np.float64(L)) for v in out['ep_ret'].tolist()]
    v = float(np.float32(np.float64(e64.slot_sum_loop(y)) / np.float64(N) * 1000.0))
    m = got['MaxEpLenRet']
    assert float(m['n']) == 1 and same_bits(m['mean'], v) and same_bits(m['min'], v) and same_bits(m['max'], v)
    assert float(m['std']) == 0.0
    # against exact sums: the sum's bound over N, the division's and the product's rounding, then the float32 of the logger
    exact = math.fsum(y) / N * 1000.0
    assert abs(v - exact) <= 1000.0 * (e64.sum_bound(y) / N) + 3 * e64.U * abs(exact) + 2.0 ** -24 * abs(exact)


def test_constraint_value():
    from guardx_amd.epstats import constraint_value, episode_stats
    d = make(8, 15, 25, 0.1)
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'))
    c = constraint_value(got, 25.0)
    assert c.dtype == torch.float64 and c.dim() == 0
    assert float(c) == (float(got['EpCost']['mean']) - 25.0) / (float(got['EpLen']['mean']) + 1e-8)
    assert float(constraint_value(got, 1.0, eps=0.5)) == (float(got['EpCost']['mean']) - 1.0) / (float(got['EpLen']['mean']) + 0.5)


def test_value_errors():
    from guardx_amd.epstats import episode_stats
    z = torch.zeros(4, 3)
    with pytest.raises(ValueError, match="max_ep_len"):
        episode_stats(z, z, z, max_ep_len=3)
    first = episode_stats(z[:3], z[:3], z[:3], max_ep_len=5)
    with pytest.raises(ValueError, match="max_ep_len"):
        episode_stats(z[:3], z[:3], z[:3], carry=first['carry'])              # 3 + 3 > 5: the carry remembers the epoch
    for bad in (dict(cost=torch.zeros(4, 2)), dict(done=torch.zeros(3, 3)), dict(val=torch.zeros(4, 4)), dict(done=torch.zeros(12))):
        kw = dict(dict(cost=z, done=z), **bad)
        with pytest.raises(ValueError, match="episode_stats"):
            episode_stats(z, kw.pop('cost'), kw.pop('done'), **kw)
    with pytest.raises(ValueError, match="rew, cost and done"):
        episode_stats(z, z)
    with pytest.raises(ValueError, match="carry"):
        episode_stats(z, z, z, carry=dict(first['carry'], acc=torch.zeros(4, 2, dtype=torch.float64)))
    with pytest.raises(KeyError, match="cost"):
        episode_stats(dict(rew=z, done=z))


@pytest.mark.parametrize("mistake", e64.MISTAKES)
def test_planted_mistakes_are_told_apart(mistake):
    """each of the errors the loop invites, planted into the restatement, no longer agrees with the product on data that
    reaches it; the unplanted restatement does"""
    from guardx_amd.epstats import episode_stats
    d = make(21, 24, 40, 0.15, values=(1.0, 1.0, 2.0))
    d['done'][-1, :20] = 1                                         # done envs on the time-out step
    d['rew'] *= np.float32(1000.1)                                 # sums whose float32 rounding shows
    kw = dict(gamma=0.97)
    got = episode_stats(*tt(d, 'rew', 'cost', 'done'), episodes=True, **kw)
    good, _ = e64.learner_loop(d['rew'], d['cost'], d['done'], **kw)
    check_result(got, good, timeout=True, val=False, **kw)
    bad, _ = e64.learner_loop(d['rew'], d['cost'], d['done'], mistake=mistake, **kw)
    with pytest.raises(AssertionError):
        check_result(got, bad, timeout=True, val=False, **kw)
    differs = {'clear_epoch_ret_at_done': 'MaxEpLenRet', 'log_done_on_timeout': 'env', 'greater_for_equal': 'env',
               'float32_accumulators': 'EpRet', 'discount_by_episode_step': 'EpCostRet'}[mistake]
    assert bad[differs] != good[differs]


# ---------------------------------------------------------------------------------------------------------------------
# libguardx_epstats.so: its argument checks and its device code (build identity and ABI: tests/test_build_identity.py)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from guardx_amd import build, _epstats_native
    build.build()                      # hipcc --offload-arch=gfx950 cross-compiles without a GPU
    return _epstats_native.load()      # refuses a library whose build id is not the tree's


def test_sizes_and_bad_arguments_are_errors_not_crashes(lib):
    from guardx_amd import _epstats_native as n
    W = lambda N: (N + 63) // 64   # noqa: E731
    for N, T in ((1, 1), (64, 3), (65, 7), (2000, 200)):
        assert lib.gxt_work_bytes(N, T) == 8 * (3 * T * N + N + T * W(N)) + 4 * (T * N + T * W(N))
    assert lib.gxt_work_bytes(0, 0) == 0 and lib.gxt_work_bytes(-1, 4) == -1 and lib.gxt_work_bytes(4, -1) == -1
    assert lib.gxt_work_bytes(1 << 20, 1 << 11) == -1 and lib.gxt_work_bytes((1 << 20) - 64, 1 << 11) > 0
    fake = 4096                        # never dereferenced: every call below fails its checks before any HIP call

    def stats(N=4, T=3, t0=0, L=3, ptrs=None):
        p = [fake] * 19 if ptrs is None else ptrs
        return lib.gxt_episode_stats(N, T, t0, L, *p, None)
    assert stats(N=-1) == n.GXT_ERR_ARG and stats(T=-1) == n.GXT_ERR_ARG and stats(t0=-1) == n.GXT_ERR_ARG
    assert stats(L=2) == n.GXT_ERR_ARG and b"max_ep_len" in lib.gxt_last_error()
    assert stats(t0=1) == n.GXT_ERR_ARG and stats(T=0x7fffffff, t0=0x7fffffff, L=0x7fffffff) == n.GXT_ERR_ARG
    for i in range(19):
        p = [fake] * 19
        p[i] = None
        want = n.GXT_OK if i in (3, 4) else n.GXT_ERR_ARG           # d_val and d_gpow are optional
        assert stats(N=0, ptrs=p) == want, i                        # (one of d_carry_in / d_carry_len_in alone is not)
    assert b"null pointer" in lib.gxt_last_error()
    assert stats(N=0, ptrs=[fake] * 5 + [None, None] + [fake] * 12) == n.GXT_OK   # no carry: the accumulators start at zero
    assert stats(N=1 << 20, T=1 << 11, L=1 << 11) == n.GXT_ERR_UNSUPPORTED
    assert stats(N=0) == n.GXT_OK and stats(T=0) == n.GXT_OK           # nothing to do, nothing launched
    assert lib.gxt_moments(1, 4, 0, None, fake, None) == n.GXT_ERR_ARG
    assert lib.gxt_moments(1, 4, 1, fake, None, None) == n.GXT_ERR_ARG
    assert lib.gxt_moments(-1, 4, 0, fake, fake, None) == n.GXT_ERR_ARG and lib.gxt_moments(1, -4, 0, fake, fake, None) == n.GXT_ERR_ARG
    assert lib.gxt_moments(0, 4, 0, fake, fake, None) == n.GXT_OK
    with pytest.raises(n.GxtError, match="status 1"):
        n.check(stats(L=2))


def test_no_scratch_in_the_device_code(tmp_path):
    """hipcc --offload-arch=gfx950 compiles the six kernels of the library (the scan, the offsets, the scatter, the
    moments per key and per row of float32 / float64) with a private segment of zero bytes"""
    from guardx_amd import build
    asm = tmp_path / "gx_epstats.s"
    subprocess.check_call([os.environ.get("HIPCC", "hipcc")] + build.FLAGS + ["--cuda-device-only", "-S", "-o", str(asm),
                                                                             os.path.join(build.CSRC, "gx_epstats.hip")])
    text = asm.read_text()
    scratch = [int(v) for v in re.findall(r"\.amdhsa_private_segment_fixed_size\s+(\d+)", text)]
    print("epstats kernels:", len(scratch), "vgpr", re.findall(r"\.amdhsa_next_free_vgpr\s+(\d+)", text))
    assert len(scratch) == 6 and max(scratch) == 0
