"""The host paths of guardx_amd/rollout_buffer.py against the float64 restatement tests/buffer64.py, the restatement
against the two numpy restatements of the original buffers the repository already has, and the proof that the
comparison can fail.  No GPU.  The inputs are those of tests/test_gpu_buffer64.py, which runs the kernels on them."""
import numpy as np
import pytest

import buffer64 as b64
from buffer64 import FACTOR, FORMS, PARTITION_N

GAMMA, LAM = 0.99, 0.95


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (who, output), (r, case) in sorted(b64.RATIOS.items()):
        print(f"\nlargest error/bound {who:28s} {output:9s} {r:8.3f}  {case}", end="")


def _host_episode(g, **kw):
    from guardx_amd.rollout_buffer import episode_rollout_batch
    return b64.to_numpy(episode_rollout_batch(b64.to_torch(g), **kw))


_cache = {}


def _partition(N, form):
    """(inputs, host batch), computed once and left unchanged"""
    if (N, form) not in _cache:
        g = b64.episode_inputs(**b64.partition_case(N, form))
        _cache[(N, form)] = (g, _host_episode(g))
    return _cache[(N, form)]


# ---------------------------------------------------------------------------------------------------------------------
# the host paths within FACTOR x bound
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("N", PARTITION_N)
def test_episode_host_path_block_partition(N, form):
    g, got = _partition(N, form)
    got = dict(got)
    A = g['act'].shape[-1]
    np.testing.assert_array_equal(got['logstd'], np.broadcast_to(g['logstd'], (got['n_valid'], A)))
    b64.check_episode(got, b64.episode64(g, GAMMA, LAM), "host episode_rollout_batch", f"partition N={N} {form}")


@pytest.mark.parametrize("name,kw", b64.episode_cases(), ids=[c[0] for c in b64.episode_cases()])
def test_episode_host_path_cases(name, kw):
    g = b64.episode_inputs(**kw)
    b64.check_episode(_host_episode(g), b64.episode64(g, GAMMA, LAM), "host episode_rollout_batch", name)


def test_episode_host_path_inputs_as_callers_hand_them():
    """int64 first_done, float64 rew, a transposed view as val: the values are float32-exact, so nothing changes"""
    import torch
    from guardx_amd.rollout_buffer import episode_rollout_batch
    g = b64.episode_inputs(N=9, T=6, D=5, A=3, first_done=(0, 1, 5, 6, 10, 2, 0, 3, 6), form='cost', seed=8)
    out = b64.to_torch(g)
    out['first_done'] = out['first_done'].to(torch.int64)
    out['rew'] = out['rew'].to(torch.float64)
    out['val'] = out['val'].t().contiguous().t()
    assert not out['val'].is_contiguous()
    b64.check_episode(b64.to_numpy(episode_rollout_batch(out)), b64.episode64(g, GAMMA, LAM), "host episode_rollout_batch",
                      "callers' dtypes")


def _rollout_host_case(N, T, kind, mixed, done_values=None):
    """safelayer / usl / lpg_rollout_batch on host tensors (all through _gae_host) against buffer64.  The reference's
    coefficients here are _gae_host's OWN, plain float32 throughout (b64.coef_host, f32_filters=True): it multiplies
    float32 tensors by python scalars and keeps both filters in float32, unlike the kernels' double filters."""
    from guardx_amd import rollout_buffer as rb
    rew, val, done, _ = b64.gae_inputs(N, T, kind, mixed=mixed)
    if done_values is not None:          # `done` values other than 0 and 1: only == 1 closes a path
        done = np.random.default_rng(5).choice(np.asarray(done_values, np.float32), size=(T, N))
    case = f"N={N} T={T} done={'mixed' if mixed else kind}" + (f" values {done_values}" if done_values else "")
    o = b64.rollout_out(N, T, 5, 3, rew, val, done)
    (adv, Ba), (ret, Br), _ = b64.rollout64(rew, val, done, None, b64.coef_host(GAMMA, LAM), 1, True)
    end = (done == 1) | (np.arange(T)[:, None] == T - 1)
    tc = b64.targetc64(o['cost'], o['qc'], end, GAMMA)
    for fn, extra in ((rb.safelayer_rollout_batch, ('act_safe', 'cost', 'prev_cost')), (rb.usl_rollout_batch, ('act_safe', 'cost')),
                      (rb.lpg_rollout_batch, ('act_safe', 'cost'))):
        got = b64.to_numpy(fn({k: v for k, v in b64.to_torch(o).items() if k != 't0'}, GAMMA, LAM))
        who = "host " + fn.__name__
        for k in ('obs', 'act', 'mu', 'logp') + extra:
            np.testing.assert_array_equal(got[k], b64.env_major(o[k]), err_msg=f"{who} {k}")
        b64.check(got['adv'], (adv.reshape(-1), Ba.reshape(-1)), who, 'adv', case)
        b64.check(got['ret'], (b64.env_major(ret), b64.env_major(Br)), who, 'ret', case)
        if 'targetc' in got:
            b64.check(got['targetc'], tuple(b64.env_major(x) for x in tc), who, 'targetc', case)


@pytest.mark.parametrize("kind", b64.GAE_DONE + ('mixed',))
@pytest.mark.parametrize("T", [2, 70])       # (not T = 1: a normalised row of one entry is 0 / 0)
@pytest.mark.parametrize("N", b64.GAE_N)
def test_gae_host_path(N, T, kind):
    _rollout_host_case(N, T, 'none' if kind == 'mixed' else kind, kind == 'mixed')


def test_done_closes_a_path_where_it_equals_one():
    """The `done` convention.  The kernels close a path where done == 1 (gx_gae.hip), and so do the buffers of the three
    learners the host paths serve (np.where(done == 1): safelayer.py:109, usl.py:112, lpg.py:112); none of them reads
    done > 0.  With values other than 0 and 1 the host paths follow: only the 1s close a path, in the advantages, the
    returns and targetc alike.  (The engine emits 0 and 1 only.)"""
    _rollout_host_case(5, 40, 'none', False, done_values=(0.0, 0.0, 0.0, 1.0, 0.5, 2.0, -1.0))
    # and the reading done > 0 would be noticed: it closes paths at 0.5 and 2 as well
    rew, val, _, _ = b64.gae_inputs(5, 40, 'none')
    done = np.random.default_rng(5).choice(np.asarray((0.0, 0.0, 0.0, 1.0, 0.5, 2.0, -1.0), np.float32), size=(40, 5))
    right = b64.rollout64(rew, val, done, None, b64.coef_host(GAMMA, LAM), 1, True)
    wrong = b64.rollout64(rew, val, (done > 0).astype(np.float32), None, b64.coef_host(GAMMA, LAM), 1, True)
    assert b64.outside(right[1][0], wrong[1]) > FACTOR and b64.outside(right[0][0], wrong[0]) > FACTOR


# ---------------------------------------------------------------------------------------------------------------------
# the restatement against the two older ones.  gamma and lambda are exact in float32 here, so that the three ways of
# rounding the coefficients (buffer64's per kernel, the older restatements' python doubles) are one and the same.
# ---------------------------------------------------------------------------------------------------------------------
G_EXACT, L_EXACT = 63 / 64, 15 / 16


@pytest.mark.parametrize("cost", [False, True])
def test_buffer64_against_the_one_episode_restatement(cost):
    from test_episode_host import _synthetic, one_episode_batch_np
    g = _synthetic(5, cost)
    want, _ = one_episode_batch_np(g, gamma=G_EXACT, lam=L_EXACT)
    # (its bootstrap rule: val_last of an env with a non-finite obs_last is 0 in the data already)
    ref = b64.episode64({k: v for k, v in g.items() if k != 'cost' or cost}, G_EXACT, L_EXACT)
    assert ref['n_valid'] == len(want['ret'])
    for k in ('obs', 'act', 'mu', 'logp'):
        np.testing.assert_array_equal(ref[k], want[k], err_msg=k)
    for k in ('ret', 'adv') + (('cost_ret', 'adc') if cost else ()):
        b64.check(want[k], ref[k], "OneEpisodeBufferNP", k, f"synthetic cost={cost}")


def test_buffer64_against_the_trpo_restatement():
    from oracle.trpo_buffer_np import TRPOBufferNP
    N, T, D, A = 6, 11, 3, 2
    rng = np.random.default_rng(2)
    r = lambda *s: rng.normal(size=s).astype(np.float32)   # noqa: E731
    rew, val = r(T, N), r(T, N)
    O = TRPOBufferNP(N, T, D, A, gamma=G_EXACT, lam=L_EXACT)
    close, boot = np.zeros((T, N), bool), np.zeros((T, N))
    calls = {3: (np.array([1, 0, 1, 0, 0, 1.0]), r(N)), 7: (np.array([0, 1, 1, 0, 0, 0.0]), r(N)), T - 1: (np.ones(N), r(N))}
    for t in range(T):
        O.store(r(N, D), r(N, A), rew[t], val[t], r(N), r(N, A), r(N, A))
        if t in calls:
            done, lv = calls[t]
            O.finish_path(lv, done)
            close[t], boot[t] = done == 1, lv
    adv, ret, Ba, Br = b64.gae64(rew, val, close, boot, b64.coef_gae(G_EXACT, L_EXACT))
    b64.check(O.adv_buf, (adv.T, Ba.T), "TRPOBufferNP", "adv raw", "N=6 T=11")
    b64.check(O.ret_buf, (ret.T, Br.T), "TRPOBufferNP", "ret", "N=6 T=11")
    y, By = b64.normalize64(adv.T, Ba.T, 1)
    b64.check(O.get()['adv'], (y.reshape(-1), By.reshape(-1)), "TRPOBufferNP", "adv", "N=6 T=11")


# ---------------------------------------------------------------------------------------------------------------------
# the test can fail: each planted mistake, built on the reference side, lies outside FACTOR x bound of the right answer
# ---------------------------------------------------------------------------------------------------------------------
def _noticed(got, wrong, keys):
    """the largest error / bound of the right batch `got` against the wrong reference over `keys`, 0 if within bound"""
    return max(b64.outside(got[k], wrong[k]) for k in keys)


MISTAKES = [
    ("a bootstrap for a finished env", dict(boot_finished=True), ('adv', 'ret'), FORMS),
    ("no bootstrap for an unfinished env", dict(no_boot=True), ('adv', 'ret'), FORMS),
    ("lambda missing at one step", dict(drop_lam_at=1), ('adv',), FORMS),
    ("the mean over L instead of T", dict(mean_over_L=True), ('adv',), FORMS),
    ("the sample deviation", dict(ddof=1), ('adv',), FORMS),
    ("the cost channel: a bootstrap for a finished env", dict(boot_finished=True), ('adc', 'cost_ret'), ('cost',)),
    ("the cost channel: the mean over L", dict(mean_over_L=True), ('adc',), ('cost',)),
    ("targetc carries gamma qc across the end of a path", dict(targetc_across=True), ('targetc',), ('usl',)),
]


@pytest.mark.parametrize("what,kw,keys,forms", MISTAKES, ids=[m[0] for m in MISTAKES])
def test_planted_mistakes_in_the_values_are_noticed(what, kw, keys, forms):
    for N in (255, 256, 257, 513):
        for form in forms:
            g, got = _partition(N, form)
            assert _noticed(got, b64.episode64(g, GAMMA, LAM), keys) == 0      # the right reference passes
            f = _noticed(got, b64.episode64(g, GAMMA, LAM, **kw), keys)
            print(f"{what}: N={N} {form}: outside the bound by a factor {f / FACTOR:.3g}")
            assert f > FACTOR, (what, N, form)


def test_a_shifted_offset_table_is_noticed():
    """the offsets of the envs from the second block of 256 on taken from the env before: every gathered column and
    every computed one changes, because the lengths on either side of the boundary differ"""
    for N, form in ((257, 'plain'), (513, 'safelayer'), (513, 'usl')):
        g, got = _partition(N, form)
        wrong = b64.episode64(g, GAMMA, LAM, shift_from=1)
        for k in ('obs', 'act', 'mu', 'logp'):
            assert (got[k] != wrong[k]).any(), (N, form, k)
            assert (got[k][:256] == wrong[k][:256]).all()                    # (the first block's rows stand)
        assert _noticed(got, wrong, ('adv', 'ret')) > FACTOR
    name, kw = b64.episode_cases()[0]
    g = b64.episode_inputs(**kw)
    got = _host_episode(g)
    for shift in (1, 256):                                                     # the second block; the second turn over bsum
        wrong = b64.episode64(g, GAMMA, LAM, shift_from=shift)
        assert (got['obs'] != wrong['obs']).any() and _noticed(got, wrong, ('ret', 'targetc')) > FACTOR


def test_an_unclamped_first_done_is_noticed():
    for N in PARTITION_N[1:]:
        g, got = _partition(N, 'plain')
        assert (g['first_done'] > g['rew'].shape[0]).any()
        assert b64.episode64(g, GAMMA, LAM, unclamped=True)['n_valid'] > got['n_valid'] == b64.episode64(g, GAMMA, LAM)['n_valid']


def test_a_one_pass_variance_is_noticed_on_the_mean_100_rows():
    """E[x^2] - mean^2 is a mistake of float32 arithmetic, not of the formula, so it is planted in float32 and compared
    with the right reference: on rows with mean 100 and deviation 1 it lies outside the bound, while the two-pass
    float32 order (the kernels') lies within it on the same rows.  On N(0, 1) rows the two cannot be told apart, which
    is why the mean-100 rows are part of the input set."""
    worst = {}
    for T in b64.NORM_T:
        x = b64.norm_rows(5, T, True)
        ref = b64.normalize64(x, np.zeros_like(x, np.float64), 1)
        mean = x.sum(1, keepdims=True, dtype=np.float32) / np.float32(T)
        d = x - mean
        two_pass = d / np.sqrt((d * d).sum(1, keepdims=True, dtype=np.float32) / np.float32(T))
        assert two_pass.dtype == np.float32 and b64.outside(two_pass, ref) == 0
        worst[T] = b64.outside(b64.normalize_one_pass_f32(x), ref)
        print(f"one-pass variance, mean-100 rows, T={T}: error / bound = {worst[T]:.3g}")
        x0 = b64.norm_rows(5, T, False)
        if T > 2:
            assert b64.outside(b64.normalize_one_pass_f32(x0), b64.normalize64(x0, np.zeros_like(x0, np.float64), 1)) == 0
    # the bound's mean term grows with T, so the short rows are where this mistake must show
    assert all(worst[T] > FACTOR for T in (2, 63, 64, 65)), worst
