"""guardx_amd.epstats on the device (libguardx_epstats.so: the scan, the ordered compaction, the 256-slot float64 moments)
against its own host-tensor path bit for bit -- which tests/test_epstats_host.py holds to the restatement of the learner
loop -- on synthetic tensors at the wave, row-block and slot edges, and end to end behind rollout_policy."""
import numpy as np
import pytest
import torch

from test_epstats_host import STAT_KEYS, make, tt

pytestmark = pytest.mark.gpu

FIELDS = ('n', 'S', 'mean', 'Q', 'std', 'min', 'max')
ARRAYS = ('env', 't_end', 'ep_ret', 'ep_cost', 'ep_cost_ret', 'ep_len')


def raw(x):
    """the bits of a tensor, whatever its type, as a list (every NaN as one NaN: sign and payload of a NaN say nothing)"""
    x = x.detach().cpu().contiguous().reshape(-1)
    if x.dtype == torch.float64:
        x = torch.where(torch.isnan(x), torch.full_like(x, float('nan')), x)
    return x.view(torch.int64 if x.dtype == torch.float64 else torch.int32).tolist()


def assert_same(dev, host, what):
    assert set(dev) == set(host), what
    for k in host:
        if k in STAT_KEYS:
            for f in FIELDS:
                assert dev[k][f].is_cuda and dev[k][f].dtype == torch.float64 and raw(dev[k][f]) == raw(host[k][f]), (what, k, f)
        elif k == 'carry':
            assert dev[k]['t'] == host[k]['t'] and dev[k]['max_ep_len'] == host[k]['max_ep_len']
            assert raw(dev[k]['acc']) == raw(host[k]['acc']) and raw(dev[k]['len']) == raw(host[k]['len']), what
        else:
            assert dev[k].is_cuda and dev[k].dtype == host[k].dtype and tuple(dev[k].shape) == tuple(host[k].shape), (what, k)
            assert raw(dev[k]) == raw(host[k]), (what, k)


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("T", [1, 2, 7, 33])
def test_device_equals_host_bit_for_bit(N, T):
    """every done density; with and without gamma, val and the episode arrays, and with the time-out step in the call and
    past it; T = 33 is two row blocks of the scan and one tail row"""
    from guardx_amd.epstats import episode_stats
    for i, density in enumerate((0.0, 0.02, 0.5, 1.0)):
        d = make(7 * N + T + i, T, N, density, values=(1.0, 1.0, 1.0, 2.0, 0.5))
        host = tt(d, 'rew', 'cost', 'done', 'val')
        dev = [x.cuda() for x in host]
        for j, kw in enumerate((dict(), dict(gamma=0.99, episodes=True), dict(gamma=0.9, max_ep_len=T + 3, episodes=True),
                                dict(episodes=True))):
            use_val = (i + j) % 2 == 0
            want = episode_stats(*host[:3], val=host[3] if use_val else None, **kw)
            got = episode_stats(*dev[:3], val=dev[3] if use_val else None, **kw)
            assert_same(got, want, (density, kw, use_val))
        if (N, T, density) == (130, 33, 0.5):
            assert int(want['n_episodes']) > 4 * 256          # several entries per slot, the whole tree in use


def test_chunks_with_carry_and_a_planted_nan_on_the_device():
    from guardx_amd.epstats import episode_stats
    T, N, k = 33, 130, 17
    d = make(1, T, N, 0.1)
    d['rew'][5, 70] = np.nan
    d['val'][20, 3] = np.nan
    host = tt(d, 'rew', 'cost', 'done', 'val')
    dev = [x.cuda() for x in host]
    whole = episode_stats(*host[:3], val=host[3], gamma=0.99, episodes=True)
    assert_same(episode_stats(*dev[:3], val=dev[3], gamma=0.99, episodes=True), whole, "whole")
    assert all(bool(torch.isnan(whole[key][f])) for key in ('EpRet', 'MaxEpLenRet', 'VVals') for f in ('mean', 'std', 'min', 'max'))
    first = episode_stats(*[x[:k] for x in dev[:3]], gamma=0.99, max_ep_len=T, episodes=True)
    second = episode_stats(*[x[k:] for x in dev[:3]], gamma=0.99, carry=first['carry'], episodes=True)
    h1 = episode_stats(*[x[:k] for x in host[:3]], gamma=0.99, max_ep_len=T, episodes=True)
    assert_same(first, h1, "first chunk")
    assert_same(second, episode_stats(*[x[k:] for x in host[:3]], gamma=0.99, carry=h1['carry'], episodes=True), "second chunk")
    for key in ARRAYS:
        assert raw(torch.cat([first[key], second[key]])) == raw(whole[key]), key
    assert raw(second['MaxEpLenRet']['S']) == raw(whole['MaxEpLenRet']['S'])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 130, 700])
def test_one_episode_form_on_the_device(N):
    from guardx_amd.epstats import episode_stats
    rng = np.random.default_rng(N)
    for T in (1, 2, 7, 33):
        out = dict(ep_ret=torch.from_numpy(rng.normal(size=N).astype(np.float32)), ep_cost=torch.from_numpy(rng.random(N).astype(np.float32)),
                   first_done=torch.from_numpy(rng.integers(0, T + 1, N).astype(np.int32)), rew=torch.zeros(T, N), t0=3)
        want = episode_stats(out)
        got = episode_stats({k: v.cuda() if torch.is_tensor(v) else v for k, v in out.items()})
        assert_same(got, want, T)


def test_behind_rollout_policy_without_a_synchronisation(monkeypatch):
    """Goal_Point_8Hazards as smoke() runs it (wide goal: resets fire inside the rollout): episode_stats(out) on the device
    is the host path on `out` moved to the host, and the call takes no path that waits for the device"""
    from guardx_amd import Engine
    from guardx_amd.epstats import constraint_value, episode_stats
    from helpers import task_config
    from test_policy64 import make_ac
    T = 50
    E = Engine(task_config(128, seed=0, num_steps=T, goal_size=2.8, device_id=0), n_candidates=20000)
    E.reset()
    p = Engine.pack_actor_critic(make_ac(E.obs_flat_size, E.action_space.shape[0], 64, seed=3)).cuda()
    out = E.rollout_policy(p, T, noise_seed=(1, 2))
    episode_stats(out, gamma=0.99)                                   # loads the library, uploads the discount table
    torch.cuda.synchronize()

    def waits(*a, **k):
        raise AssertionError("episode_stats waited for the device")
    with monkeypatch.context() as m:
        for name in ('item', 'cpu', 'tolist', 'numpy', '__bool__', '__int__', '__float__'):
            m.setattr(torch.Tensor, name, waits)
        m.setattr(torch.cuda, 'synchronize', waits)
        m.setattr(torch.cuda.Stream, 'synchronize', waits)
        got = Engine.episode_stats(out, gamma=0.99)
        c = constraint_value(got, 25.0)
    want = episode_stats({k: v.cpu() for k, v in out.items() if torch.is_tensor(v)}, gamma=0.99)
    assert_same(got, want, "rollout_policy")
    assert int(got['n_episodes']) > 0 and 'VVals' in got and 'MaxEpLenRet' in got
    assert float(got['EpLen']['min']) < T                                    # resets fired inside the rollout
    assert float(c) == float(constraint_value(want, 25.0))
    E.close()
