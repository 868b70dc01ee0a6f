"""What rollout_policy and rollout_episode refuse before anything is launched, the hand-off of the episode path's state
between calls, rollout_policy and reset(), and the tail's rule through episode.tail_probe.  Point, env_num = 17 (one
env past the 16-env workgroup granule), T = 1."""
import numpy as np
import pytest

from test_policy64 import make_ac, critic_net
from test_gpu_statewise import _cfg, _engine, _softplus_critic, SEED

pytestmark = pytest.mark.gpu

N = 17


@pytest.fixture(scope="module")
def world():
    """an engine that was never reset, and for its D and A: params, a cost critic, and the cost critics that do not fit"""
    import torch
    from guardx_amd import Engine
    E = _engine(_cfg("point", N))
    D, A = E.obs_flat_size, E.action_space.shape[0]
    w = dict(E=E, D=D, A=A, p=Engine.pack_actor_critic(make_ac(D, A, 64, seed=1)).cuda(),
             vcp=Engine.pack_critic(critic_net(D, 64, seed=2), device='cuda'),
             softplus=Engine.pack_critic(_softplus_critic(D, 64, seed=3)[0], device='cuda', output='softplus'),
             short=torch.zeros(1234, device='cuda'),
             wider=Engine.pack_critic(critic_net(D + 1, 64, seed=4), device='cuda'))
    yield w
    E.close()


# (what is wrong, the keyword arguments that make it so, the class and the text for rollout_policy, for rollout_episode)
REFUSED = [
    ("params of 1234 floats", dict(params='short'),
     (ValueError, "params has 1234 floats; expected one of"), (ValueError, "params has 1234 floats; expected one of")),
    ("obs0 of 16 rows", dict(obs0=16),
     (AssertionError, None),(ValueError, r"obs0 has shape \(16, 43\); expected \(17, 43\)")),
    ("a softplus cost critic", dict(cost_critic='softplus'),
     (ValueError, "rollout_policy evaluates the cost critic with a linear output; cost_critic was packed with output='softplus'"),
     (ValueError, "rollout_episode evaluates the cost critic with a linear output; cost_critic was packed with output='softplus'")),
    ("a cost critic of 1234 floats", dict(cost_critic='short'),
     (ValueError, "cost_critic has 1234 floats; expected one of"), (ValueError, "cost_critic has 1234 floats; expected one of")),
    ("a cost critic for D + 1", dict(cost_critic='wider'),
     (ValueError, "cost_critic has 7105 floats; expected one of"), (ValueError, "cost_critic has 7105 floats; expected one of")),
]


def _call(w, which, params='p', obs0=None, cost_critic=None):
    import torch
    if obs0 is not None:
        obs0 = torch.zeros(obs0, w['D'], device='cuda')
    return getattr(w['E'], which)(w[params], 1, obs0=obs0, noise_seed=SEED, cost_critic=w.get(cost_critic))


def test_refusals_then_the_state_hand_off(world):
    """every refusal with the class and the text it has always had; none of them leaves anything behind: the calls after
    them count from zero.  rollout_policy neither reads nor advances the episode path's counters, reset() clears the
    bookkeeping and leaves the noise counter."""
    E, p = world['E'], world['p']
    for which in ("rollout_policy", "rollout_episode"):
        with pytest.raises(RuntimeError, match=which + r"\(\) before reset\(\)"):
            _call(world, which)
    E.reset()
    for what, kw, *expected in REFUSED:
        for which, (cls, text) in zip(("rollout_policy", "rollout_episode"), expected):
            with pytest.raises(cls, match=text) as info:
                _call(world, which, **kw)
            assert type(info.value) is cls, (what, which)
    assert E._episode is None                                    # nothing was made for a refused call
    a = E.rollout_episode(p, 2, noise_seed=SEED)
    b = E.rollout_episode(p, 1, noise_seed=SEED)
    st = E._episode
    assert (a['t0'], b['t0']) == (0, 2) and (st.book.t_base, st.steps) == (3, 3)
    ints, sums = st.book.ints.clone(), st.book.sums.clone()
    assert (ints[1] == 3).any()                                  # ep_len: the bookkeeping is not a zero that hides a reset
    E.rollout_policy(p, 1, noise_seed=SEED)
    assert (st.book.t_base, st.steps) == (3, 3) and E._episode is st
    assert (st.book.ints == ints).all() and (st.book.sums == sums).all()
    E.reset()
    assert st.book.t_base == 0 and st.steps == 3
    assert int(st.book.ints.abs().sum()) == 0 and float(st.book.sums.abs().sum()) == 0
    c = E.rollout_episode(p, 1, noise_seed=SEED)
    assert c['t0'] == 0 and (st.book.t_base, st.steps) == (1, 4)
    assert (c['ep_len'] == 1).all()


@pytest.mark.parametrize("with_cost", [False, True])
def test_the_tail_probe_on_a_row_with_a_nan(world, with_cost):
    """17 rows, one of them with a NaN: val_last (and vc_last with a cost critic) is 0 there, obs_last the rows' bits"""
    import torch
    from guardx_amd.episode import tail_probe
    rows = np.random.default_rng(5).normal(size=(N, world['D'])).astype(np.float32)
    rows[16, 3] = np.nan
    got = tail_probe(world['p'], torch.from_numpy(rows).cuda(), world['A'], cost_critic=world['vcp'] if with_cost else None)
    assert set(got) == {'obs_last', 'val_last'} | ({'vc_last'} if with_cost else set())
    np.testing.assert_array_equal(got['obs_last'].cpu().numpy().view(np.uint32), rows.view(np.uint32))
    for k in set(got) - {'obs_last'}:
        v = got[k].cpu().numpy()
        assert v.shape == (N,) and v.view(np.uint32)[16] == 0 and (v[:16] != 0).all(), k
