"""The host front end of the closed-loop rollouts without a device (guardx_amd/_closed_loop.py and what Engine builds on
it): pack_actor_critic's layout, sizes and refusals, and the first-done bookkeeping's hand-off (Book, State)."""
import ctypes as C

import pytest

from test_policy64 import make_ac


def _mlp(widths, act=None, out_act=None):
    """Linear(widths[0], widths[1]), act, ..., Linear(widths[-2], widths[-1]) [, out_act]"""
    import torch.nn as nn
    act = act or nn.Tanh
    mods = []
    for i, (a, b) in enumerate(zip(widths[:-1], widths[1:])):
        mods += [nn.Linear(a, b)] + ([act()] if i < len(widths) - 2 else [])
    return nn.Sequential(*mods, *([out_act()] if out_act else []))


@pytest.mark.parametrize("D,A,h", [(43, 2, 64), (70, 10, 256)])
def test_pack_actor_critic_is_the_concatenation(D, A, h):
    """W1 b1 W2 b2 W3 b3 of mu_net, then of v_net, then log_std; numel() is policy_floats is Engine._policy_floats"""
    import torch
    from guardx_amd import Engine
    from guardx_amd._closed_loop import policy_floats
    ac = make_ac(D, A, h, seed=D)
    want = torch.cat([t.detach().reshape(-1) for net in (ac.pi.mu_net, ac.v.v_net) for m in net
                      if isinstance(m, torch.nn.Linear) for t in (m.weight, m.bias)] + [ac.pi.log_std])
    got = Engine.pack_actor_critic(ac)
    assert got.dtype == torch.float32 and torch.equal(got, want)
    assert torch.equal(Engine.pack_actor_critic(mu_net=ac.pi.mu_net, v_net=ac.v.v_net, log_std=ac.pi.log_std), want)
    assert got.numel() == policy_floats(D, A, h) == Engine._policy_floats(D, A, h)


def _refusals():
    import torch.nn as nn
    pair = lambda *a, **k: (_mlp(*a, **k), None)    # noqa: E731 (None: the critic of the actor's shape)
    return {
        "one hidden layer": (*pair([43, 64, 2]), 2, "two hidden layers"),
        "ReLU": (*pair([43, 64, 64, 2], act=nn.ReLU), 2, "Tanh"),
        "an output activation": (*pair([43, 64, 64, 2], out_act=nn.Tanh), 2, "linear output"),
        "unequal hidden widths": (*pair([43, 64, 32, 2]), 2, "equal width"),
        "width 96": (*pair([43, 96, 96, 2]), 2, r"\(64, 128, 192, 256\)"),
        "actor and critic of different widths": (_mlp([43, 64, 64, 2]), _mlp([43, 128, 128, 1]), 2, "same for actor and critic"),
        "different input widths": (_mlp([43, 64, 64, 2]), _mlp([44, 64, 64, 1]), 2, "same observation width"),
        "a two-output critic": (_mlp([43, 64, 64, 2]), _mlp([43, 64, 64, 2]), 2, "critic with one output"),
        "a wrong log_std length": (_mlp([43, 64, 64, 2]), _mlp([43, 64, 64, 1]), 3, "log_std has 3"),
    }


@pytest.mark.parametrize("case", ["one hidden layer", "ReLU", "an output activation", "unequal hidden widths", "width 96",
                                  "actor and critic of different widths", "different input widths", "a two-output critic",
                                  "a wrong log_std length"])
def test_pack_actor_critic_refuses(case):
    """what the kernels would evaluate differently: NotImplementedError, the cause named"""
    import torch
    from guardx_amd import Engine
    mu_net, v_net, n_log_std, cause = _refusals()[case]
    if v_net is None:          # the same fault in the critic, with the one output a critic has
        mods = list(mu_net)
        last = max(i for i, m in enumerate(mods) if isinstance(m, torch.nn.Linear))
        mods[last] = torch.nn.Linear(mods[last].in_features, 1)
        v_net = torch.nn.Sequential(*mods)
    with pytest.raises(NotImplementedError, match=cause):
        Engine.pack_actor_critic(mu_net=mu_net, v_net=v_net, log_std=torch.zeros(n_log_std))


def test_policy_hidden_is_the_critics():
    from guardx_amd import Engine, critic
    assert Engine.POLICY_HIDDEN == critic.HIDDEN == (64, 128, 192, 256)


class _Env:
    """what Book and State read of an engine"""
    env_num, device = 5, 'cpu'

    def _out_slab(self, k):
        return ("slab", k)


def test_book_and_state_hand_off():
    """reset_book() is a no-op before the first episode call and zeroes ints, sums and t_base after it; c_struct() carries
    the four pointers and t_base"""
    import torch
    from guardx_amd import _closed_loop as cl
    env = _Env()
    st = cl.State(env)
    assert st.slab == ("slab", 1) and st.steps == 0 and st.book is None
    st.reset_book()
    st.reset()
    assert st.book is None and st.steps == 0
    book = st.book = cl.Book(env)
    assert book.ints.shape == (2, 5) and book.ints.dtype == torch.int32 and not book.ints.any()
    assert book.sums.shape == (2, 5) and book.sums.dtype == torch.float32 and not book.sums.any() and book.t_base == 0
    book.ints.fill_(3)
    book.sums.fill_(1.5)
    book.t_base = st.steps = 7
    b = book.c_struct()
    assert b.struct_size == C.sizeof(b) and b.t_base == 7
    assert (b.d_first_done, b.d_ep_len) == (book.ints[0].data_ptr(), book.ints[1].data_ptr())
    assert (b.d_ep_ret, b.d_ep_cost) == (book.sums[0].data_ptr(), book.sums[1].data_ptr())
    assert len({b.d_first_done, b.d_ep_len, b.d_ep_ret, b.d_ep_cost}) == 4
    st.reset()                                                    # the path's own state, not the book
    assert book.t_base == 7 and int(book.ints.sum()) == 30
    st.reset_book()
    assert st.book is book and not book.ints.any() and not book.sums.any() and book.t_base == 0
    assert st.steps == 7                                          # the noise counter is not the book's
    assert book.c_struct().t_base == 0
