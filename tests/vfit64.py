"""The value fit of include/guardx_vfit.h in numpy float64, for any hidden width: the gradient of the learners' MSE loss in
closed form (grad64), torch's single-tensor Adam (adam64) and the learners' loop around both (fit64) -- the oracle of
tests/test_vfit64.py (which checks it against float64 autograd and torch.optim.Adam), tests/test_reference_vfit.py and
tests/test_gpu_vfit.py.  Also the learners' own method (autograd and torch.optim.Adam in the precision of the critic it is
given), a critic declared the way the learners declare theirs, and the cases the CPU and the GPU tests share.

Vectors are in the order of critic.parameters(): W1[h][D], b1[h], W2[h][h], b2[h], W3[1][h], b3[1]."""
import functools

import numpy as np

H = 64
LR, BETAS, EPS = 1e-3, (0.9, 0.999), 1e-8        # the learners' vf_lr and torch.optim.Adam's defaults
BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")
ALLOWED = 4.0                                    # x the learners' float32 error: the project's allowance
MISTAKES = ("no_bias_correction", "eps_inside_sqrt", "step_restarts", "no_tanh_slope", "no_two_over_b")


def param_count(D, h=H):
    return h * D + h + h * h + h + h + 1


def _shapes(D, h):
    return ((h, D), (h,), (h, h), (h,), (1, h), (1,))


def unpack(v, D, h=H):
    """(W1, b1, W2, b2, W3, b3) views of the flat vector v"""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (param_count(D, h),)
    out, at = [], 0
    for shape in _shapes(D, h):
        n = int(np.prod(shape))
        out.append(v[at:at + n].reshape(shape))
        at += n
    return out


def pack(parts):
    return np.concatenate([np.ravel(p) for p in parts])


def block_slices(D, h=H):
    slices, at = {}, 0
    for name, shape in zip(BLOCKS, _shapes(D, h)):
        n = int(np.prod(shape))
        slices[name] = slice(at, at + n)
        at += n
    assert at == param_count(D, h)
    return slices


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


def rel_err(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def pooled(errors):
    """the root-mean-square of several errors"""
    e = np.asarray(errors, dtype=np.float64)
    return float(np.sqrt(np.mean(e * e)))


# ---------------------------------------------------------------------------------------------------------------------
# the statement of include/guardx_vfit.h
# ---------------------------------------------------------------------------------------------------------------------
def grad64(theta, obs, ret, h=H, mistake=None):
    """-> (g (P,), loss): loss = mean((v(obs) - ret)^2) and its gradient.  `mistake`: a planted one (MISTAKES)"""
    o, r = np.asarray(obs, dtype=np.float64), np.asarray(ret, dtype=np.float64)
    B, D = o.shape
    assert r.shape == (B,)
    W1, b1, W2, b2, W3, b3 = unpack(theta, D, h)
    h1 = np.tanh(o @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    e = (h2 @ W3.T + b3)[:, 0] - r
    loss = float(np.mean(e * e))
    dval = (e if mistake == "no_two_over_b" else 2.0 * e / B)[:, None]
    s2 = 1.0 if mistake == "no_tanh_slope" else 1.0 - h2 * h2
    dW3, db3 = dval.T @ h2, dval.sum(0)
    dz2 = (dval @ W3) * s2
    dW2, db2 = dz2.T @ h1, dz2.sum(0)
    dz1 = (dz2 @ W2) * (1.0 - h1 * h1)
    dW1, db1 = dz1.T @ o, dz1.sum(0)
    return pack((dW1, db1, dW2, db2, dW3, db3)), loss


def adam64(theta, m, v, g, t, lr=LR, betas=BETAS, eps=EPS, store=None, mistake=None):
    """one step of torch's single-tensor Adam, t counted from 1 -> (theta, m, v).  Every operation in float64, in the
    header's order; `store`: a dtype each result is rounded to once (the header: float32), None: kept in float64"""
    d = np.float64
    theta, m, v, g = (np.asarray(x).astype(d) for x in (theta, m, v, g))
    b1, b2 = betas
    M = b1 * m + (1.0 - b1) * g
    V = b2 * v + (1.0 - b2) * (g * g)
    c1, c2 = (1.0, 1.0) if mistake == "no_bias_correction" else (1.0 - b1 ** t, 1.0 - b2 ** t)
    if mistake == "eps_inside_sqrt":
        den = np.sqrt(V / c2 + eps)
    else:
        den = np.sqrt(V) / np.sqrt(c2) + eps
    T = theta - (lr / c1) * (M / den)
    if store is not None:
        T, M, V = (x.astype(store) for x in (T, M, V))
    return T, M, V


def new_state(P):
    return dict(m=np.zeros(P), v=np.zeros(P), step=0)


def fit64(theta, obs, ret, iters, state=None, h=H, lr=LR, betas=BETAS, eps=EPS, mistake=None):
    """The learners' loop in float64 -> (thetas, losses, state): thetas[k] the parameters after k steps (iters + 1
    entries, thetas[0] = theta), losses[i] the loss before step i, state = dict(m, v, step) to hand to the next call (a
    new optimizer when None).  `mistake`: a planted one (MISTAKES)"""
    theta = np.asarray(theta, dtype=np.float64)
    st = dict(state) if state is not None else new_state(theta.size)
    if mistake == "step_restarts":
        st["step"] = 0
    thetas, losses = [theta], []
    for _ in range(iters):
        g, loss = grad64(theta, obs, ret, h, mistake=mistake)
        st["step"] += 1
        theta, st["m"], st["v"] = adam64(theta, st["m"], st["v"], g, st["step"], lr, betas, eps, mistake=mistake)
        thetas.append(theta)
        losses.append(loss)
    return thetas, np.array(losses), st


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch)
# ---------------------------------------------------------------------------------------------------------------------
def make_critic(D, h=H, seed=0, dtype=None, scale=1.0, out_act=None):
    """An MLP critic declared as the learners declare theirs (trpo_core.MLPCritic): v_net = Linear/Tanh/Linear/Tanh/Linear/
    Identity, forward squeezes the last axis.  Weights from torch's default initialisation under `seed`, times `scale` (one
    number, or one per layer)."""
    import torch
    nn = torch.nn

    class Critic(nn.Module):
        def __init__(self):
            super().__init__()
            self.v_net = nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, 1),
                                       (out_act or nn.Identity)())

        def forward(self, obs):
            return torch.squeeze(self.v_net(obs), -1)

    torch.manual_seed(seed)
    critic = Critic()
    lin = [m for m in critic.v_net if isinstance(m, nn.Linear)]
    scales = [float(scale)] * len(lin) if np.ndim(scale) == 0 else [float(s) for s in scale]
    assert len(scales) == len(lin)
    with torch.no_grad():
        for m, sc in zip(lin, scales):
            m.weight.mul_(sc)
    return critic.to(dtype) if dtype is not None else critic


def flat(critic):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in critic.parameters()])


def assign_flat(critic, theta):
    import torch
    at = 0
    with torch.no_grad():
        for p in critic.parameters():
            p.copy_(torch.as_tensor(np.asarray(theta[at:at + p.numel()])).view_as(p).to(p.dtype))
            at += p.numel()


def learners_loss(critic, obs, ret):
    """compute_loss_v (trpo.py:375-377)"""
    return ((critic(obs) - ret) ** 2).mean()


def autograd_grad(critic, obs, ret):
    """one zero_grad / backward of the learners' loss, in the dtype of the critic: (g, loss) as numpy"""
    import torch
    loss = learners_loss(critic, obs, ret)
    g = torch.autograd.grad(loss, list(critic.parameters()))
    return torch.cat([x.reshape(-1) for x in g]).numpy(), loss.item()


def learners_loop(critic, obs, ret, iters, optimizer=None, lr=LR):
    """The loop the learners run (trpo.py:434-439), on a copy of nothing: `critic` is updated in place.  -> (thetas,
    losses, optimizer): the flat parameters after 0 .. iters steps, the loss before each step"""
    import torch
    opt = optimizer or torch.optim.Adam(critic.parameters(), lr=lr)
    thetas, losses = [flat(critic).numpy().copy()], []
    for _ in range(iters):
        opt.zero_grad()
        loss = learners_loss(critic, obs, ret)
        loss.backward()
        opt.step()
        losses.append(loss.item())
        thetas.append(flat(critic).numpy().copy())
    return thetas, np.array(losses), opt


# ---------------------------------------------------------------------------------------------------------------------
# regimes: where the critic's units sit on tanh (tests/test_vfit64.py asserts what each name promises)
# ---------------------------------------------------------------------------------------------------------------------
SMALL, SAT = 0.625, 9.0          # gx_vfit.hip:tanh_act switches to tanh_f at 0.625; tanh_f returns 1 above 9
# name -> the scales of W1, W2, W3 over torch's default initialisation (fisher64.REGIMES' scalings of W1, W2), obs = mean + std N(0, 1)
REGIMES = {
    "default": dict(scale=(1.0, 1.0, 1.0), obs=(0.0, 1.0)),
    "trained": dict(scale=(4.0, 3.0, 2.0), obs=(0.5, 1.5)),
    "saturated": dict(scale=(12.0, 8.0, 1.0), obs=(0.0, 1.0)),
}


def problem(regime, D, B, seed=0):
    """-> (critic, obs, ret, theta, facts): the regime's critic (float32, hidden width 64), obs (B, D) and ret = 1 + 2 N(0, 1)
    (B,) float32 tensors, theta the flat float32 vector (numpy), facts = dict(z1, z2): both layers' pre-activations in
    float64"""
    import torch
    r = REGIMES[regime]
    critic = make_critic(D, H, seed=seed, scale=r["scale"])
    gen = torch.Generator().manual_seed(100 + seed)
    obs = torch.randn(B, D, generator=gen)
    ret = (1.0 + 2.0 * torch.randn(B, generator=gen)).contiguous()
    mean, std = r["obs"]
    if (mean, std) != (0.0, 1.0):
        obs = (mean + std * obs).contiguous()
    theta = flat(critic).numpy()
    W1, b1, W2, b2, _, _ = unpack(theta, D, H)
    z1 = obs.numpy().astype(np.float64) @ W1.T + b1
    z2 = np.tanh(z1) @ W2.T + b2
    return critic, obs, ret, theta, dict(z1=z1, z2=z2)


# ---------------------------------------------------------------------------------------------------------------------
# cases shared by tests/test_vfit64.py (CPU) and tests/test_gpu_vfit.py: computed once per process, never written to
# ---------------------------------------------------------------------------------------------------------------------
GRAD_SEEDS = (0, 1, 2)
GRAD_ROWS = (1, 63, 64, 65, 257, 4099)
GRAD_WIDTHS = (43, 44, 64)
EDGE_WIDTHS = (1, 16, 17, 32, 65, 72, 73, 96, 97, 128)      # the first-layer instantiations of gx_vfit.hip at their edges
EDGE_ROWS = 130
FIT_SHAPES = ((43, 257), (64, 130))                         # D, B
FIT_SEEDS = {(43, 257): (1, 2, 3, 4), (64, 130): (0, 1, 2, 3)}   # tests/test_vfit64.py: test_the_seeds_are_well_conditioned
FIT_KS = (1, 2, 3, 10)


def grad_errors(g, loss, want_g, want_loss, D):
    """(whole-vector relative L2, {block: relative L2}, relative error of the loss)"""
    return rel_l2(g, want_g), {k: rel_l2(g[s], want_g[s]) for k, s in block_slices(D).items()}, rel_err(loss, want_loss)


def pool_grads(errs):
    return (pooled([e[0] for e in errs]), {k: pooled([e[1][k] for e in errs]) for k in BLOCKS}, pooled([e[2] for e in errs]))


@functools.lru_cache(maxsize=None)
def gradient_case(regime, D, B, seed):
    """dict(critic, obs, ret, theta, g (P,) float64, loss, yard): yard = grad_errors of the learners' float32 autograd on
    the same inputs"""
    critic, obs, ret, theta, _ = problem(regime, D, B, seed)
    g, loss = grad64(theta, obs.numpy(), ret.numpy())
    ag, al = autograd_grad(critic, obs, ret)
    g.setflags(write=False)
    return dict(critic=critic, obs=obs, ret=ret, theta=theta, g=g, loss=loss, yard=grad_errors(ag, al, g, loss, D))


def fit_errors(thetas, losses, ref):
    """{("theta", k): relative L2 of the displacement theta_k - theta_0, ("loss", k): the largest relative error of the
    first k entries of the loss trace} against fit_case()'s float64 ones, k in FIT_KS"""
    errs = {}
    for k in FIT_KS:
        errs["theta", k] = rel_l2(np.asarray(thetas[k], np.float64) - ref["theta"], ref["thetas"][k] - ref["theta"])
        errs["loss", k] = max(rel_err(losses[i], ref["losses"][i]) for i in range(k))
    return errs


def pool_fits(errs):
    return {key: pooled([e[key] for e in errs]) for key in errs[0]}


def float32_loop_errors(D, B, seed, order=None):
    """fit_errors of the learners' float32 loop on problem("default", D, B, seed), its rows taken in `order`"""
    import copy
    c = fit_case(D, B, seed)
    obs, ret = (c["obs"], c["ret"]) if order is None else (c["obs"][order].contiguous(), c["ret"][order].contiguous())
    thetas, losses, _ = learners_loop(copy.deepcopy(c["critic"]), obs, ret, max(FIT_KS))
    return fit_errors(thetas, losses, c)


@functools.lru_cache(maxsize=None)
def fit_case(D, B, seed):
    """dict(critic, obs, ret, theta (float32), thetas / losses / states: fit64's over max(FIT_KS) steps): the default
    regime.  states[k] is the optimizer's state after k steps"""
    critic, obs, ret, theta, _ = problem("default", D, B, seed)
    thetas, losses, state, states = [theta.astype(np.float64)], [], None, [new_state(theta.size)]
    for _ in range(max(FIT_KS)):                                  # step by step, so that every state is on record
        ts, ls, state = fit64(thetas[-1], obs.numpy(), ret.numpy(), 1, state=state)
        thetas.append(ts[1])
        losses.append(ls[0])
        states.append(state)
    return dict(critic=critic, obs=obs, ret=ret, theta=theta, thetas=thetas, losses=np.array(losses), states=states)


@functools.lru_cache(maxsize=None)
def fit_yardstick(D, B):
    """the learners' float32 loop's fit_errors, pooled over FIT_SEEDS"""
    return pool_fits([float32_loop_errors(D, B, s) for s in FIT_SEEDS[D, B]])
