"""The safety-critic fit of include/guardx_cfit.h in numpy float64: the row-weighted squared loss under the three heads and its
gradient in closed form (grad64), and the learners' loop around it with vfit64's Adam (fit64) -- the oracle of
tests/test_cfit64.py (which checks it against float64 autograd of the learners' own expressions), tests/test_reference_cfit.py
and tests/test_gpu_cfit.py.  Also the modules declared the way the learners declare theirs, the learners' expressions
themselves (the down-sampled forms with supplied indices among them) and the cases the CPU and the GPU tests share.

Vectors are in the order of the module's parameters(): W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]."""
import functools

import numpy as np

import vfit64 as v64

H = 64
LR, BETAS, EPS = 1e-3, v64.BETAS, v64.EPS
BLOCKS = v64.BLOCKS
ALLOWED = 4.0                                    # x the learners' float32 error: the project's allowance
HEADS = ("identity", "softplus", "dot")
MISTAKES = ("no_fprime", "over_b", "weight_after_sqrt", "no_offset", "act_for_act_safe")
rel_l2, rel_err, pooled = v64.rel_l2, v64.rel_err, v64.pooled
adam64, new_state = v64.adam64, v64.new_state


def param_count(D, A=1, h=H):
    return h * D + h + h * h + h + A * h + A


def _shapes(D, A, h):
    return ((h, D), (h,), (h, h), (h,), (A, h), (A,))


def unpack(v, D, A=1, h=H):
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (param_count(D, A, h),)
    out, at = [], 0
    for shape in _shapes(D, A, h):
        n = int(np.prod(shape))
        out.append(v[at:at + n].reshape(shape))
        at += n
    return out


def pack(parts):
    return np.concatenate([np.ravel(p) for p in parts])


def block_slices(D, A=1, h=H):
    slices, at = {}, 0
    for name, shape in zip(BLOCKS, _shapes(D, A, h)):
        n = int(np.prod(shape))
        slices[name] = slice(at, at + n)
        at += n
    return slices


def softplus64(z):
    """torch's Softplus(beta=1, threshold=20)"""
    z = np.asarray(z, dtype=np.float64)
    return np.where(z > 20.0, z, np.log1p(np.exp(np.minimum(z, 20.0))))


def softplus_grad64(z):
    """its derivative as torch's backward takes it: 1 past the threshold, the sigmoid below"""
    z = np.asarray(z, dtype=np.float64)
    return np.where(z > 20.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(z, 20.0))))


# ---------------------------------------------------------------------------------------------------------------------
# the statement of include/guardx_cfit.h
# ---------------------------------------------------------------------------------------------------------------------
def forward64(head, theta, x, act=None, offset=None, h=H):
    """-> (f (B,), z (B, A), h1, h2)"""
    x = np.asarray(x, dtype=np.float64)
    D = x.shape[1]
    A = 1 if head != "dot" else np.asarray(act).shape[1]
    W1, b1, W2, b2, W3, b3 = unpack(theta, D, A, h)
    h1 = np.tanh(x @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    z = h2 @ W3.T + b3
    if head == "identity":
        f = z[:, 0]
    elif head == "softplus":
        f = softplus64(z[:, 0])
    else:
        f = (z * np.asarray(act, dtype=np.float64)).sum(1) + (0.0 if offset is None else np.asarray(offset, dtype=np.float64))
    return f, z, h1, h2


def grad64(head, theta, x, y, w=None, act=None, offset=None, h=H, mistake=None, wrong_act=None):
    """-> (g (P,), loss, W): loss = sum_i w_i (f_i - y_i)^2 / W over the rows with w_i != 0, which are selected (the others may
    hold anything), and its gradient.  No live row: NaN, the mean of an empty selection.  `mistake`: a planted one (MISTAKES;
    'act_for_act_safe' takes the action from `wrong_act`)"""
    assert head in HEADS and (mistake is None or mistake in MISTAKES)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    B, D = x.shape
    w = np.ones(B) if w is None else np.asarray(w, dtype=np.float64)
    assert y.shape == (B,) and w.shape == (B,)
    live = w != 0
    A = 1 if head != "dot" else np.asarray(act).shape[1]
    if not live.any():
        return np.full(param_count(D, A, h), np.nan), float("nan"), 0.0
    if mistake == "act_for_act_safe":
        act = wrong_act
    if mistake == "no_offset":
        offset = None
    sel = lambda a: None if a is None else np.asarray(a, dtype=np.float64)[live]     # noqa: E731
    x, y, w, act, offset = x[live], y[live], w[live], sel(act), sel(offset)
    W1, b1, W2, b2, W3, b3 = unpack(theta, D, A, h)
    f, z, h1, h2 = forward64(head, theta, x, act, offset, h)
    e = f - y
    W = float(w.sum())
    den = float(B) if mistake == "over_b" else W
    ww = w * w if mistake == "weight_after_sqrt" else w         # the weight on the residual, not on its square
    loss = float((ww * e * e).sum() / den)
    u = 2.0 * ww * e / den
    if head == "identity":
        dz = u[:, None]
    elif head == "softplus":
        dz = (u * (1.0 if mistake == "no_fprime" else softplus_grad64(z[:, 0])))[:, None]
    else:
        dz = u[:, None] * (1.0 if mistake == "no_fprime" else act)
    dW3, db3 = dz.T @ h2, dz.sum(0)
    dz2 = (dz @ W3) * (1.0 - h2 * h2)
    dW2, db2 = dz2.T @ h1, dz2.sum(0)
    dz1 = (dz2 @ W2) * (1.0 - h1 * h1)
    dW1, db1 = dz1.T @ x, dz1.sum(0)
    return pack((dW1, db1, dW2, db2, dW3, db3)), loss, W


def fit64(head, theta, x, y, iters, weights=None, act=None, offset=None, state=None, h=H, lr=LR, betas=BETAS, eps=EPS):
    """The learners' loop in float64 -> (thetas, losses, Ws, state); weights: None, (B,) or (iters, B) (row i for round i)"""
    theta = np.asarray(theta, dtype=np.float64)
    st = dict(state) if state is not None else new_state(theta.size)
    thetas, losses, Ws = [theta], [], []
    for i in range(iters):
        w = None if weights is None else (weights[i] if np.ndim(weights) == 2 else weights)
        g, loss, W = grad64(head, theta, x, y, w, act, offset, h)
        st["step"] += 1
        theta, st["m"], st["v"] = adam64(theta, st["m"], st["v"], g, st["step"], lr, betas, eps)
        thetas.append(theta)
        losses.append(loss)
        Ws.append(W)
    return thetas, np.array(losses), np.array(Ws), st


def downsample_count(n_pos, n_zero):
    """rows with target == 0 the reference keeps, None where it keeps the whole batch (safelayer.py:400-413)"""
    if n_zero == 0:
        return None
    frac = n_pos / n_zero
    return int(n_zero * frac) if frac < 1.0 else None


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch)
# ---------------------------------------------------------------------------------------------------------------------
def make_module(head, D, A=2, h=H, seed=0, dtype=None, scale=1.0, attr=None):
    """ac.ccritic / ac.vc as the learners declare them: 'softplus' with attr 'c_net' (usl_core.C_Critic, forward on
    cat(obs, act)) or 'v_net' (scpo_core.MLPMaxCostCritic), 'dot' with .g_net (safelayer_core.C_Critic), 'identity' with
    .v_net (trpo_core.MLPCritic).  Weights from torch's default initialisation under `seed`, times `scale` (one number, or
    one per layer)."""
    import torch
    nn = torch.nn
    attr = attr or {"identity": "v_net", "softplus": "c_net", "dot": "g_net"}[head]
    out = 1 if head != "dot" else A
    tail = nn.Softplus if head == "softplus" else nn.Identity

    class Module(nn.Module):
        def __init__(self):
            super().__init__()
            setattr(self, attr, nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, out), tail()))

        def forward(self, x, act=None):
            net = getattr(self, attr)
            if head == "dot":
                g = net(x)
                return torch.flatten(torch.bmm(g.unsqueeze(1), act.unsqueeze(2)))
            return torch.squeeze(net(x), -1)

    torch.manual_seed(seed)
    mod = Module()
    lin = [m for m in getattr(mod, attr) if isinstance(m, nn.Linear)]
    scales = [float(scale)] * 3 if np.ndim(scale) == 0 else [float(s) for s in scale]
    with torch.no_grad():
        for m, sc in zip(lin, scales):
            m.weight.mul_(sc)
    return mod.to(dtype) if dtype is not None else mod


flat, assign_flat = v64.flat, v64.assign_flat


def weighted_loss(mod, head, x, y, w=None, act=None, offset=None):
    """the header's loss as a torch expression"""
    f = mod(x, act) if head == "dot" else mod(x)
    if head == "dot" and offset is not None:
        f = f + offset
    if w is None:
        return ((f - y) ** 2).mean()
    return (w * (f - y) ** 2).sum() / w.sum()


def learners_loss(mod, head, x, y, keep=None, act=None, offset=None):
    """The learners' own lines.  keep None: the plain forms (usl.py:378-383; the `else` branches of the other two).
    keep = (indices of the positive rows' complement to keep, among the rows with y == 0): the down-sampled forms, with
    the random choice supplied -- safelayer.py:384-418 for 'dot' (predictions indexed), scpo.py:419-450 otherwise (inputs
    indexed)."""
    import torch
    import torch.nn.functional as F
    if head == "dot":
        cur = mod(x, act) + offset
        if keep is None:
            return F.mse_loss(cur, y)
        t_zero, c_zero = y[y == 0], cur[y == 0]
        t_pos, c_pos = y[y > 0], cur[y > 0]
        return F.mse_loss(torch.cat((c_pos, c_zero[keep]), dim=0), torch.cat((t_pos, t_zero[keep]), dim=0))
    if keep is None:
        return ((mod(x) - y) ** 2).mean()
    y_pos, x_pos = y[y > 0], x[y > 0]
    y_zero, x_zero = y[y == 0], x[y == 0]
    return ((mod(torch.cat((x_pos, x_zero[keep]), dim=0)) - torch.cat((y_pos, y_zero[keep]), dim=0)) ** 2).mean()


def keep_to_weights(y, keep):
    """the (B,) 0 / 1 weights of a down-sampled batch: the positive rows and the `keep`-th of the rows with y == 0"""
    y = np.asarray(y)
    w = (y > 0).astype(np.float32)
    w[np.flatnonzero(y == 0)[np.asarray(keep)]] = 1.0
    return w


def autograd_grad(loss, mod):
    import torch
    g = torch.autograd.grad(loss, list(mod.parameters()))
    return torch.cat([t.reshape(-1) for t in g]).numpy(), loss.item()


# ---------------------------------------------------------------------------------------------------------------------
# regimes and cases shared by tests/test_cfit64.py (CPU) and tests/test_gpu_cfit.py: computed once, never written to
# ---------------------------------------------------------------------------------------------------------------------
# name -> the scales of W1, W2, W3 over torch's default initialisation, the share of targets that are exactly 0
REGIMES = {
    "default": dict(scale=(1.0, 1.0, 1.0), zeros=0.0),
    "z20": dict(scale=(2.0, 2.0, 60.0), zeros=0.0),             # z = W3 h2 + b3 passes +20 and -20 (tests/test_cfit64.py asserts it)
    "sparse": dict(scale=(1.0, 1.0, 1.0), zeros=0.9),
}
WEIGHTINGS = ("none", "mask", "fractional")
GRAD_SEEDS = (0, 1, 2, 3)
GRAD_ROWS = (1, 63, 64, 65, 257, 4099)
EDGE_WIDTHS = (1, 16, 17, 32, 33, 44, 45, 48, 49, 64, 65, 72, 73, 96, 97, 128)
EDGE_ROWS = 130
DOT_D, DOT_AS = 43, (2, 8, 10, 16)
SOFT_D = 45
FIT_SHAPES = (("softplus", 45, 1, 257), ("dot", 43, 2, 130), ("identity", 64, 1, 257))   # head, D, A, B
FIT_SEEDS = (0, 1, 2, 3)
FIT_ITERS = 10


def make_weights(kind, B, seed):
    """none: None.  mask: 0 / 1 with whole tiles dead (rows 64 .. 127 and every tile from 256 on but its row 5) and one row in
    three elsewhere; at least one row lives.  fractional: uniform in (0.25, 1.75)."""
    if kind == "none":
        return None
    rng = np.random.default_rng(1000 + seed)
    if kind == "fractional":
        return rng.uniform(0.25, 1.75, B).astype(np.float32)
    w = (rng.uniform(size=B) < 1.0 / 3.0).astype(np.float32)
    w[64:128] = 0.0
    w[256:] = 0.0
    w[256 + 5::64] = 1.0                                         # a tile with a single live row
    w[0] = 1.0
    return w


def problem(head, regime, D, A, B, seed=0):
    """-> dict(mod, x, y, act, offset (torch float32; act and offset None off 'dot'), theta (numpy float32))"""
    import torch
    r = REGIMES[regime]
    mod = make_module(head, D, A, seed=seed, scale=r["scale"])
    gen = torch.Generator().manual_seed(200 + seed)
    x = torch.randn(B, D, generator=gen)
    y = torch.randn(B, generator=gen).abs() + 2.0       # above what a fresh network says: the residuals share a sign and the bias
                                                        # gradients are sums without cancellation, so each seed's float32 error is typical
    if r["zeros"]:
        y = torch.where(torch.rand(B, generator=gen) < r["zeros"], torch.zeros(()), y).contiguous()
    act = offset = None
    if head == "dot":
        act = (0.4 + 0.5 * torch.randn(B, A, generator=gen)).clamp(-1.0, 1.0).contiguous()
        offset = (torch.randn(B, generator=gen).abs() * 0.5).contiguous()
    return dict(mod=mod, x=x, y=y, act=act, offset=offset, theta=flat(mod).numpy())


def grad_errors(g, loss, want_g, want_loss, D, A):
    return rel_l2(g, want_g), {k: rel_l2(g[s], want_g[s]) for k, s in block_slices(D, A).items()}, rel_err(loss, want_loss)


HALF_ULP = 2.0 ** -24       # a float32 loss is no closer to its float64 value than this, but for luck: the floor of its yardstick


def pool_grads(errs):
    return (pooled([e[0] for e in errs]), {k: pooled([e[1][k] for e in errs]) for k in BLOCKS},
            max(pooled([e[2] for e in errs]), HALF_ULP))


def _np(t):
    return None if t is None else t.numpy()


@functools.lru_cache(maxsize=None)
def gradient_case(head, regime, weighting, D, A, B, seed):
    """problem() plus w (numpy float32 or None), g (P,) float64, loss, W, and yard = grad_errors of float32 autograd of the
    learners' expression on the same inputs (the indexed form for a mask, the weighted sum for fractional weights)"""
    import torch
    c = problem(head, regime, D, A, B, seed)
    w = make_weights(weighting, B, seed)
    g, loss, W = grad64(head, c["theta"], c["x"].numpy(), c["y"].numpy(), w, _np(c["act"]), _np(c["offset"]))
    if weighting == "mask":
        live = torch.from_numpy(w != 0)
        pick = lambda t: None if t is None else t[live]          # noqa: E731
        expr = weighted_loss(c["mod"], head, c["x"][live], c["y"][live], None, pick(c["act"]), pick(c["offset"]))
    else:
        expr = weighted_loss(c["mod"], head, c["x"], c["y"], None if w is None else torch.from_numpy(w), c["act"], c["offset"])
    ag, al = autograd_grad(expr, c["mod"])
    g.setflags(write=False)
    c.update(w=w, g=g, loss=loss, W=W, yard=grad_errors(ag, al, g, loss, D, A))
    return c


def fit_weights(B, seed):
    """(FIT_ITERS, B) 0 / 1 weights that change every round: three rows in ten always (the down-sampling's positive rows) and a
    fresh third of the others"""
    rng = np.random.default_rng(3000 + seed)
    always = rng.uniform(size=B) < 0.3
    w = (rng.uniform(size=(FIT_ITERS, B)) < 1.0 / 3.0).astype(np.float32)
    w[:, always] = 1.0
    return w


@functools.lru_cache(maxsize=None)
def fit_case(head, D, A, B, seed):
    """the default regime's problem, (FIT_ITERS, B) weights, and fit64's thetas / losses / Ws over FIT_ITERS steps"""
    c = problem(head, "default", D, A, B, seed)
    w = fit_weights(B, seed)
    thetas, losses, Ws, state = fit64(head, c["theta"], c["x"].numpy(), c["y"].numpy(), FIT_ITERS, w, _np(c["act"]), _np(c["offset"]))
    c.update(w=w, thetas=thetas, losses=losses, Ws=Ws, state=state)
    return c


def learners_loop(c, head, iters=FIT_ITERS):
    """the learners' float32 loop (zero_grad / the indexed loss / backward / Adam.step) on a copy of the case's module under its
    weight table -> (thetas, losses)"""
    import copy
    import torch
    mod = copy.deepcopy(c["mod"])
    opt = torch.optim.Adam(mod.parameters(), lr=LR)
    thetas, losses = [flat(mod).numpy().copy()], []
    for i in range(iters):
        live = torch.from_numpy(c["w"][i] != 0)
        pick = lambda t: None if t is None else t[live]          # noqa: E731
        opt.zero_grad()
        loss = weighted_loss(mod, head, c["x"][live], c["y"][live], None, pick(c["act"]), pick(c["offset"]))
        loss.backward()
        opt.step()
        losses.append(loss.item())
        thetas.append(flat(mod).numpy().copy())
    return thetas, np.array(losses)


def fit_errors(theta_end, losses, c):
    """(relative L2 of the displacement theta_end - theta_0, the largest relative error of the loss trace) against fit64's"""
    k = len(losses)
    return (rel_l2(np.asarray(theta_end, np.float64) - c["theta"], c["thetas"][k] - c["theta"]),
            max(rel_err(losses[i], c["losses"][i]) for i in range(k)))


@functools.lru_cache(maxsize=None)
def fit_yardstick(head, D, A, B):
    """the learners' float32 loop's fit_errors, pooled over FIT_SEEDS (vfit64.fit_yardstick's scheme)"""
    errs = []
    for s in FIT_SEEDS:
        c = fit_case(head, D, A, B, s)
        thetas, losses = learners_loop(c, head)
        errs.append(fit_errors(thetas[-1], losses, c))
    return pooled([e[0] for e in errs]), max(pooled([e[1] for e in errs]), HALF_ULP)
