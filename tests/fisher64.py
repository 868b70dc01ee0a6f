"""The Fisher-vector product of include/guardx_fisher.h and the learners' cg in numpy float64, for any hidden width: the
oracle of tests/test_fisher64.py (which checks it against a float64 double backward through autograd),
tests/test_fisher_host.py and tests/test_gpu_fisher.py.  Also the learners' own method (the double backward, in the
precision of the actor it is given) and an actor declared the way the learners declare theirs.

Vectors are in the order of pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]."""
import functools

import numpy as np

EPS = 1e-8


def param_count(D, A, h):
    return A + h * D + h + h * h + h + A * h + A


def unpack(v, D, A, h):
    """(ls, W1, b1, W2, b2, W3, b3) views of the flat vector v"""
    v = np.asarray(v, dtype=np.float64)
    assert v.shape == (param_count(D, A, h),)
    sizes = [("ls", (A,)), ("W1", (h, D)), ("b1", (h,)), ("W2", (h, h)), ("b2", (h,)), ("W3", (A, h)), ("b3", (A,))]
    out, at = [], 0
    for _, shape in sizes:
        n = int(np.prod(shape))
        out.append(v[at:at + n].reshape(shape))
        at += n
    return out


def pack(parts):
    ls, W1, b1, W2, b2, W3, b3 = parts
    return np.concatenate([np.ravel(p) for p in (ls, W1, b1, W2, b2, W3, b3)])


def log_std_curvature(ls, eps=EPS):
    """c of y_ls = c dls"""
    v = np.exp(2.0 * np.asarray(ls, dtype=np.float64))
    return 0.5 * v * (-4.0 * v / (v + eps) ** 2 + 8.0 * v * v / (v + eps) ** 3)


def fvp64(theta, x, obs, A, h=64, eps=EPS, damping=0.0):
    """y = H x + damping x: H the Hessian of the learners' mean KL at the old policy, over the rows of obs (B, D)"""
    o = np.asarray(obs, dtype=np.float64)
    B, D = o.shape
    ls, W1, b1, W2, b2, W3, b3 = unpack(theta, D, A, h)
    dls, dW1, db1, dW2, db2, dW3, db3 = unpack(x, D, A, h)
    h1 = np.tanh(o @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    dh1 = (1.0 - h1 * h1) * (o @ dW1.T + db1)
    dh2 = (1.0 - h2 * h2) * (h1 @ dW2.T + dh1 @ W2.T + db2)
    dmu = h2 @ dW3.T + dh2 @ W3.T + db3
    u = dmu / (np.exp(2.0 * ls) + eps) / B
    gW3, gb3 = u.T @ h2, u.sum(0)
    gz2 = (u @ W3) * (1.0 - h2 * h2)
    gW2, gb2 = gz2.T @ h1, gz2.sum(0)
    gz1 = (gz2 @ W2) * (1.0 - h1 * h1)
    gW1, gb1 = gz1.T @ o, gz1.sum(0)
    y_ls = log_std_curvature(ls, eps) * dls
    return pack((y_ls, gW1, gb1, gW2, gb2, gW3, gb3)) + damping * np.asarray(x, dtype=np.float64)


def dense64(theta, obs, A, h, eps=EPS):
    """H, column by column"""
    P = param_count(np.asarray(obs).shape[1], A, h)
    eye = np.eye(P)
    return np.stack([fvp64(theta, eye[i], obs, A, h, eps) for i in range(P)], axis=1)


def cg64(Hx, g, iters=100, eps=EPS):
    """The learners' cg(Hx, g, cg_iters=iters) in float64, with the stop as a state (include/guardx_fisher.h): r.r == 0
    stops like |p| < eps, so g = 0 gives x = 0 after 0 iterations.  -> x, iterations done, the final r.r"""
    g = np.asarray(g, dtype=np.float64)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr, done = float(r @ r), 0
    stop = rr == 0.0
    for _ in range(iters):
        if stop:
            break
        z = Hx(p)
        alpha = rr / (float(p @ z) + eps)
        x += alpha * p
        r -= alpha * z
        rr_new = float(r @ r)
        p = r + (rr_new / rr) * p
        rr = rr_new
        done += 1
        stop = np.linalg.norm(p) < eps or rr == 0.0
    return x, done, rr


def rel_l2(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.linalg.norm(got - want) / np.linalg.norm(want))


# ---------------------------------------------------------------------------------------------------------------------
# the learners' side (torch)
# ---------------------------------------------------------------------------------------------------------------------
def make_actor(D, A, h=64, seed=0, dtype=None, scale=1.0, log_std=None):
    """A Gaussian MLP actor declared in the learners' order: the log_std parameter first, then mu_net =
    Linear/Tanh/Linear/Tanh/Linear/Identity.  Weights from torch's default initialisation under `seed`, times `scale`
    (one number, or one per layer); log_std spread around the learners' -0.5 so that no two actions share a variance,
    or the A values given."""
    import torch
    nn = torch.nn

    class GaussianActor(nn.Module):
        def __init__(self):
            super().__init__()
            ls = -0.5 + 0.1 * np.arange(A, dtype=np.float32) if log_std is None else np.asarray(log_std, np.float32)
            assert ls.shape == (A,)
            self.log_std = nn.Parameter(torch.as_tensor(ls))
            self.mu_net = nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, A), nn.Identity())

    torch.manual_seed(seed)
    pi = GaussianActor()
    lin = [m for m in pi.mu_net if isinstance(m, nn.Linear)]
    scales = [float(scale)] * len(lin) if np.ndim(scale) == 0 else [float(v) for v in scale]
    assert len(scales) == len(lin)
    with torch.no_grad():
        for m, sc in zip(lin, scales):
            m.weight.mul_(sc)
    return pi.to(dtype) if dtype is not None else pi


def flat(pi):
    import torch
    return torch.cat([p.detach().reshape(-1) for p in pi.parameters()])


def mean_kl(mu_old, log_std_old, mu, log_std, eps=EPS):
    """the learners' mean KL between two batches of diagonal Gaussians, old to new"""
    import torch
    var_old, var = torch.exp(2 * log_std_old), torch.exp(2 * log_std)
    per_dim = 0.5 * (((mu - mu_old) ** 2 + var_old) / (var + eps) - 1) + log_std - log_std_old
    return per_dim.sum(dim=1).mean()


def autograd_fvp(pi, obs, x, eps=EPS):
    """The learners' Hx: the gradient of (grad KL . x), KL between the old policy (the actor's own output, detached) and
    the actor; in the dtype of pi, obs and x"""
    import torch
    params = list(pi.parameters())
    mu = pi.mu_net(obs)
    kl = mean_kl(mu.detach(), pi.log_std.detach(), mu, pi.log_std, eps)
    grad = torch.cat([g.reshape(-1) for g in torch.autograd.grad(kl, params, create_graph=True)])
    hx = torch.autograd.grad(torch.dot(grad, x), params)
    return torch.cat([g.reshape(-1) for g in hx]).detach()


def learners_cg32(Hx, g, iters=100, eps=EPS, trace=False):
    """The loop the learners run, in their types: float32 numpy vectors, Hx a float32 product, the break on |p| < eps.
    -> x; with `trace`: (x, xs, rrs), the iterate and r.r after 0, 1, ... iterations (one entry more than iterations
    done), so that one run serves every smaller iteration count"""
    g = np.asarray(g, dtype=np.float32)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr = np.dot(r, r)
    xs, rrs = [x.copy()], [rr]
    for _ in range(iters):
        z = Hx(p)
        alpha = rr / (np.dot(p, z) + eps)
        x += alpha * p
        r -= alpha * z
        rr_new = np.dot(r, r)
        p = r + (rr_new / rr) * p
        rr = rr_new
        xs.append(x.copy())
        rrs.append(rr)
        if np.linalg.norm(p) < eps:
            break
    return (x, xs, rrs) if trace else x


# ---------------------------------------------------------------------------------------------------------------------
# regimes: where the actor's units sit on tanh (tests/test_fisher64.py asserts what each name promises)
# ---------------------------------------------------------------------------------------------------------------------
H = 64
SMALL, SAT = 0.625, 9.0          # gx_fisher.hip:tanh_act switches to tanh_f at 0.625; tanh_f returns 1 above 9
# name -> the scales of W1, W2, W3 over torch's default initialisation, obs = mean + std N(0, 1), log_std of A actions
REGIMES = {
    "default": dict(scale=(1.0, 1.0, 1.0), obs=(0.0, 1.0), log_std=lambda A: None),                 # make_actor's: -0.5 + 0.1 i
    "trained": dict(scale=(4.0, 3.0, 2.0), obs=(0.5, 1.5), log_std=lambda A: -1.5 + 0.1 * np.arange(A)),
    "saturated": dict(scale=(12.0, 8.0, 1.0), obs=(0.0, 1.0), log_std=lambda A: None),                 # make_actor's: -0.5 + 0.1 i
    "wide_log_std": dict(scale=(1.0, 1.0, 1.0), obs=(0.0, 1.0), log_std=lambda A: np.linspace(-4.0, 1.0, A)),
}
BLOCKS = ("W1", "b1", "W2", "b2", "W3", "b3")
TANGENTS = 8


def block_slices(D, A, h=H):
    """{name: slice of the flat vector} of the six blocks of the net (log_std, the first A entries, is not one)"""
    slices, at = {}, A
    for name, n in zip(BLOCKS, (h * D, h, h * h, h, A * h, A)):
        slices[name] = slice(at, at + n)
        at += n
    assert at == param_count(D, A, h)
    return slices


def pooled(errors):
    """the root-mean-square of the errors of several tangents (or right-hand sides)"""
    e = np.asarray(errors, dtype=np.float64)
    return float(np.sqrt(np.mean(e * e)))


def problem(regime, D, A, B, seed=0):
    """-> (pi, obs, theta, facts): the regime's actor (float32, hidden width 64), obs (B, D) float32, theta its flat
    float32 vector (numpy), and facts = dict(z1, z2): the pre-activations of both layers in float64, (B, 64) each.
    The default regime's actor and obs are the ones tests/test_gpu_fisher.py has always used."""
    import torch
    r = REGIMES[regime]
    pi = make_actor(D, A, H, seed=seed, scale=r["scale"], log_std=r["log_std"](A))
    gen = torch.Generator().manual_seed(100 + seed)
    obs = torch.randn(B, D, generator=gen)
    mean, std = r["obs"]
    if (mean, std) != (0.0, 1.0):
        obs = (mean + std * obs).contiguous()
    theta = flat(pi).numpy()
    _, W1, b1, W2, b2, _, _ = unpack(theta, D, A, H)
    z1 = obs.numpy().astype(np.float64) @ W1.T + b1
    z2 = np.tanh(z1) @ W2.T + b2
    return pi, obs, theta, dict(z1=z1, z2=z2)


def tangents(D, A, n=TANGENTS, seed=0):
    """n standard normal vectors of the actor's length, float32 (n, P)"""
    return np.random.default_rng(1000 + seed).standard_normal((n, param_count(D, A, H))).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# a float32 yardstick: the header's arithmetic in plain numpy float32 (no emulation of the kernel)
# ---------------------------------------------------------------------------------------------------------------------
TILE = 64


def _tile_sums(a, b):
    """sum over rows of a[r, :, None] b[r, None, :]: per 64-row tile in float32, the tiles added in float64 (the rows
    are padded with zeros to whole tiles, which adds nothing)"""
    B = a.shape[0]
    T = -(-B // TILE)
    if T * TILE != B:
        a = np.concatenate([a, np.zeros((T * TILE - B, a.shape[1]), np.float32)])
        b = np.concatenate([b, np.zeros((T * TILE - B, b.shape[1]), np.float32)])
    per_tile = np.matmul(a.reshape(T, TILE, -1).transpose(0, 2, 1), b.reshape(T, TILE, -1))
    assert per_tile.dtype == np.float32
    return per_tile.astype(np.float64).sum(0)


def fvp32(theta, x, obs, A, h=H, eps=EPS, damping=0.0):
    """y = H x + damping x as include/guardx_fisher.h states it, every operation in numpy float32: np.tanh on float32,
    1 - h h in float32, 1 / ((v + eps) B) and the log_std block in float64 and rounded once, the sums over the rows of
    a 64-row tile in float32 and the tiles added in float64.  -> float32"""
    f = np.float32
    o = np.ascontiguousarray(obs, dtype=f)
    B, D = o.shape
    th, xv = np.asarray(theta, dtype=f), np.asarray(x, dtype=f)
    at, parts = 0, []
    for v in (th, xv):
        at, got = 0, []
        for shape in ((A,), (h, D), (h,), (h, h), (h,), (A, h), (A,)):
            n = int(np.prod(shape))
            got.append(v[at:at + n].reshape(shape))
            at += n
        parts.append(got)
    (ls, W1, b1, W2, b2, W3, b3), (dls, dW1, db1, dW2, db2, dW3, db3) = parts
    h1 = np.tanh(o @ W1.T + b1)
    h2 = np.tanh(h1 @ W2.T + b2)
    d1, d2 = f(1.0) - h1 * h1, f(1.0) - h2 * h2
    dh1 = d1 * (o @ dW1.T + db1)
    t2 = h1 @ dW2.T + dh1 @ W2.T + db2
    dh2 = d2 * t2
    dmu = h2 @ dW3.T + dh2 @ W3.T + db3
    inv = (1.0 / ((np.exp(2.0 * ls.astype(np.float64)) + eps) * B)).astype(f)
    u = dmu * inv
    gz2 = (u @ W3) * d2
    gz1 = (gz2 @ W2) * d1
    ones = np.ones((B, 1), f)
    gW3, gb3 = _tile_sums(u, h2), _tile_sums(u, ones).reshape(-1)
    gW2, gb2 = _tile_sums(gz2, h1), _tile_sums(gz2, ones).reshape(-1)
    gW1, gb1 = _tile_sums(gz1, o), _tile_sums(gz1, ones).reshape(-1)
    for t in (h1, dh1, dh2, dmu, u, gz2, gz1):
        assert t.dtype == f
    y_ls = log_std_curvature(ls, eps) * dls.astype(np.float64)
    y = pack((y_ls, gW1, gb1, gW2, gb2, gW3, gb3)).astype(f)
    if damping != 0.0:
        y = y + f(damping) * xv
    assert y.dtype == f
    return y


def header_cg32(Hx, g, iters=100, eps=EPS):
    """The solve as include/guardx_fisher.h states it, around a float32 product Hx: the dots are float64 sums of the
    float32 vectors' products, alpha and rr' / rr are float64, each vector update is rounded once to float32, the stop
    is a state.  -> (xs, rrs, done): the iterate and r.r after 0, 1, ... iterations, frozen after the stop, so
    iters + 1 entries each; done[k] = iterations done when k were asked for"""
    f, d = np.float32, np.float64
    g = np.asarray(g, dtype=f)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr = float(r.astype(d) @ r.astype(d))
    stop = not (rr != 0.0 and np.isfinite(rr))
    xs, rrs, done, n = [x.copy()], [rr], [0], 0
    for _ in range(iters):
        if not stop:
            z = np.asarray(Hx(p), dtype=f)
            alpha = rr / (float(p.astype(d) @ z.astype(d)) + eps)
            x = (x.astype(d) + alpha * p.astype(d)).astype(f)
            r = (r.astype(d) - alpha * z.astype(d)).astype(f)
            rr_new = float(r.astype(d) @ r.astype(d))
            p = (r.astype(d) + (rr_new / rr) * p.astype(d)).astype(f)
            rr = rr_new
            n += 1
            stop = not (np.sqrt(float(p.astype(d) @ p.astype(d))) >= eps) or rr == 0.0
        xs.append(x.copy())
        rrs.append(rr)
        done.append(n)
    return xs, rrs, done


# ---------------------------------------------------------------------------------------------------------------------
# cases shared by tests/test_fisher64.py (CPU) and tests/test_gpu_fisher.py: computed once per process, never written to
# ---------------------------------------------------------------------------------------------------------------------
PRODUCT_SHAPES = [(43, 2, 1), (43, 2, 65), (64, 8, 130), (17, 16, 130)]       # D, A, B
SOLVE_SHAPES = [(43, 2, 257), (64, 8, 130)]
SOLVE_REGIMES = {"default": 0.0, "trained": 0.1, "saturated": 0.0}            # regime -> damping
SOLVE_ITERS = (1, 2, 3, 10)


def rel_err(got, want):
    return abs(float(got) - float(want)) / abs(float(want))


def product_errors(got, want, D, A):
    """(whole-vector relative L2, {block: relative L2}) of one product"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return rel_l2(got, want), {k: rel_l2(got[s], want[s]) for k, s in block_slices(D, A).items()}


def pool_products(gots, wants, D, A):
    """(pooled whole-vector error, {block: pooled error}) over the tangents"""
    errs = [product_errors(g, w, D, A) for g, w in zip(gots, wants)]
    return pooled([e[0] for e in errs]), {k: pooled([e[1][k] for e in errs]) for k in BLOCKS}


@functools.lru_cache(maxsize=None)
def product_case(regime, D, A, B):
    """dict(pi, obs, theta, xs (8, P) float32, wants (8, P) float64 = H64 xs, yard, yard_blocks): the yardsticks are the
    pooled errors of the learners' float32 double backward on the same inputs, whole vector and per block"""
    import torch
    pi, obs, theta, _ = problem(regime, D, A, B)
    xs = tangents(D, A)
    wants = np.stack([fvp64(theta, x, obs.numpy(), A) for x in xs])
    auto = [autograd_fvp(pi, obs, torch.from_numpy(x)).numpy() for x in xs]
    yard, yard_blocks = pool_products(auto, wants, D, A)
    for a in (xs, wants):
        a.setflags(write=False)
    return dict(pi=pi, obs=obs, theta=theta, xs=xs, wants=wants, yard=yard, yard_blocks=yard_blocks)


def solve_errors(xs, ss, rrs, ref):
    """{(what, k): pooled error over the right-hand sides} of a solver's iterates xs[j][k], s[j][k] and r.r rrs[j][k]
    (right-hand side j, k iterations) against the float64 ones of solve_case()"""
    errs = {}
    for k in SOLVE_ITERS:
        errs["x", k] = pooled([rel_l2(xs[j][k], ref["x64"][j][k]) for j in range(len(xs))])
        errs["s", k] = pooled([rel_err(ss[j][k], ref["s64"][j][k]) for j in range(len(xs))])
        errs["r_dot", k] = pooled([rel_err(rrs[j][k], ref["rr64"][j][k]) for j in range(len(xs))])
    return errs


@functools.lru_cache(maxsize=None)
def solve_case(regime, D, A, B):
    """dict(pi, obs, theta, damping, gs (8, P) float32, x64 / s64 / rr64 [j][k]: cg64's iterate, x' H64 x and r.r of
    right-hand side j after k = 0 .. 10 iterations, yard: {(what, k): the pooled error of the learners' float32 loop
    around their float32 double backward}); what is "x" (relative L2), "s" or "r_dot" (relative error)"""
    import torch
    damping = SOLVE_REGIMES[regime]
    pi, obs, theta, _ = problem(regime, D, A, B)
    gs = tangents(D, A, seed=7)
    top = max(SOLVE_ITERS)
    H64 = lambda v: fvp64(theta, v, obs.numpy(), A, damping=damping)                        # noqa: E731
    Hx32 = lambda v: autograd_fvp(pi, obs, torch.from_numpy(v)).numpy() + np.float32(damping) * v    # noqa: E731
    ref = dict(x64=[], s64=[], rr64=[])
    lx, ls, lrr = [], [], []
    for g in gs:
        x64, s64, rr64 = {}, {}, {}
        for k in (0,) + SOLVE_ITERS:
            x, done, rr = cg64(H64, g, iters=k)
            assert done == k
            x64[k], s64[k], rr64[k] = x, float(x @ H64(x)), rr
        ref["x64"].append(x64)
        ref["s64"].append(s64)
        ref["rr64"].append(rr64)
        _, xs, rrs = learners_cg32(Hx32, g, top, trace=True)
        assert len(xs) == top + 1
        lx.append(xs)
        lrr.append(rrs)
        ls.append({k: np.dot(xs[k], Hx32(xs[k])) for k in SOLVE_ITERS})
    yard = solve_errors(lx, ls, lrr, ref)
    gs.setflags(write=False)
    return dict(pi=pi, obs=obs, theta=theta, damping=damping, gs=gs, yard=yard, **ref)
