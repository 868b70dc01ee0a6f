"""The Fisher-vector product of include/guardx_fisher.h and the learners' cg in numpy float64, for any hidden width: the
oracle of tests/test_fisher64.py (which checks it against a float64 double backward through autograd),
tests/test_fisher_host.py and tests/test_gpu_fisher.py.  Also the learners' own method (the double backward, in the
precision of the actor it is given) and an actor declared the way the learners declare theirs.

Vectors are in the order of pi.parameters(): log_std[A], W1[h][D], b1[h], W2[h][h], b2[h], W3[A][h], b3[A]."""
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
def make_actor(D, A, h=64, seed=0, dtype=None, scale=1.0):
    """A Gaussian MLP actor declared in the learners' order: the log_std parameter first, then mu_net =
    Linear/Tanh/Linear/Tanh/Linear/Identity.  Weights from torch's default initialisation under `seed`, times `scale`;
    log_std spread around the learners' -0.5 so that no two actions share a variance."""
    import torch
    nn = torch.nn

    class GaussianActor(nn.Module):
        def __init__(self):
            super().__init__()
            self.log_std = nn.Parameter(torch.as_tensor(-0.5 + 0.1 * np.arange(A, dtype=np.float32)))
            self.mu_net = nn.Sequential(nn.Linear(D, h), nn.Tanh(), nn.Linear(h, h), nn.Tanh(), nn.Linear(h, A), nn.Identity())

    torch.manual_seed(seed)
    pi = GaussianActor()
    with torch.no_grad():
        for m in pi.mu_net:
            if isinstance(m, nn.Linear):
                m.weight.mul_(scale)
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


def learners_cg32(Hx, g, iters=100, eps=EPS):
    """The loop the learners run, in their types: float32 numpy vectors, Hx a float32 product, the break on |p| < eps"""
    g = np.asarray(g, dtype=np.float32)
    x, r, p = np.zeros_like(g), g.copy(), g.copy()
    rr = np.dot(r, r)
    for _ in range(iters):
        z = Hx(p)
        alpha = rr / (np.dot(p, z) + eps)
        x += alpha * p
        r -= alpha * z
        rr_new = np.dot(r, r)
        p = r + (rr_new / rr) * p
        rr = rr_new
        if np.linalg.norm(p) < eps:
            break
    return x
