"""policy64.py -- TEST INFRASTRUCTURE ONLY: a float64 restatement of the learner's `ac.step(o)`.

Restated from the reference learner's source (safe_rl_libX/trpo/trpo_core.py; line numbers below are of that
file), not from the C checker or its numpy twin; this module imports neither:
  * mlp()             :30-35   Linear, activation, ..., Linear, output activation (Identity by default)
  * MLPGaussianActor  :110-125  mu = mu_net(obs), std = exp(log_std), logp = Normal(mu, std).log_prob(a).sum(-1)
  * MLPCritic         :136-145  v = v_net(obs).squeeze(-1)
  * MLPActorCritic.step :166-173  returns a, v, logp_a, mu, log(std)
and the cost critic of safe_rl_libX/cpo/cpo_core.py (`vc`, another MLPCritic).  The weights are read from the
torch modules themselves (`net[i].weight` / `.bias`), never from a packed vector, so the packing is under test too.

The reference samples `a` from torch's global generator; the project replaces it by its own documented stream
(guardx_amd/csrc/gx_policy.h normal_pair, oracle/gx_oracle.c normal_pair): one Threefry-2x32-20 block keyed by the
noise seed at counter (global env index, (t0 + t) * 16 + pair) gives the bits b0, b1;
    u1 = ((b0 >> 8) + 1) 2^-24 in (0, 1],  u2 = (b1 >> 8) 2^-24 in [0, 1),
    z0 = sqrt(-2 ln u1) cos(2 pi u2),  z1 = sqrt(-2 ln u1) sin(2 pi u2)     (Box-Muller)
and pair p feeds action dims 2p and 2p + 1; a = mu + std z.

Error bounds.  Every value comes with a bound on how far a correct fp32 evaluation may lie from it.  They are
ESTIMATED, not proven: standard worst-case rounding analysis (u = 2^-24, gamma_n = n u / (1 - n u)) with the
accuracy of the project's fp32 log / exp / tanh / sincos taken from the tests that pin them, and small second-order
terms absorbed by a 1 % margin.  Worst-case sums over K terms are loose at K = 256, so the layers use sqrt(K)-scaled
estimates instead: rounding errors and the errors of different hidden units are taken as independent, and the
bound is SIGMAS = 4 standard deviations of their sum (never more than the worst case).
  * a layer's pre-activation: 4 sqrt(K+1) u (|b| + sum_k |w_k x_k|) for its K-term fma chain (any summation
    order of the K + 1 terms), plus min(sum_k |w_k| dx_k, 4 sqrt(sum_k w_k^2 dx_k^2)) for the error dx of its inputs.
  * the output layer: 16 partial chains of K / 16 terms, a 4-level butterfly and the bias: K / 16 + 5 roundings.
  * tanh: |tanh'| = sech^2 <= sech^2(max(|x| - dx, 0)) carries the input error; the fp32 tanh adds 2.5e-7.
  * the noise: ln's error (5e-7 absolute, 3e-7 relative near u1 = 1), sqrt and the product rounded, 2 pi and
    2 pi u2 rounded to fp32, sin / cos within 1.3e-7.
  * act: mu's error, std's error (exp within 1.6e-7 relative) times |z|, std times z's error, one rounding.
  * logp: per dim the error of (a - mu) / std -- z's error plus the roundings of a and of a - mu over std -- through
    z^2 / 2, three roundings of the quotient, log(std)'s error and two subtractions; then gamma_A over the sum.
How tight: on the test networks the fp32 errors of mu, act, val and vc sit 100 to 500 times below their bounds
(largest err / bound about 0.01 to 0.06; median mu bound 1e-4 to 6e-4), logp's within a factor of about 1.2.  The
bounds catch a wrong weight row, noise pair, counter or log_std entry, and reduced-precision (bf16 / tf32-grade)
arithmetic, but an fp32 tanh or exp off by about 1e-5 could pass: read them as an estimate that catches such
faults, not as a tight fp32 check.
"""
import math

import numpy as np

U = 2.0 ** -24                  # unit roundoff of fp32
TANH_ABS = 2.5e-7               # fp32 tanh (tests/test_policy_rollout.py::test_log_tanh_accuracy)
LOG_ABS, LOG_REL = 5e-7, 3e-7   # fp32 log: absolute, and relative to max(|ln x|, 1e-3) (same test)
EXP_REL = 1.6e-7                # fp32 exp (tests/test_oracle_math.py::test_exp_accuracy)
SINCOS_ABS = 1.3e-7             # fp32 sin / cos (tests/test_oracle_math.py::test_sincos_accuracy)
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
MARGIN = 1.01
SIGMAS = 4.0                    # of the sqrt(K)-scaled estimates below

ACTIVATIONS = {'Tanh': np.tanh, 'Identity': None}


def gamma(n):
    return n * U / (1.0 - n * U)


def chain(n):
    """relative error of an n-rounding sum, sqrt(n)-scaled: the n rounding errors (each within u of a partial sum)
    add as independent terms, taken at SIGMAS standard deviations; never above the worst case gamma_n"""
    return min(gamma(n), SIGMAS * math.sqrt(n) * U)


# ---------------------------------------------------------------------------------------------------------------------
# the noise stream
# ---------------------------------------------------------------------------------------------------------------------
_ROT = ((13, 15, 26, 6), (17, 29, 16, 24))
_M32 = np.uint64(0xFFFFFFFF)


def threefry2x32(k0, k1, x0, x1):
    """Threefry-2x32 with 20 rounds (Salmon et al., SC'11, Random123), elementwise over uint32-valued arrays."""
    u = lambda v: np.asarray(v, dtype=np.uint64) & _M32        # noqa: E731
    k0, k1, x0, x1 = np.broadcast_arrays(u(k0), u(k1), u(x0), u(x1))
    ks = (k0, k1, k0 ^ k1 ^ np.uint64(0x1BD11BDA))
    x0, x1 = (x0 + ks[0]) & _M32, (x1 + ks[1]) & _M32
    for i in range(5):
        for r in _ROT[i % 2]:
            x0 = (x0 + x1) & _M32
            x1 = ((x1 << np.uint64(r)) | (x1 >> np.uint64(32 - r))) & _M32
            x1 = x1 ^ x0
        x0 = (x0 + ks[(i + 1) % 3]) & _M32
        x1 = (x1 + ks[(i + 2) % 3] + np.uint64(i + 1)) & _M32
    return x0.astype(np.uint32), x1.astype(np.uint32)


def _log_err(t):
    """error of the fp32 log whose exact value is t"""
    return np.minimum(LOG_ABS, LOG_REL * np.maximum(np.abs(t), 1e-3))


def normal_pair(seed, env, ctr):
    """(z0, z1, bound): Box-Muller over one Threefry block at counter (env, ctr), elementwise"""
    b0, b1 = threefry2x32(seed[0], seed[1], env, ctr)
    u1 = ((b0.astype(np.float64) // 256) + 1.0) * 2.0 ** -24
    u2 = (b1.astype(np.float64) // 256) * 2.0 ** -24
    lg = np.log(u1)
    L = -2.0 * lg
    r = np.sqrt(L)
    th = 2.0 * np.pi * u2
    c, s = np.cos(th), np.sin(th)
    dL = 2.0 * _log_err(lg) + U * L
    dr = r - np.sqrt(np.maximum(L - dL, 0.0))              # >= sqrt(L + dL) - r
    dr = dr + 2.0 * U * (r + dr)                             # sqrt rounded
    dth = 3.0 * U * th                                       # 2 pi and the product rounded
    dsc = SINCOS_ABS + dth
    out = []
    for z, v in ((r * c, c), (r * s, s)):
        dz = dr * (np.abs(v) + dsc) + r * dsc
        out.append(MARGIN * (dz + U * (np.abs(z) + dz)))
    return r * c, r * s, np.maximum(out[0], out[1])


def noise(seed, env, step, A):
    """z (..., A) and its bound for the rows at global env index `env` and global step `step` (broadcast)"""
    env, step = np.broadcast_arrays(np.asarray(env, np.int64), np.asarray(step, np.int64))
    pairs = (A + 1) // 2
    p = np.arange(pairs, dtype=np.int64)
    ctr = (step[..., None] * 16 + p) & 0xFFFFFFFF
    z0, z1, dz = normal_pair(seed, env[..., None], ctr)
    z = np.stack([z0, z1], -1).reshape(*env.shape, 2 * pairs)[..., :A]
    dz = np.repeat(dz, 2, -1)[..., :A]
    return z, dz


# ---------------------------------------------------------------------------------------------------------------------
# the networks
# ---------------------------------------------------------------------------------------------------------------------
def layers(net):
    """[(W, b, activation)] of an nn.Sequential built the way mlp() builds it, in float64 from the module's tensors"""
    mods = list(net)
    out, i = [], 0
    while i < len(mods):
        m = mods[i]
        if type(m).__name__ != 'Linear':
            raise ValueError(f"expected Linear at position {i}, got {type(m).__name__}")
        act = None
        if i + 1 < len(mods) and type(mods[i + 1]).__name__ != 'Linear':
            name = type(mods[i + 1]).__name__
            if name not in ACTIVATIONS:
                raise ValueError(f"policy64 restates Tanh / Identity activations, not {name}")
            act = ACTIVATIONS[name]
            i += 1
        W = m.weight.detach().cpu().double().numpy()
        b = m.bias.detach().cpu().double().numpy()
        out.append((W, b, act))
        i += 1
    return out


def mlp(net_layers, x, head_partials=16):
    """forward pass in float64: (y, bound on a correct fp32 evaluation's error, [hidden pre-activations])"""
    y = np.asarray(x, np.float64)
    dy = np.zeros_like(y)
    pres = []
    n = len(net_layers)
    for li, (W, b, act) in enumerate(net_layers):
        K = W.shape[1]
        aW = np.abs(W)
        pre = y @ W.T + b
        S = (np.abs(y) + dy) @ aW.T + np.abs(b)
        g = chain(K // head_partials + 5) if li == n - 1 else chain(K + 1)
        dpre = MARGIN * (g * S + np.minimum(dy @ aW.T, SIGMAS * np.sqrt((dy * dy) @ (W * W).T)))
        if act is np.tanh:
            pres.append(pre)
            y = np.tanh(pre)
            sech = 1.0 / np.cosh(np.minimum(np.maximum(np.abs(pre) - dpre, 0.0), 350.0))
            dy = np.minimum(dpre * sech * sech, 2.0) + TANH_ABS
        else:
            y, dy = pre, dpre
    return y, dy, pres


def gaussian_logp(act, mu, log_std):
    """Normal(mu, exp(log_std)).log_prob(act).sum(-1) (torch.distributions.Normal.log_prob)"""
    std = np.exp(log_std)
    return np.sum(-((act - mu) ** 2) / (2.0 * std * std) - log_std - HALF_LOG_2PI, -1)


class ActorCritic:
    """the learner's actor-critic in float64: from `ac` (.pi.mu_net, .pi.log_std, .v.v_net) or the three pieces"""

    def __init__(self, ac=None, *, mu_net=None, v_net=None, log_std=None):
        if ac is not None:
            mu_net, v_net, log_std = ac.pi.mu_net, ac.v.v_net, ac.pi.log_std
        self.pi = layers(mu_net)
        self.v = layers(v_net)
        ls = log_std.detach().cpu() if hasattr(log_std, 'detach') else log_std
        self.log_std = np.asarray(ls, np.float64).reshape(-1)
        self.A = self.pi[-1][0].shape[0]
        assert self.log_std.size == self.A

    def step(self, obs, seed, env, step):
        """ac.step over rows obs (..., D) at global env index `env` and global step `step` (both broadcast to obs'
        leading shape): dict of mu, act, logp, val, logstd and, under the same names + '_b', their bounds"""
        A, ls = self.A, self.log_std
        mu, dmu, pres = mlp(self.pi, obs)
        v, dv, pres_v = mlp(self.v, obs)
        z, dz = noise(seed, env, step, A)
        std = np.exp(ls)
        act = mu + std * z
        logp = gaussian_logp(act, mu, ls)
        dstd = EXP_REL * std
        d_ls = MARGIN * EXP_REL + _log_err(ls)
        d_act = MARGIN * (dmu + std * dz + (np.abs(z) + dz) * dstd)
        d_act = d_act + MARGIN * U * (np.abs(act) + d_act)
        # logp: the kernel's (a - mu) / std is z up to z's error and the roundings of a and of a - mu
        dzeta = MARGIN * (dz + U * (np.abs(act) + d_act + np.abs(std * z) + d_act) / std)
        q = 0.5 * z * z
        dq = np.abs(z) * dzeta + 0.5 * dzeta ** 2 + MARGIN * 3.0 * U * 0.5 * (np.abs(z) + dzeta) ** 2
        term = np.abs(q) + np.abs(ls) + HALF_LOG_2PI
        dterm = dq + d_ls + U * HALF_LOG_2PI + MARGIN * 2.0 * U * term
        d_logp = MARGIN * (dterm.sum(-1) + gamma(A) * (term + dterm).sum(-1))
        return dict(mu=mu, act=act, logp=logp, val=v[..., 0], logstd=ls,
                    mu_b=dmu, act_b=d_act, logp_b=d_logp, val_b=dv[..., 0], logstd_b=d_ls,
                    z=z, z_b=dz, pre=pres + pres_v)


def critic(net, obs):
    """MLPCritic(obs) = v_net(obs).squeeze(-1) in float64: (v, bound)"""
    v, dv, _ = mlp(layers(getattr(net, 'v_net', net)), obs)
    return v[..., 0], dv[..., 0]


def rollout(ac, out, seed, t0=0, env_offset=0, cost_critic=None):
    """what rollout_policy's policy outputs should be, given the observations it recorded (out['obs'] (T, N, D),
    out['obs_last'] (N, D)): ac.step on every row, at env index env_offset + i and step t0 + t; val_last on
    obs_last; with `cost_critic` (the torch module) vc / vc_last.  dict of want values and bounds ('<key>_b')."""
    obs, last = np.asarray(out['obs']), np.asarray(out['obs_last'])
    T, N = obs.shape[:2]
    env = env_offset + np.arange(N, dtype=np.int64)[None, :]
    step = t0 + np.arange(T, dtype=np.int64)[:, None]
    w = ac.step(obs, seed, env, step)
    vl, dvl, _ = mlp(ac.v, last)
    w['val_last'], w['val_last_b'] = vl[..., 0], dvl[..., 0]
    if cost_critic is not None:
        w['vc'], w['vc_b'] = critic(cost_critic, obs)
        w['vc_last'], w['vc_last_b'] = critic(cost_critic, last)
    return w


OUTPUTS = ('mu', 'act', 'logp', 'val', 'val_last', 'logstd')


def compare(got, want, keys=OUTPUTS, what="", report=None):
    """every got[k] within want[k + '_b'] of want[k]; returns {k: (largest err / bound, median bound)} (also added
    to `report` when given).  NaN / Inf in got fail."""
    res = {}
    for k in keys:
        g = np.asarray(got[k], np.float64)
        w, b = np.broadcast_arrays(want[k], want[k + '_b'])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        err = np.abs(g - w)
        ok = err <= b
        if not ok.all():
            i = np.unravel_index(np.argmax(np.where(ok, 0.0, np.where(np.isfinite(err), err / b, np.inf))), g.shape)
            raise AssertionError(f"{what} {k}: {int((~ok).sum())} of {ok.size} outside the float64 bound; worst at "
                                 f"{tuple(int(j) for j in i)}: got {g[i]!r}, want {w[i]!r}, bound {b[i]:.3g}")
        res[k] = (float((err / b).max()), float(np.median(b)))
    if report is not None:
        for k, v in res.items():
            old = report.get(k, (0.0, v[1]))
            report[k] = (max(old[0], v[0]), v[1])
    return res
