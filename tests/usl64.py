"""usl64.py -- TEST INFRASTRUCTURE ONLY: USL's cost critic Q(obs, a) = Softplus(c_net(cat(obs, a))), its analytic action
gradient and the learner's correction (safe_rl_libX/usl/usl_core.py:146-196) restated in float64, with a bound on how far
a correct fp32 evaluation in the kernel's operation order (include/guardx_usl.h) may lie from each value; and update32,
the numpy float32 transcription of the update step.  The weights are read from the torch module, never from a packed
vector.

The rule (usl_core.py:180-194).  safety_correction never clears act.grad: c_net.zero_grad() (182) zeroes the network's
gradients only and act is one leaf tensor across the passes, so every pred.mean().backward() (184) ADDS to act.grad, in
fp32.  The update of pass p (190-194) therefore uses the running sum of the passes' scaled gradients,
    acc_p = acc_{p-1} + s_p  (acc_1 = s_1),      a = a - eta acc_p / (max_k |acc_p[k]| + 1e-8),
not s_p alone.  one_pass and iterate carry acc; update32 takes it.  (Rows that have stopped keep accumulating in the
reference and never move again: their sum is never read.)

Bounds.  ESTIMATED like oracle/policy64.py's, from its constants (U, chain, MARGIN, SIGMAS, TANH_ABS, EXP_REL) and the
statewise path's Softplus bound (tests/test_gpu_statewise.py:softplus_bound); exact fp32 inputs (obs, a) carry no error.
  forward   policy64.mlp's recurrence, kept per layer: pre-activation 4 sqrt(K + 1) u sum |w x| plus the inputs' error
            through |W| (or 4 sigma of it), tanh's slope at the near end of the interval, + TANH_ABS.
  q         softplus_bound(z3) + softplus'(z3) dz3 (slope <= 1; taken at z3 + dz3).
  t = 1 - h h     two roundings on values <= 1: 2 u, plus 2 |h| dh + dh^2.  (A saturated fp32 tanh gives t = 0 exactly
            where the true t is 4 e^(-2|x|) <= 6e-8: inside 2 |h| TANH_ABS.)
  d2 = t2 w3      dt2 |w3| + u |d2|
  d1 = d2 W2      an h_c-term fma chain from 0: chain(h_c) sum |d2 W2| + the error of d2 through |W2| (or 4 sigma)
  g1 = t1 d1      dt1 |d1| + (t1 + dt1) dd1 + u |g1|
  g~ = g1 W1a     16 partial chains and a butterfly: chain(h_c / 16 + 4) sum |g1 W1a| + dg1 through |W1a| (or 4 sigma)
  sp = e / (e + 1)   sigma' = sp (1 - sp): sp (1 - sp) (dz3 + EXP_REL) + 2 u sp; + 2.1e-9 for the switch to 1 at z3 > 20,
            + 1e-37 for exp's flush to zero below -87
  c = grad_scale sp, s = c g~      one rounding each
  acc = acc + s   every add contributes ds plus one rounding, u |acc|, to dacc (none in a row's first pass, acc = s)
  Z = max |acc|   dZ = max dacc;  den = Z + 1e-8: dZ + u den
  r = acc / den   (dacc + |r| dden) / (den - dden) + u |r|, never more than 2 (|r| <= 1 on both sides)
  a' = a - eta r  eta dr + u |eta r| + u |a'|
A row is an EDGE row when |q - delta| < dq or |max a - 1| < da at the pass: there a correct fp32 evaluation may stop where
float64 goes on, or the reverse: such rows may differ in `stop` (and what follows from it) only, and their share is capped.
"""
import numpy as np

from oracle import policy64
from oracle.policy64 import U, MARGIN, SIGMAS, TANH_ABS, EXP_REL, chain

F = np.float32
THRESH_JUMP = float(np.log1p(np.exp(-20.0)))


def softplus64(x):
    x = np.asarray(x, np.float64)
    return np.where(x > 20.0, x, np.log1p(np.exp(np.minimum(x, 20.0))))


def softplus_bound(x):
    """tests/test_gpu_statewise.py:softplus_bound (derived there)"""
    x = np.asarray(x, np.float64)
    L = np.log1p(np.exp(-np.abs(x)))
    y = softplus64(x)
    b = MARGIN * ((EXP_REL + 4.0 * U) * L + 2.0 * policy64._log_err(L) + U * np.abs(y)) + 2.0 ** -126 + THRESH_JUMP
    return np.where(x > 20.0, THRESH_JUMP, b)


def sigmoid64(z):
    z = np.asarray(z, np.float64)
    return np.where(z > 20.0, 1.0, 1.0 / (1.0 + np.exp(-np.minimum(z, 20.0))))


def _through(dx, W):
    """error dx (n, K) of the inputs through y = x W^T, W (out, K): worst case, or SIGMAS sigma of independent terms"""
    return np.minimum(dx @ np.abs(W).T, SIGMAS * np.sqrt((dx * dx) @ (W * W).T))


class QCritic:
    """c_net in float64, from the module (anything with .c_net, or the nn.Sequential Linear/Tanh/Linear/Tanh/Linear/
    Softplus itself)"""

    def __init__(self, ccritic):
        net = getattr(ccritic, 'c_net', ccritic)
        mods = [m for m in net if type(m).__name__ != 'Identity']
        assert type(mods[-1]).__name__ == 'Softplus'
        (self.W1, self.b1, _), (self.W2, self.b2, _), (self.W3, self.b3, _) = policy64.layers(mods[:-1])
        self.hc = self.W1.shape[0]

    def forward(self, obs, a):
        """dict z3, q, h1, h2 and their bounds (dz3, dq, dh1, dh2)"""
        x = np.concatenate([np.asarray(obs, np.float64), np.asarray(a, np.float64)], -1)
        y, dy, r = x, np.zeros_like(x), {}
        for i, (W, b) in enumerate(((self.W1, self.b1), (self.W2, self.b2)), 1):
            pre = y @ W.T + b
            S = (np.abs(y) + dy) @ np.abs(W).T + np.abs(b)
            dpre = MARGIN * (chain(W.shape[1] + 1) * S + _through(dy, W))
            y = np.tanh(pre)
            sech = 1.0 / np.cosh(np.minimum(np.maximum(np.abs(pre) - dpre, 0.0), 350.0))
            dy = np.minimum(dpre * sech * sech, 2.0) + TANH_ABS
            r[f'h{i}'], r[f'dh{i}'] = y, dy
        w3 = self.W3[0]
        z3 = y @ w3 + self.b3[0]
        S = (np.abs(y) + dy) @ np.abs(w3) + abs(self.b3[0])
        dz3 = MARGIN * (chain(self.hc // 16 + 5) * S + _through(dy, self.W3)[..., 0])
        r['z3'], r['dz3'] = z3, dz3
        r['q'] = softplus64(z3)
        r['dq'] = softplus_bound(z3) + sigmoid64(z3 + dz3) * dz3
        return r

    def grad(self, obs, a, grad_scale=1.0):
        """forward's dict plus gt (the gradient of z3 with respect to a), sp, s = grad_scale sp gt and the bound ds"""
        r = self.forward(obs, a)
        D = self.W1.shape[1] - np.asarray(a).shape[-1]
        W1a = self.W1[:, D:]                                   # (hc, A)
        w3 = self.W3[0]
        gs = float(F(grad_scale))
        t2 = 1.0 - r['h2'] ** 2
        dt2 = 2.0 * np.abs(r['h2']) * r['dh2'] + r['dh2'] ** 2 + 2.0 * U
        d2 = t2 * w3
        dd2 = dt2 * np.abs(w3) + U * np.abs(d2)
        d1 = d2 @ self.W2
        dd1 = MARGIN * (chain(self.hc) * (np.abs(d2) + dd2) @ np.abs(self.W2) + _through(dd2, self.W2.T))
        t1 = 1.0 - r['h1'] ** 2
        dt1 = 2.0 * np.abs(r['h1']) * r['dh1'] + r['dh1'] ** 2 + 2.0 * U
        g1 = t1 * d1
        dg1 = dt1 * np.abs(d1) + (t1 + dt1) * dd1 + U * np.abs(g1)
        gt = g1 @ W1a
        dgt = MARGIN * (chain(self.hc // 16 + 4) * (np.abs(g1) + dg1) @ np.abs(W1a) + _through(dg1, W1a.T))
        sp = sigmoid64(r['z3'])
        dsp = MARGIN * (sp * (1.0 - sp) * (r['dz3'] + EXP_REL) + 2.0 * U * sp) + THRESH_JUMP + 1e-37
        c = gs * sp
        dc = gs * dsp + U * c
        s = c[..., None] * gt
        ds = MARGIN * (dc[..., None] * np.abs(gt) + (c + dc)[..., None] * dgt + U * np.abs(s))
        r.update(gt=gt, dgt=dgt, sp=sp, s=s, ds=ds)
        return r

    def one_pass(self, obs, a, delta=0.0, eta=0.05, grad_scale=1.0, da=None, acc=None, dacc=None):
        """one pass of the iteration on exact fp32 rows (da: the error the actions already carry, for the edge test;
        acc, dacc: the running sum of the earlier passes' s and its bound, None in the first pass): forward / grad's
        dict plus stop (-1: the row moved, 1, 2), edge, a_next and its bound da_next, and acc / dacc after this pass"""
        a = np.asarray(a, np.float64)
        r = self.grad(obs, a, grad_scale)
        if acc is None:
            acc, dacc = r['s'], r['ds']
        else:
            acc = np.asarray(acc, np.float64) + r['s']
            dacc = (0.0 if dacc is None else dacc) + r['ds'] + U * np.abs(acc)
        da = np.zeros(a.shape[:-1]) if da is None else da
        mx = a.max(-1)
        stop = np.where(mx > 1.0, 1, np.where(r['q'] <= float(F(delta)), 2, -1))
        edge = (np.abs(mx - 1.0) < da) | ((mx <= 1.0) & (np.abs(r['q'] - float(F(delta))) < r['dq']))
        e32, tiny = float(F(eta)), float(F(1e-8))
        s, ds = acc, dacc
        Z, dZ = np.abs(s).max(-1), ds.max(-1)
        den = Z + tiny
        dden = dZ + U * den
        q = s / den[..., None]
        room = (den - dden)[..., None]
        dq = np.where(room > 0, (ds + np.abs(q) * dden[..., None]) / np.where(room > 0, room, 1.0) + U * np.abs(q), 2.0)
        dq = np.minimum(dq, 2.0)
        a_next = a - e32 * q
        da_next = MARGIN * (e32 * dq + U * np.abs(e32 * q) + U * np.abs(a_next))
        moved = stop < 0
        r.update(acc=acc, dacc=dacc, stop=stop, edge=edge, a_next=np.where(moved[..., None], a_next, a),
                 da_next=np.where(moved[..., None], da_next, 0.0))
        return r

    def iterate(self, obs, a, delta=0.0, niter=20, eta=0.05, grad_scale=1.0):
        """the whole iteration in float64 (no bounds): a_safe, iters, stop (0 niter exhausted, 1, 2), q0"""
        a = np.array(a, np.float64)
        n = a.shape[0]
        stop, iters, q0, acc = np.full(n, -1), np.zeros(n, np.int64), None, None
        for p in range(niter):
            live = stop < 0
            if not live.any():
                break
            r = self.one_pass(obs, a, delta, eta, grad_scale, acc=acc)
            acc = r['acc']
            if p == 0:
                q0 = r['q']
            st = np.where(live, r['stop'], stop)
            moved = live & (st < 0)
            a = np.where(moved[:, None], r['a_next'], a)
            iters += moved
            stop = st
        if q0 is None:
            q0 = self.forward(obs, a)['q']
        return dict(a_safe=a, iters=iters, stop=np.where(stop < 0, 0, stop), q0=q0)


def update32(a, s, eta):
    """the update of include/guardx_usl.h in numpy float32 from the ACCUMULATED s (the fp32 running sum of the passes'
    scaled gradients; the first pass's s itself), one IEEE operation per operator: Z = |s[0]|, then
    Z = |s[i]| > Z ? |s[i]| : Z for i ascending; den = Z + 1e-8f; a[i] - eta * (s[i] / den)"""
    a, s = np.asarray(a, F), np.asarray(s, F)
    ab = np.abs(s)
    Z = ab[..., 0].copy()
    for i in range(1, s.shape[-1]):
        Z = np.where(ab[..., i] > Z, ab[..., i], Z).astype(F)
    den = (Z + F(1e-8)).astype(F)
    with np.errstate(all='ignore'):
        r = (s / den[..., None]).astype(F)
        return (a - (F(eta) * r).astype(F)).astype(F)


def torch_autograd_s(ccritic, obs, a, grad_scale=1.0):
    """s = grad_scale dQ/da by torch autograd in float64 on a float64 copy of the module: what keeps grad() honest"""
    import copy
    import torch
    net = copy.deepcopy(getattr(ccritic, 'c_net', ccritic)).double()
    o = torch.as_tensor(np.asarray(obs, np.float64))
    x = torch.as_tensor(np.asarray(a, np.float64)).clone().requires_grad_()
    q = net(torch.cat((o, x), 1)).squeeze(-1)
    q.sum().backward()
    return q.detach().numpy(), float(F(grad_scale)) * x.grad.numpy()
