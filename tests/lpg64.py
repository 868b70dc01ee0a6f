"""lpg64.py -- TEST INFRASTRUCTURE ONLY: LPG's projection (include/guardx_lpg.h) restated twice.  project32 is the numpy
float32 transcription of the header's lines, one IEEE operation per operator; project64 is the same projection in
float64 with a bound on how far a correct fp32 evaluation in the header's order may lie from each value.  The critic's
part -- q = Q(obs, act) with dq, G = grad_scale dQ(obs, 0)/da with dG -- comes from tests/usl64.py:QCritic.forward / grad
(the weights are read from the torch module, never from a packed vector); probe64 puts the two together.

Bounds, propagated the way usl64.one_pass does it (U, MARGIN and chain from oracle/policy64.py; exact fp32 inputs act,
q_init and delta carry no error):
  eps = |delta - q_init|     one rounding: u eps
  top = sum_k G[k] a[k] - eps   A products, A - 1 sums and the difference, every partial result within u of itself:
            chain(A + 1) (sum |G a| + eps), plus dG through |a|, plus eps's own u eps
  bot = sum_k G[k] G[k]      chain(A) bot, plus 2 |G| dG + dG^2 summed
  lam = top / bot            (dtop + |lam| dbot) / (bot - dbot) + u |lam|; unbounded (inf) once dbot reaches bot
  a' = a + sign (lam+ G)     lam+ = max(lam, 0): dlam |G| + (lam+ + dlam) dG, the product's u |lam+ G| and the sum's u |a'|
A row is an EDGE row when |q - delta| < dq, or when it is corrected and |lam| < dlam: there a correct fp32 evaluation may
take another branch than float64 does.  Such rows may differ in `branch` (and what follows from it) only.
"""
import numpy as np

from oracle.policy64 import U, MARGIN, chain

F = np.float32


def project32(a, G, q, q_init, delta, step_sign=1.0):
    """the projection of include/guardx_lpg.h in numpy float32 on rows a (n, A), G (n, A), q (n,), q_init (n,):
    -> a_safe (n, A), lam (n,) [0 for branch 0], branch (n,) [0 q <= delta, 1 lam > 0, 2 lam clipped to 0 or NaN]"""
    a, G, q, qi = np.asarray(a, F), np.asarray(G, F), np.asarray(q, F), np.asarray(q_init, F)
    d, sg = F(delta), F(step_sign)
    A = a.shape[-1]
    with np.errstate(all='ignore'):
        eps = np.abs((d - qi).astype(F))
        top = (G[:, 0] * a[:, 0]).astype(F)
        bot = (G[:, 0] * G[:, 0]).astype(F)
        for k in range(1, A):
            top = (top + (G[:, k] * a[:, k]).astype(F)).astype(F)
            bot = (bot + (G[:, k] * G[:, k]).astype(F)).astype(F)
        top = (top - eps).astype(F)
        lam = (top / bot).astype(F)
        lam = np.where(lam < 0, F(0), lam).astype(F)
        moved = (a + (sg * (lam[:, None] * G).astype(F)).astype(F)).astype(F)
    keep = q <= d
    a_safe = np.where(keep[:, None], a, moved).astype(F)
    return a_safe, np.where(keep, F(0), lam).astype(F), np.where(keep, 0, np.where(lam > 0, 1, 2)).astype(np.int32)


def project64(a, G, dG, q, dq, q_init, delta, step_sign=1.0):
    """the projection in float64 on rows whose G and q carry the errors dG and dq: dict a_safe, lam (0 for branch 0),
    branch, edge and the bounds dlam, da_safe (0 for branch 0: such a row keeps its action exactly)"""
    a, G, dG = np.asarray(a, np.float64), np.asarray(G, np.float64), np.asarray(dG, np.float64)
    q, dq, qi = np.asarray(q, np.float64), np.asarray(dq, np.float64), np.asarray(q_init, np.float64)
    d, sg = float(F(delta)), float(F(step_sign))
    A = a.shape[-1]
    eps = np.abs(d - qi)
    S = np.abs(G * a).sum(-1)
    top = (G * a).sum(-1) - eps
    dtop = MARGIN * (chain(A + 1) * (S + eps) + (dG * np.abs(a)).sum(-1) + U * eps)
    bot = (G * G).sum(-1)
    dbot = MARGIN * (chain(A) * bot + (2.0 * np.abs(G) * dG + dG * dG).sum(-1))
    room = bot - dbot
    with np.errstate(all='ignore'):
        lam = top / bot
        dlam = np.where(room > 0, (dtop + np.abs(lam) * dbot) / np.where(room > 0, room, 1.0) + U * np.abs(lam), np.inf)
        lamp = np.maximum(lam, 0.0)
        step = lamp[:, None] * G
        moved = a + sg * step
        dmoved = MARGIN * (dlam[:, None] * np.abs(G) + (lamp + dlam)[:, None] * dG + U * np.abs(step) + U * np.abs(moved))
    keep = q <= d
    edge = (np.abs(q - d) < dq) | (~keep & ~(np.abs(lam) >= dlam))
    return dict(a_safe=np.where(keep[:, None], a, moved), da_safe=np.where(keep[:, None], 0.0, dmoved),
                lam=np.where(keep, 0.0, lamp), dlam=np.where(keep, 0.0, dlam),
                branch=np.where(keep, 0, np.where(lam > 0, 1, 2)), edge=edge)


def probe64(Q, obs, act, q_init, delta=0.0, grad_scale=1.0, step_sign=1.0):
    """gxp_projection_probe in float64 for a usl64.QCritic `Q`: project64's dict plus q, dq, G, dG"""
    f = Q.forward(obs, act)
    g = Q.grad(obs, np.zeros_like(np.asarray(act, np.float64)), grad_scale)
    r = project64(act, g['s'], g['ds'], f['q'], f['dq'], q_init, delta, step_sign)
    r.update(q=f['q'], dq=f['dq'], G=g['s'], dG=g['ds'])
    return r


def torch_autograd_G(ccritic, obs, A):
    """N times the gradient of mean(Q(obs, 0)) with respect to the action, by torch autograd in float64 on a float64
    copy of the module (lpg_core.py:174-178 times the batch size): what keeps probe64's G honest"""
    import copy
    import torch
    net = copy.deepcopy(getattr(ccritic, 'c_net', ccritic)).double()
    o = torch.as_tensor(np.asarray(obs, np.float64))
    x = torch.zeros(o.shape[0], A, dtype=torch.float64, requires_grad=True)
    net(torch.cat((o, x), 1)).squeeze(-1).mean().backward()
    return o.shape[0] * x.grad.numpy()
