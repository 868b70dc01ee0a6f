"""The actor half of the first-order learners' update() on the device path: `PolicyFit(ac.pi, lr=pi_lr).fit(data,
iters=train_pi_iters, target_kl=target_kl, clip_ratio=clip_ratio)` is their

    for i in range(train_pi_iters):
        pi_optimizer.zero_grad(); loss_pi, pi_info = compute_loss_pi(data)
        if pi_info['kl'] > target_kl: break
        loss_pi.backward(); pi_optimizer.step()

with pi_optimizer = Adam(ac.pi.parameters(), lr=pi_lr) (safe_rl_libX ppo_one_episode/ppo.py:307-316 and the same lines of
ppo/ppo_train.py, ppo_runner.py and ppo_isaac.py; espo_one_episode/espo.py:292-301 with clip_ratio=None and its delta as
target_kl; a2c/a2c.py:303-307 with loss='logp', iters=1, target_kl=None, clip_ratio=None) as one stream-ordered call: two
launches per iteration, no autograd graph, nothing synchronised; the stop is decided on the device and the launches after it
return at once (libguardx_pifit.so, include/guardx_pifit.h; INTEGRATION.md, "Policy fit on the device path").

The gradient is taken in closed form over the Gaussian MLP actor (hidden width 64, tanh, a linear mean, a free log_std) with
the row weight autograd gives torch.min of the two branches, and Adam is torch's single-tensor form with its step count on
the device.  Vectors are in the order of ac.pi.parameters(), log_std first (fisher.flat_params).

Not served: mpi_avg and mpi_avg_grads (several ranks averaging kl and their gradients; `gradient` is the half before an
all-reduce), alphappo's beta * kl term, papo's and apo's variance losses, pdo's Lagrangian loop, mini-batches, weight decay
and amsgrad.
"""
import ctypes as C
import math

import torch

from . import _pifit_native as _n
from . import fisher as _fisher

HIDDEN = _fisher.HIDDEN
HALF_LOG_2PI = 0.5 * math.log(2.0 * math.pi)
TABLE_LIMIT = 2 ** 20
LOSSES = ('ratio', 'logp')
WHO = "PolicyFit"


def _checked(name, x, shape, device):
    """fisher._checked in PolicyFit's name"""
    try:
        return _fisher._checked(name, x, shape, device)
    except ValueError as e:
        raise ValueError(str(e).replace("FisherOperator", WHO, 1)) from None


def bias_table(betas, limit=TABLE_LIMIT):
    """([b1 ** 1, b2 ** 1, b1 ** 2, b2 ** 2, ...], t_sat): Python's b ** t for t = 1 .. t_sat, t_sat the first t at which
    1 - b1 ** t == 1.0 and 1 - b2 ** t == 1.0 in float64 (from there on both bias corrections are exactly 1, so the kernel,
    which does not know t on the host, reads entry min(t, t_sat)).  NotImplementedError where t_sat would pass `limit`."""
    b1, b2 = float(betas[0]), float(betas[1])
    if any(1.0 - b ** limit != 1.0 for b in (b1, b2)):
        raise NotImplementedError(f"{WHO} supports betas whose bias corrections reach 1 within 2^20 steps, not {(b1, b2)}")
    table, t = [], 0
    while True:
        t += 1
        p1, p2 = b1 ** t, b2 ** t
        table += [p1, p2]
        if 1.0 - p1 == 1.0 and 1.0 - p2 == 1.0:
            return table, t


def _loss_args(who, clip_ratio, loss):
    """(the C loss kind, clip_ratio as a float, NaN for none)"""
    if loss not in LOSSES:
        raise ValueError(f"{who}: loss must be 'ratio' or 'logp', got {loss!r}")
    if loss == 'logp' and clip_ratio is not None:
        raise ValueError(f"{who}: loss='logp' takes clip_ratio=None")
    if clip_ratio is not None and not float(clip_ratio) >= 0.0:
        raise ValueError(f"{who}: clip_ratio must be None or a number that is not negative, got {clip_ratio!r}")
    return LOSSES.index(loss), float('nan') if clip_ratio is None else float(clip_ratio)


class PolicyFit:
    """`pi`: an actor FisherOperator serves (.mu_net Linear/Tanh/Linear/Tanh/Linear[/Identity], hidden width 64, D <= 128, an
    even A <= 16, and .log_std).  Built once, where the learner builds pi_optimizer: the object owns Adam's moments `m` and
    `v` (float32, (P,)), the step count `count` (int64 on the device, from the first call on: the host does not know how
    many steps a call took) and the workspace, and all of it persists across fit calls as the optimizer's state persists
    across epochs.  `lr`, `betas`, `eps`: torch.optim.Adam's.  `workgroups`: the size of the gradient's grid, 0 = the
    default for the device (a test hook; the result depends on it in the last bits only)."""

    def __init__(self, pi, lr, betas=(0.9, 0.999), eps=1e-8, workgroups=0, weight_decay=0.0, amsgrad=False):
        try:
            self.D, self.A = _fisher._layers(pi)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("FisherOperator", WHO)) from None
        if weight_decay != 0.0 or amsgrad:
            raise NotImplementedError(f"{WHO} supports Adam without weight_decay and amsgrad")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr >= 0.0 and self.eps >= 0.0 and all(0.0 <= b < 1.0 for b in self.betas)):
            raise ValueError(f"{WHO}: lr and eps must not be negative, and betas must lie in [0, 1)")
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError(f"{WHO}: workgroups must be 0 (the default) .. 4096")
        self.table, self.t_sat = bias_table(self.betas)
        self.pi, self.workgroups = pi, int(workgroups)
        self.P = _fisher.param_count(self.D, self.A)
        self.m = self.v = self.count = None
        self._table, self._work, self._lib = None, None, None

    def _batch(self, data):
        for key in ('obs', 'act', 'adv', 'logp'):
            if key not in data:
                raise ValueError(f"{WHO}: data has no '{key}'")
        obs = _checked("obs", data['obs'], (None, self.D), None)
        B = int(obs.shape[0])
        if B < 1 or B >= 2 ** 31:
            raise ValueError(f"{WHO}: obs must have 1 .. 2^31 - 1 rows, got {B}")
        act = _checked("act", data['act'], (B, self.A), obs.device)
        adv = _checked("adv", data['adv'], (B,), obs.device)
        logp = _checked("logp", data['logp'], (B,), obs.device)
        return obs, act, adv, logp, B

    def _workspace(self, B, device):
        """the library, and a workspace for B rows on `device` (kept while it is large enough)"""
        if self._lib is None:
            self._lib = _n.load()
        nbytes = int(self._lib.gxa_work_bytes(B, self.D, self.A, self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"{WHO}: {self._lib.gxa_last_error().decode()}")
        if self._work is None or self._work.device != device or self._work.numel() * 8 < nbytes:
            self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        return self._work

    def _state(self, device):
        """m, v, the count and the table of bias corrections on `device` (made, or moved, at the first call there)"""
        if self.m is None:
            self.m = torch.zeros(self.P, dtype=torch.float32, device=device)
            self.v = torch.zeros(self.P, dtype=torch.float32, device=device)
            self.count = torch.zeros(2, dtype=torch.int64, device=device)    # the count; the value a call started from
        elif self.m.device != device:
            self.m, self.v, self.count = self.m.to(device), self.v.to(device), self.count.to(device)
        if self._table is None or self._table.device != device:
            self._table = torch.tensor(self.table, dtype=torch.float64).to(device)

    def gradient(self, data, clip_ratio=0.2, loss='ratio'):
        """(g (P,) float32, info) of the loss at pi's current parameters, on the device: one backward(), and the half before
        an all-reduce.  info, 0-dim float64 device tensors: `loss`, `kl` = mean(logp_old - logp), `cf` and `ent`.  Nothing
        here synchronises."""
        kind, clip = _loss_args(f"{WHO}.gradient", clip_ratio, loss)
        obs, act, adv, logp, B = self._batch(data)
        device = obs.device
        work = self._workspace(B, device)
        theta = _fisher.flat_params(self.pi, device).contiguous()
        g = torch.empty_like(theta)
        info = torch.empty(4, dtype=torch.float64, device=device)
        hyper = (C.c_double * 1)(clip)
        with torch.cuda.device(device):                         # the launch goes to the data's device, whichever is current
            _n.check(self._lib.gxa_gradient(B, self.D, self.A, HIDDEN, theta.data_ptr(), obs.data_ptr(), act.data_ptr(),
                                            adv.data_ptr(), logp.data_ptr(), kind, C.cast(hyper, C.c_void_p), self.workgroups,
                                            work.data_ptr(), g.data_ptr(), info.data_ptr(), _fisher._stream(device)))
        return g, {'loss': info[0], 'kl': info[1], 'cf': info[2], 'ent': info[3]}

    def fit(self, data, iters=80, target_kl=None, clip_ratio=0.2, loss='ratio'):
        """The learners' loop over at most `iters` iterations.  `data`: a mapping with obs (B, D), act (B, A), adv (B,) and
        logp (B,), float32, contiguous, on one cuda device (what *_rollout_batch gives and SurrogateGradient takes; adc is
        ignored).  `target_kl`: a number, the threshold itself (not 1.5 times it), or None: never stop.  `clip_ratio`: a
        number, or None for the unclipped surrogate -(ratio * adv).mean() (espo).  `loss`: 'ratio', or 'logp' for a2c's
        -(logp * adv).mean(), which takes clip_ratio=None.  Iteration i evaluates loss, kl and cf at the current parameters,
        stops where kl > target_kl (a NaN kl does not stop) and otherwise takes one Adam step; a stopped iteration takes no
        step.  The actor's parameters are packed, updated on the device and copied back in place, stream-ordered.
        -> info, device tensors only: `loss`, `kl`, `cf` (iters,) float64, entry i the value at the parameters before step i,
        NaN after the stopping iteration; `stop_iter` (int32) the learners' StopIter, the iteration that stopped, else
        iters - 1; `steps` (int32) the Adam steps of this call; `step` (int64) the optimizer's count after it; `loss_last`,
        `kl_last`, `cf_last` the last evaluated entries (what the learners log as loss_pi.item(), pi_info['kl'] and
        pi_info['cf']); `ent` the entropy at the call's first parameters (pi_info_old['ent']); `theta` the flat parameters
        after the call.  iters = 0 changes nothing.  Nothing here synchronises, and the number of launches, 2 iters, does
        not depend on the data."""
        if not (int(iters) == iters and iters >= 0):
            raise ValueError(f"{WHO}.fit: iters must be a non-negative integer")
        iters = int(iters)
        kind, clip = _loss_args(f"{WHO}.fit", clip_ratio, loss)
        if target_kl is not None and (torch.is_tensor(target_kl) or math.isnan(float(target_kl))):
            raise ValueError(f"{WHO}.fit: target_kl must be None or a Python number")
        target = float('nan') if target_kl is None else float(target_kl)
        obs, act, adv, logp, B = self._batch(data)
        device = obs.device
        work = self._workspace(B, device)
        self._state(device)
        theta = _fisher.flat_params(self.pi, device).contiguous()
        nan = float('nan')
        trace = torch.full((3, iters), nan, dtype=torch.float64, device=device)
        last = torch.full((4,), nan, dtype=torch.float64, device=device)
        ctl = torch.zeros(3, dtype=torch.int32, device=device)  # the stop flag, stop_iter, steps
        ctl[1].fill_(iters - 1)
        if iters:
            hyper = (C.c_double * 6)(self.lr, self.betas[0], self.betas[1], self.eps, target, clip)
            with torch.cuda.device(device):
                _n.check(self._lib.gxa_fit(B, self.D, self.A, HIDDEN, theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr(),
                                           self.count.data_ptr(), obs.data_ptr(), act.data_ptr(), adv.data_ptr(), logp.data_ptr(),
                                           iters, kind, C.cast(hyper, C.c_void_p), self._table.data_ptr(), self.t_sat,
                                           self.workgroups, work.data_ptr(), trace.data_ptr(), ctl.data_ptr(), last.data_ptr(),
                                           _fisher._stream(device)))
            at = 0
            with torch.no_grad():
                for p in self.pi.parameters():
                    p.copy_(theta[at:at + p.numel()].view_as(p))
                    at += p.numel()
        else:
            last[3] = (theta[:self.A].to(torch.float64) + 0.5 + HALF_LOG_2PI).sum()
        return {'loss': trace[0], 'kl': trace[1], 'cf': trace[2], 'stop_iter': ctl[1], 'steps': ctl[2],
                'step': self.count[0].clone(), 'loss_last': last[0], 'kl_last': last[1], 'cf_last': last[2], 'ent': last[3],
                'theta': theta}
