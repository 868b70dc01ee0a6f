"""The backtracking line search of the TRPO-family learners on the device path: `LineSearch(ac.pi, data).search(x_direction,
target_kl)` is their `for j in range(backtrack_iters)` loop (safe_rl_libX trpo/trpo.py:406-431 and the same lines of trpolag,
trpoipo, trpofac, safelayer, usl, lpg; with `cost_margin` and `need_loss`, cpo/cpo.py:527-560, scpo and pdo) as one
stream-ordered call: no deep copy of the actor, no parameter vector on the host, no `.item()` per candidate
(libguardx_linesearch.so, include/guardx_linesearch.h; INTEGRATION.md, "Line search on the device path").

Each candidate theta - coeff**j x_direction is evaluated over the whole batch: the mean KL to the old policy (mu and logstd of
the buffer's rows), pi_l = -mean(ratio adv), surr_cost = mean(ratio adc) and approx_kl = mean(logp_old - logp).  The first
one that meets the learners' conditions is accepted on the device; the launches queued behind it do nothing.  Vectors are in
the order of ac.pi.parameters(), log_std first, as get_net_param_np_vec has them (fisher.flat_params).

A loss with a Lagrangian term, trpolag's and trpofac's loss_pi = -mean(ratio adv) + lmd mean(ratio adc) (trpolag.py:380-394),
is linear in ratio: pass adv - lmd adc as adv.  apo's variance loss (apo.py:402) is not, and is not served.
"""
import ctypes as C

import torch

from . import _linesearch_native as _n
from . import fisher as _fisher

HIDDEN = _fisher.HIDDEN
MEANS = ('kl', 'pi_l', 'surr_cost', 'approx_kl')     # the order of every row of four


def _checked(name, x, shape, device):
    """fisher._checked in LineSearch's name"""
    try:
        return _fisher._checked(name, x, shape, device)
    except ValueError as e:
        raise ValueError(str(e).replace("FisherOperator", "LineSearch", 1)) from None


def assign_flat_params(pi, theta):
    """The learners' assign_net_param_from_flat(theta, pi) for a flat device tensor: a copy per parameter, on the device, in
    the order of pi.parameters()."""
    theta = torch.as_tensor(theta)
    params = list(pi.parameters())
    if theta.dim() != 1 or theta.numel() != sum(p.numel() for p in params):
        raise ValueError(f"assign_flat_params: theta must be ({sum(p.numel() for p in params)},), got {tuple(theta.shape)}")
    at = 0
    with torch.no_grad():
        for p in params:
            p.copy_(theta[at:at + p.numel()].view_as(p))
            at += p.numel()


class LineSearch:
    """`pi`: an actor FisherOperator serves (.mu_net Linear/Tanh/Linear/Tanh/Linear[/Identity], hidden width 64, and
    .log_std); its parameters are read at every call, so one LineSearch serves an epoch's update.  `data`: a mapping with
    obs (B, D), act (B, A), adv (B,), logp (B,), mu (B, A), logstd (B, A) and, optionally, adc (B,), float32, contiguous,
    on one cuda device: what *_rollout_batch gives; kept by reference, not copied.  SCPO passes cat(obs, M) as obs.
    `workgroups`: the size of the grid, 0 = the default for the device (a test hook; the result depends on it in the last
    bits only)."""

    def __init__(self, pi, data, workgroups=0):
        try:
            D, A = _fisher._layers(pi)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("FisherOperator", "LineSearch")) from None
        for key in ('obs', 'act', 'adv', 'logp', 'mu', 'logstd'):
            if key not in data:
                raise ValueError(f"LineSearch: data has no '{key}'")
        obs = _checked("obs", data['obs'], (None, D), None)
        B = int(obs.shape[0])
        if B < 1 or B >= 2 ** 31:
            raise ValueError(f"LineSearch: obs must have 1 .. 2^31 - 1 rows, got {B}")
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError("LineSearch: workgroups must be 0 (the default) .. 4096")
        self.device = obs.device
        self.pi, self.obs, self.B, self.D, self.A = pi, obs, B, D, A
        self.act = _checked("act", data['act'], (B, A), self.device)
        self.adv = _checked("adv", data['adv'], (B,), self.device)
        self.logp = _checked("logp", data['logp'], (B,), self.device)
        self.mu = _checked("mu", data['mu'], (B, A), self.device)
        self.logstd = _checked("logstd", data['logstd'], (B, A), self.device)
        self.adc = _checked("adc", data['adc'], (B,), self.device) if data.get('adc') is not None else None
        self.P = _fisher.param_count(D, A)
        self.workgroups = int(workgroups)
        self._lib = _n.load()
        nbytes = int(self._lib.gxb_work_bytes(B, D, A, self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"LineSearch: {self._lib.gxb_last_error().decode()}")
        self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)

    def _batch(self):
        return (self.obs.data_ptr(), self.act.data_ptr(), self.adv.data_ptr(), self.logp.data_ptr(), self.mu.data_ptr(),
                self.logstd.data_ptr(), self.adc.data_ptr() if self.adc is not None else None)

    def _theta(self):
        return _fisher.flat_params(self.pi, self.device).contiguous()

    def _criterion(self, name, v):
        """a Python number, or a 0-dim tensor on the device -> 0-dim float64 on the device, without a synchronisation"""
        if torch.is_tensor(v):
            if v.numel() != 1:
                raise ValueError(f"LineSearch: {name} must be a number or a tensor of one element, got {tuple(v.shape)}")
            if v.device != self.device:
                raise ValueError(f"LineSearch: {name} lives on {v.device}; it must be a number or on {self.device}, where obs is")
            return v.detach().reshape(()).to(torch.float64)
        return float(v)

    def evaluate(self, x_direction, steps):
        """(len(steps), 4) float64 on the device: kl, pi_l, surr_cost, approx_kl of theta - t x_direction for every t of
        `steps` (Python numbers), unconditionally.  Nothing here synchronises."""
        steps = [float(t) for t in steps]
        if not steps:
            raise ValueError("LineSearch.evaluate: steps must not be empty")
        d = _checked("x_direction", x_direction, (self.P,), self.device)
        out = torch.empty((len(steps), 4), dtype=torch.float64, device=self.device)
        theta = self._theta()
        arr = (C.c_double * len(steps))(*steps)
        _n.check(self._lib.gxb_evaluate(self.B, self.D, self.A, HIDDEN, theta.data_ptr(), d.data_ptr(), *self._batch(),
                                        len(steps), C.cast(arr, C.c_void_p), self.workgroups, self._work.data_ptr(),
                                        out.data_ptr(), _fisher._stream(self.device)))
        return out

    def search(self, x_direction, target_kl, cost_margin=None, need_loss=True, coeff=0.8, iters=100):
        """The learners' loop: the first j < iters whose candidate theta - coeff**j x_direction has
            kl <= target_kl  and  (not need_loss or pi_l <= pi_l_old)  and  (no adc or surr_cost - surr_cost_old <= cost_margin)
        with pi_l_old and surr_cost_old the same means at theta itself, evaluated here.  `target_kl`, `cost_margin` (CPO's
        max(-c, -cost_reduction)) and `need_loss` (CPO's optim_case > 1) are Python numbers or 0-dim tensors on the device.
        -> (theta_new (P,) float32, info): theta_new is the accepted candidate, or theta itself when none is accepted;
        info holds `accepted` (int32, -1 for none), `kl`, `pi_l`, `surr_cost`, `approx_kl` at theta_new, `pi_l_old`,
        `surr_cost_old` (float64) and `trace` ((iters + 1, 4) float64: row 0 at theta, row j + 1 candidate j, NaN where
        nothing was evaluated), all on the device; nothing here synchronises."""
        if not (int(iters) == iters and iters >= 0):
            raise ValueError("LineSearch.search: iters must be a non-negative integer")
        iters = int(iters)
        if self.adc is not None and cost_margin is None:
            raise ValueError("LineSearch.search: data has adc, so cost_margin must be given")
        if self.adc is None and cost_margin is not None:
            raise ValueError("LineSearch.search: cost_margin needs data['adc']")
        crit = [self._criterion("target_kl", target_kl), self._criterion("cost_margin", 0.0 if cost_margin is None else cost_margin),
                self._criterion("need_loss", need_loss)]
        coeff = float(coeff)
        d = _checked("x_direction", x_direction, (self.P,), self.device)
        # numbers become 0-dim tensors through a fill kernel (its value travels as a kernel argument): no copy from the host
        crit = torch.stack([v if torch.is_tensor(v) else torch.full((), v, dtype=torch.float64, device=self.device) for v in crit])
        steps = [coeff ** j for j in range(iters)] or [1.0]
        arr = (C.c_double * len(steps))(*steps)
        theta = self._theta()
        theta_new = torch.empty_like(theta)
        accepted = torch.empty(1, dtype=torch.int32, device=self.device)
        means = torch.empty(6, dtype=torch.float64, device=self.device)
        trace = torch.full((iters + 1, 4), float('nan'), dtype=torch.float64, device=self.device)
        _n.check(self._lib.gxb_search(self.B, self.D, self.A, HIDDEN, theta.data_ptr(), d.data_ptr(), *self._batch(), iters,
                                      C.cast(arr, C.c_void_p), crit.data_ptr(), self.workgroups, self._work.data_ptr(),
                                      theta_new.data_ptr(), accepted.data_ptr(), means.data_ptr(), trace.data_ptr(),
                                      _fisher._stream(self.device)))
        info = {'accepted': accepted[0], 'kl': means[0], 'pi_l': means[1], 'surr_cost': means[2], 'approx_kl': means[3],
                'pi_l_old': means[4], 'surr_cost_old': means[5], 'trace': trace}
        return theta_new, info
