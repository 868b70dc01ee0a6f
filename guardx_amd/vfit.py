"""The closing block of the learners' update() on the device path: `ValueFit(ac.v, lr=vf_lr).fit(obs, ret, iters=train_v_iters)`
is their

    for i in range(train_v_iters):
        vf_optimizer.zero_grad(); loss_v = ((ac.v(obs) - ret)**2).mean(); loss_v.backward(); vf_optimizer.step()

with vf_optimizer = Adam(ac.v.parameters(), lr=vf_lr) (safe_rl_libX trpo/trpo.py:434-439, cpo/cpo.py:563-576, which runs it a
second time for ac.vc on cost_ret, and the same lines of every other learner, PPO included) as one stream-ordered call: two
launches per iteration, no autograd graph, nothing synchronised (libguardx_vfit.so, include/guardx_vfit.h; INTEGRATION.md,
"Value fit on the device path").

The gradient of the loss is taken in closed form over the MLP critic (hidden width 64, tanh, one linear output) and Adam is
torch's single-tensor form.  Vectors are in the order of critic.parameters(): W1 b1 W2 b2 W3 b3.

Not served: mpi_avg_grads (several ranks averaging their gradients), mini-batches (the reference has none), weight decay and
amsgrad.  SCPO's down-sampled vc loss with its softplus head, and the cost critics of usl, lpg and safelayer, are
guardx_amd.cfit's (CostCriticFit).
"""
import ctypes as C

import torch

from . import _closed_loop as _cl
from . import _vfit_native as _n
from . import fisher as _fisher

HIDDEN = _fisher.HIDDEN
MAX_OBS = _fisher.MAX_OBS


def _checked(name, x, shape, device):
    """fisher._checked in ValueFit's name"""
    try:
        return _fisher._checked(name, x, shape, device)
    except ValueError as e:
        raise ValueError(str(e).replace("FisherOperator", "ValueFit", 1)) from None


def _layers(critic):
    """D of a critic the kernel serves, or NotImplementedError in the words of fisher._layers"""
    who = "ValueFit"
    v_net = getattr(critic, 'v_net', None)
    if v_net is None:
        raise NotImplementedError(f"{who} supports a critic with .v_net (trpo_core.MLPCritic)")
    lin = _cl.two_tanh_layers([m for m in v_net if not isinstance(m, torch.nn.Identity)], who, tanh_tail=(
        " and a linear output only (activation=nn.Tanh, output_activation=nn.Identity)"))
    if lin[0].out_features != HIDDEN:
        raise NotImplementedError(f"{who} supports hidden width 64, not {lin[0].out_features}")
    if any(m.bias is None for m in lin):
        raise NotImplementedError(f"{who} supports Linear layers with a bias")
    D = lin[0].in_features
    if D > MAX_OBS:
        raise NotImplementedError(f"{who} supports an observation width <= {MAX_OBS}, not {D}")
    if lin[2].out_features != 1:
        raise NotImplementedError(f"{who} supports one output, not {lin[2].out_features}")
    order = [tuple(p.shape) for p in critic.parameters()]
    if order != [(HIDDEN, D), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (1, HIDDEN), (1,)]:
        raise NotImplementedError(f"{who} supports a critic whose parameters() are v_net's weights and biases")
    return D


def param_count(D, h=HIDDEN):
    return h * D + h + h * h + h + h + 1


def bias_corrections(betas, step0, iters):
    """b1^t, b2^t for t = step0 + 1 .. step0 + iters as Python floats, step by step in turn (what the kernel is handed)"""
    b1, b2 = betas
    return [b ** t for t in range(step0 + 1, step0 + iters + 1) for b in (b1, b2)]


class ValueFit:
    """`critic`: anything with .v_net = Linear/Tanh/Linear/Tanh/Linear[/Identity], hidden width 64, biases, one output,
    D <= 128, whose parameters() are W1 b1 W2 b2 W3 b3: ac.v and ac.vc of the learners.  Built once, where the learner
    builds vf_optimizer: the object owns Adam's moments `m` and `v` (float32, (P,), on the critic's device from the first
    call on), the step count `step` and the workspace, and all of it persists across fit calls as the optimizer's state
    persists across epochs.  `lr`, `betas`, `eps`: torch.optim.Adam's.  `workgroups`: the size of the gradient's grid,
    0 = the default for the device (a test hook; the result depends on it in the last bits only)."""

    def __init__(self, critic, lr, betas=(0.9, 0.999), eps=1e-8, workgroups=0, weight_decay=0.0, amsgrad=False):
        self.D = _layers(critic)
        if weight_decay != 0.0 or amsgrad:
            raise NotImplementedError("ValueFit supports Adam without weight_decay and amsgrad")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr >= 0.0 and self.eps >= 0.0 and all(0.0 <= b < 1.0 for b in self.betas)):
            raise ValueError("ValueFit: lr and eps must not be negative, and betas must lie in [0, 1)")
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError("ValueFit: workgroups must be 0 (the default) .. 4096")
        self.critic, self.workgroups = critic, int(workgroups)
        self.P = param_count(self.D)
        self.step = 0
        self.m = self.v = None
        self._work, self._lib = None, None

    def _batch(self, obs, ret):
        obs = _checked("obs", obs, (None, self.D), None)
        B = int(obs.shape[0])
        if B < 1 or B >= 2 ** 31:
            raise ValueError(f"ValueFit: obs must have 1 .. 2^31 - 1 rows, got {B}")
        ret = _checked("ret", ret, (B,), obs.device)
        return obs, ret, B

    def _workspace(self, B, device):
        """the library, and a workspace for B rows on `device` (kept while it is large enough)"""
        if self._lib is None:
            self._lib = _n.load()
        nbytes = int(self._lib.gxv_work_bytes(B, self.D, self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"ValueFit: {self._lib.gxv_last_error().decode()}")
        if self._work is None or self._work.device != device or self._work.numel() * 8 < nbytes:
            self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        return self._work

    def _theta(self, device):
        return _cl.flatten([m for m in self.critic.v_net if isinstance(m, torch.nn.Linear)], device).contiguous()

    def gradient(self, obs, ret):
        """(g (P,) float32, loss 0-dim float32) of loss_v = ((critic(obs) - ret)**2).mean() at the critic's current
        parameters, on the device: one backward().  Nothing here synchronises."""
        obs, ret, B = self._batch(obs, ret)
        work = self._workspace(B, obs.device)
        theta = self._theta(obs.device)
        g = torch.empty_like(theta)
        loss = torch.empty(1, dtype=torch.float32, device=obs.device)
        _n.check(self._lib.gxv_gradient(B, self.D, HIDDEN, theta.data_ptr(), obs.data_ptr(), ret.data_ptr(), self.workgroups,
                                        work.data_ptr(), g.data_ptr(), loss.data_ptr(), _fisher._stream(obs.device)))
        return g, loss[0]

    def fit(self, obs, ret, iters=80):
        """The learners' loop over `iters` iterations: obs (B, D) and ret (B,) float32, contiguous, on one cuda device.
        The critic's parameters are packed, updated on the device and copied back in place, stream-ordered, so that
        whatever reads the module next (pack_actor_critic) sees them.  -> info, device tensors only: info['loss']
        (iters,) float32, entry i the loss at the parameters before step i (loss[0] is the learners' v_l_old, loss[-1]
        their closing loss_v.item()); info['step'] the optimizer's step count after the call (int64, 0-dim); info['theta']
        the flat parameters after the call.  iters = 0 changes nothing.  Nothing here synchronises."""
        if not (int(iters) == iters and iters >= 0):
            raise ValueError("ValueFit.fit: iters must be a non-negative integer")
        iters = int(iters)
        obs, ret, B = self._batch(obs, ret)
        device = obs.device
        work = self._workspace(B, device)
        if self.m is None or self.m.device != device:
            zeros = lambda: torch.zeros(self.P, dtype=torch.float32, device=device)     # noqa: E731
            self.m, self.v = (zeros(), zeros()) if self.m is None else (self.m.to(device), self.v.to(device))
        theta = self._theta(device)
        loss = torch.empty(iters, dtype=torch.float32, device=device)
        if iters:
            hyper = [self.lr, self.betas[0], self.betas[1], self.eps] + bias_corrections(self.betas, self.step, iters)
            arr = (C.c_double * len(hyper))(*hyper)
            _n.check(self._lib.gxv_fit(B, self.D, HIDDEN, theta.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.step,
                                       obs.data_ptr(), ret.data_ptr(), iters, C.cast(arr, C.c_void_p), self.workgroups,
                                       work.data_ptr(), loss.data_ptr(), _fisher._stream(device)))
            self.step += iters
            at = 0
            with torch.no_grad():
                for p in self.critic.parameters():
                    p.copy_(theta[at:at + p.numel()].view_as(p))
                    at += p.numel()
        return {'loss': loss, 'step': torch.full((), self.step, dtype=torch.int64, device=device), 'theta': theta}
