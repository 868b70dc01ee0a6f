"""The safety critics' fit on the device path: `CostCriticFit(ac.ccritic, lr=ccritic_lr).fit(x, target, iters=80, ...)` is the
learners'

    for i in range(train_ccritic_iters):
        ccritic_optimizer.zero_grad(); loss = compute_loss_ccritic(data); loss.backward(); ccritic_optimizer.step()

with ccritic_optimizer = Adam(ac.ccritic.parameters(), lr=ccritic_lr), as one stream-ordered call: two launches per iteration,
no autograd graph, no boolean index, nothing synchronised (libguardx_cfit.so, include/guardx_cfit.h; INTEGRATION.md,
"Safety-critic fit on the device path").  Three heads over the MLP (hidden width 64, tanh), z its output:

    'softplus'  f = Softplus(z)              usl, lpg (usl/usl.py:378-383, 449-454, lpg/lpg.py:386-391, 457-462:
                                             x = cat(obs, act_safe), target = targetc) and scpo's compute_loss_vc
                                             (scpo/scpo.py:419-450: x = cat(obs, M), target = cost_ret)
    'dot'       f = z . act + offset         safelayer (safelayer/safelayer.py:384-418: x = obs, act = act_safe,
                                             offset = prev_cost, target = cost)
    'identity'  f = z                        vfit's loss, under row weights

and the loss L = sum_i w_i (f_i - y_i)^2 / W, W = sum_i w_i (w_i = 1 without weights: the plain mean).  The reference's
down-sampling (keep every row with target > 0 and as many of the rows with target == 0, drawn afresh each round) is the 0 / 1
weight table of `downsample_weights`, one row per iteration: a row of weight 0 is selected out of the loss and of every
gradient entry, whatever it holds (NaN and Inf included), as the reference's indexing takes it out.

W == 0 (a weight row that selects nothing) is the reference's mean of an empty selection: that round's loss and gradient are
NaN and Adam carries the NaN into the parameters, m and v.  The reference does the same when a batch has no row the loss
keeps: a batch of zero targets without a positive one has frac = 0, keeps int(n_zero * 0) = 0 rows and takes the mean of
nothing, and `downsample_weights` returns rows of zeros for it, as it must.

Vectors are in the order of the module's parameters(): W1 b1 W2 b2 W3 b3.

Not served: mpi_avg_grads (several ranks averaging their gradients), hidden widths other than 64, mini-batches, weight decay
and amsgrad.
"""
import ctypes as C

import torch

from . import _cfit_native as _n
from . import _closed_loop as _cl
from . import fisher as _fisher
from .vfit import bias_corrections

HIDDEN = _fisher.HIDDEN
MAX_IN = _fisher.MAX_OBS
HEADS = ("identity", "softplus", "dot")
_HEAD_ID = {"identity": _n.GXQ_HEAD_IDENTITY, "softplus": _n.GXQ_HEAD_SOFTPLUS, "dot": _n.GXQ_HEAD_DOT}
_WHO = "CostCriticFit"


def _checked(name, x, shape, device):
    """fisher._checked in CostCriticFit's name"""
    try:
        return _fisher._checked(name, x, shape, device)
    except ValueError as e:
        raise ValueError(str(e).replace("FisherOperator", _WHO, 1).replace("where obs is", "where x is")) from None


def _in_my_words(pack, theirs, *args, **kw):
    """what the packer `pack` refuses, in CostCriticFit's name"""
    try:
        return pack(*args, **kw)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace(theirs, _WHO)) from None


def _ends_in_softplus(net):
    mods = [m for m in net if not isinstance(m, torch.nn.Identity)]
    return bool(mods) and isinstance(mods[-1], torch.nn.Softplus)


def _layers(critic):
    """(head, net, Din, A) of a module the kernel serves, or NotImplementedError in the words of the packer that serves the
    same module to its rollout (usl.pack_q_critic, safelayer.pack_g_net, Engine.pack_critic)"""
    from . import safelayer as _sl, usl as _usl
    from .engine import Engine
    net = next((getattr(critic, k) for k in ('c_net', 'g_net', 'v_net') if getattr(critic, k, None) is not None), None)
    if net is not None and any(isinstance(m, torch.nn.Linear) and m.bias is None for m in net):
        raise NotImplementedError(f"{_WHO} supports Linear layers with a bias")     # the packers take the bias for granted
    if getattr(critic, 'c_net', None) is not None:
        head = 'softplus'
        _in_my_words(_usl.pack_q_critic, "rollout_usl", critic)
    elif getattr(critic, 'g_net', None) is not None:
        head = 'dot'
        _in_my_words(_sl.pack_g_net, "rollout_safelayer", critic)
    elif getattr(critic, 'v_net', None) is not None:
        head = 'softplus' if _ends_in_softplus(net) else 'identity'
        theirs = "pack_critic(output='softplus')" if head == 'softplus' else "the cost critic pass"
        try:
            _in_my_words(Engine.pack_critic, theirs, critic, output=head)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("the cost critic pass", _WHO)) from None
    else:
        raise NotImplementedError(f"{_WHO} supports a module with .c_net (usl, lpg), .g_net (safelayer) or .v_net (scpo's "
                                  "MLPMaxCostCritic, trpo_core.MLPCritic)")
    lin = [m for m in net if isinstance(m, torch.nn.Linear)]
    if lin[0].out_features != HIDDEN:
        raise NotImplementedError(f"{_WHO} supports hidden width 64, not {lin[0].out_features}")
    Din, A = lin[0].in_features, lin[2].out_features
    if Din > MAX_IN:
        raise NotImplementedError(f"{_WHO} supports an input width <= {MAX_IN}, not {Din}")
    order = [tuple(p.shape) for p in critic.parameters()]
    if order != [(HIDDEN, Din), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (A, HIDDEN), (A,)]:
        raise NotImplementedError(f"{_WHO} supports a module whose parameters() are its network's weights and biases")
    return head, lin, Din, A


def param_count(Din, A=1, h=HIDDEN):
    return h * Din + h + h * h + h + A * h + A


def downsample_weights(target, iters, generator=None):
    """The reference's down-sampling (safelayer/safelayer.py:392-413, scpo/scpo.py:425-446) as an (iters, B) float32 table of
    0 / 1 on target's device, one row per round of the fit.  With n_pos = (target > 0).sum() and n_zero = (target == 0).sum():
    if n_zero == 0 or n_pos / n_zero >= 1 every row of the batch gets 1 (the reference takes the whole batch, rows with
    negative or NaN targets included); otherwise 1 goes on the rows with target > 0 and on exactly
    k = floor(n_zero * (n_pos / n_zero)) (float64, the reference's int(len * frac), which can be n_pos - 1) of the rows with
    target == 0, drawn uniformly without replacement and independently per iteration, and 0 on every other row.  The k rows
    are those of smallest rank among per-row random keys, so the count is exact even where keys tie.  Pure torch, CPU
    tensors included; k stays a device value and nothing synchronises.  The random stream is torch's (`generator`, or the
    device's default), not numpy's RandomState: the distribution is the reference's, the draws are not."""
    if not torch.is_tensor(target) or target.dim() != 1:
        raise ValueError("downsample_weights: target must be a (B,) tensor")
    if not (int(iters) == iters and iters >= 0):
        raise ValueError("downsample_weights: iters must be a non-negative integer")
    iters, B, dev = int(iters), int(target.shape[0]), target.device
    pos, zero = target > 0, target == 0
    n_pos, n_zero = pos.sum().to(torch.float64), zero.sum().to(torch.float64)
    frac = n_pos / n_zero                                        # n_zero == 0: inf or nan, and `whole` decides
    whole = (n_zero == 0) | (frac >= 1.0)
    k = torch.floor(n_zero * frac)
    keys = torch.rand((iters, B), generator=generator, device=dev, dtype=torch.float32)
    keys = torch.where(zero.unsqueeze(0), keys, torch.full((), 2.0, dtype=torch.float32, device=dev))
    order = keys.argsort(dim=1, stable=True)                     # the rows with target == 0 first, in key order
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(B, device=dev).unsqueeze(0).expand(iters, B))
    keep = whole | pos.unsqueeze(0) | (zero.unsqueeze(0) & (rank.to(torch.float64) < k))
    return keep.to(torch.float32)


def softplus_probe(x):
    """(Softplus(x), Softplus'(x)) as the gradient kernel evaluates them, for x a float32 device tensor (gxq_softplus_probe)."""
    if not (torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32):
        raise ValueError("softplus_probe: x must be a float32 device tensor")
    x = x.contiguous()
    if x.numel() >= 2 ** 31:
        raise ValueError("softplus_probe: more than 2^31 - 1 values")
    f, df = torch.empty_like(x), torch.empty_like(x)
    lib = _n.load()
    _n.check(lib.gxq_softplus_probe(x.numel(), x.data_ptr(), f.data_ptr(), df.data_ptr(), _fisher._stream(x.device)))
    return f, df


class CostCriticFit:
    """`critic`: ac.ccritic of usl / lpg (.c_net = Linear/Tanh/Linear/Tanh/Linear/Softplus(beta=1, threshold=20): head
    'softplus'), of safelayer (.g_net = Linear/Tanh/Linear/Tanh/Linear[/Identity] with an even number <= 16 of outputs: head
    'dot'), scpo's ac.vc (.v_net ending in the same Softplus: 'softplus') or a critic with a linear .v_net ('identity');
    hidden width 64, biases, input width <= 128, parameters() = W1 b1 W2 b2 W3 b3.  The head is read off the module; `head=`,
    when given, is checked against it.  Built once, where the learner builds ccritic_optimizer: the object owns Adam's
    moments `m` and `v` (float32, (P,)), the step count `step` and the workspace, and all of it persists across fit calls as
    the optimizer's state persists across epochs.  `lr`, `betas`, `eps`: torch.optim.Adam's.  `workgroups`: the size of the
    gradient's grid, 0 = the default for the device (a test hook; the result depends on it in the last bits only)."""

    def __init__(self, critic, lr, betas=(0.9, 0.999), eps=1e-8, workgroups=0, weight_decay=0.0, amsgrad=False, head=None):
        if head is not None and head not in HEADS:
            raise ValueError(f"{_WHO}: head must be one of {HEADS}, got {head!r}")
        self.head, self._lin, self.Din, self.A = _layers(critic)
        if head is not None and head != self.head:
            raise NotImplementedError(f"{_WHO}: head={head!r} was asked for, the module's head is {self.head!r}")
        if weight_decay != 0.0 or amsgrad:
            raise NotImplementedError(f"{_WHO} supports Adam without weight_decay and amsgrad")
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        if not (self.lr >= 0.0 and self.eps >= 0.0 and all(0.0 <= b < 1.0 for b in self.betas)):
            raise ValueError(f"{_WHO}: lr and eps must not be negative, and betas must lie in [0, 1)")
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError(f"{_WHO}: workgroups must be 0 (the default) .. 4096")
        self.critic, self.workgroups = critic, int(workgroups)
        self.P = param_count(self.Din, self.A)
        self.step = 0
        self.m = self.v = None
        self._work, self._lib = None, None

    def _batch(self, x, target, weight, act, offset, iters):
        x = _checked("x", x, (None, self.Din), None)
        B = int(x.shape[0])
        if B < 1 or B >= 2 ** 31:
            raise ValueError(f"{_WHO}: x must have 1 .. 2^31 - 1 rows, got {B}")
        dev = x.device
        target = _checked("target", target, (B,), dev)
        stride = 0
        if weight is not None:
            if iters is not None and torch.is_tensor(weight) and weight.dim() == 2:
                weight, stride = _checked("weight", weight, (iters, B), dev), B
            else:
                weight = _checked("weight", weight, (B,), dev)
        if self.head == 'dot':
            if act is None:
                raise ValueError(f"{_WHO}: head 'dot' needs act (safelayer's act_safe)")
            act = _checked("act", act, (B, self.A), dev)
            if offset is not None:
                offset = _checked("offset", offset, (B,), dev)
        elif act is not None or offset is not None:
            raise ValueError(f"{_WHO}: act and offset belong to head 'dot'; this module's head is {self.head!r}")
        return x, target, weight, stride, act, offset, B

    def _workspace(self, B, device):
        """the library, and a workspace for B rows on `device` (kept while it is large enough)"""
        if self._lib is None:
            self._lib = _n.load()
        nbytes = int(self._lib.gxq_work_bytes(B, self.Din, self.A, _HEAD_ID[self.head], self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"{_WHO}: {self._lib.gxq_last_error().decode()}")
        if self._work is None or self._work.device != device or self._work.numel() * 8 < nbytes:
            self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=device)
        return self._work

    def _theta(self, device):
        return _cl.flatten(self._lin, device).contiguous()

    @staticmethod
    def _ptr(t):
        return None if t is None else t.data_ptr()

    def gradient(self, x, target, weight=None, act=None, offset=None):
        """(g (P,) float32, loss 0-dim float32, W 0-dim float64) of the loss at the module's current parameters, on the device:
        one backward().  weight: None or (B,).  Nothing here synchronises."""
        x, target, weight, _, act, offset, B = self._batch(x, target, weight, act, offset, None)
        work = self._workspace(B, x.device)
        theta = self._theta(x.device)
        g = torch.empty_like(theta)
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        W = torch.empty(1, dtype=torch.float64, device=x.device)
        _n.check(self._lib.gxq_gradient(B, self.Din, self.A, HIDDEN, _HEAD_ID[self.head], theta.data_ptr(), x.data_ptr(),
                                        target.data_ptr(), self._ptr(weight), self._ptr(act), self._ptr(offset), self.workgroups,
                                        work.data_ptr(), g.data_ptr(), loss.data_ptr(), W.data_ptr(), _fisher._stream(x.device)))
        return g, loss[0], W[0]

    def fit(self, x, target, iters=80, weight=None, act=None, offset=None):
        """The learners' loop over `iters` iterations: x (B, Din), target (B,), and for head 'dot' act (B, A) and offset (B,)
        or None (zeros), float32, contiguous, on one cuda device.  weight: None (the plain mean), (B,) (the same weights
        every round) or (iters, B) (row i for round i: downsample_weights).  The module's parameters are packed, updated on
        the device and copied back in place, stream-ordered, so that whatever reads the module next (Engine.pack_q_critic,
        pack_g_net, pack_critic) sees them.  -> info, device tensors only: info['loss'] (iters,) float32, entry i the loss
        at the parameters before step i; info['weight'] (iters,) float64, each round's W; info['step'] the optimizer's step
        count after the call (int64, 0-dim); info['theta'] the flat parameters after the call.  A round whose W is 0 turns
        the parameters into NaN (the module's docstring).  iters = 0 changes nothing.  Nothing here synchronises."""
        if not (int(iters) == iters and iters >= 0):
            raise ValueError(f"{_WHO}.fit: iters must be a non-negative integer")
        iters = int(iters)
        x, target, weight, stride, act, offset, B = self._batch(x, target, weight, act, offset, iters)
        device = x.device
        work = self._workspace(B, device)
        if self.m is None or self.m.device != device:
            zeros = lambda: torch.zeros(self.P, dtype=torch.float32, device=device)     # noqa: E731
            self.m, self.v = (zeros(), zeros()) if self.m is None else (self.m.to(device), self.v.to(device))
        theta = self._theta(device)
        loss = torch.empty(iters, dtype=torch.float32, device=device)
        W = torch.empty(iters, dtype=torch.float64, device=device)
        if iters:
            hyper = [self.lr, self.betas[0], self.betas[1], self.eps] + bias_corrections(self.betas, self.step, iters)
            arr = (C.c_double * len(hyper))(*hyper)
            _n.check(self._lib.gxq_fit(B, self.Din, self.A, HIDDEN, _HEAD_ID[self.head], theta.data_ptr(), self.m.data_ptr(),
                                       self.v.data_ptr(), self.step, x.data_ptr(), target.data_ptr(), self._ptr(weight), stride,
                                       self._ptr(act), self._ptr(offset), iters, C.cast(arr, C.c_void_p), self.workgroups,
                                       work.data_ptr(), loss.data_ptr(), W.data_ptr(), _fisher._stream(device)))
            self.step += iters
            at = 0
            with torch.no_grad():
                for p in self.critic.parameters():
                    p.copy_(theta[at:at + p.numel()].view_as(p))
                    at += p.numel()
        return {'loss': loss, 'weight': W, 'step': torch.full((), self.step, dtype=torch.int64, device=device), 'theta': theta}
