"""The trust-region step of the TRPO-family learners on the device path: `FisherOperator(ac.pi, data['obs'])` is their
`Hx = lambda x: auto_hession_x(kl_div, ac.pi, x)` (safe_rl_libX trpo/trpo.py:386-404 and the same lines of cpo, pcpo, scpo,
trpolag, trpoipo, trpofac, apo, pdo, safelayer, usl, lpg) as one HIP product, and `.solve(g)` their `cg(Hx, g)` followed
by `s = x_hat' H x_hat`, without a host round trip (libguardx_fisher.so, include/guardx_fisher.h; INTEGRATION.md, "Trust-region
step on the device path").

The Hessian of diagonal_gaussian_kl (trpo_core.py:12-22) at the old policy is taken in closed form: a Gauss-Newton term
J' diag(1 / (exp(2 log_std) + eps)) J / B over mu_net's parameters plus a diagonal block for log_std.  It is evaluated at
mu_old = mu_net(obs), which is what the learners' buffers hold.  Vectors are in the order of ac.pi.parameters(), log_std
first, as get_net_param_np_vec has them.
"""
import ctypes as C

import numpy as np
import torch

from . import _closed_loop as _cl
from . import _fisher_native as _n

HIDDEN = 64
MAX_OBS, MAX_ACT = 128, 16


def _layers(pi):
    """(D, A) of an actor the kernel serves, or NotImplementedError"""
    who = "FisherOperator"
    mu_net, log_std = getattr(pi, 'mu_net', None), getattr(pi, 'log_std', None)
    if mu_net is None or log_std is None:
        raise NotImplementedError(f"{who} supports a Gaussian actor with .mu_net and .log_std (trpo_core.MLPGaussianActor)")
    lin = _cl.two_tanh_layers([m for m in mu_net if not isinstance(m, torch.nn.Identity)], who, tanh_tail=(
        " and a linear output only (activation=nn.Tanh, output_activation=nn.Identity)"))
    if lin[0].out_features != HIDDEN:
        raise NotImplementedError(f"{who} supports hidden width 64, not {lin[0].out_features}")
    if any(m.bias is None for m in lin):
        raise NotImplementedError(f"{who} supports Linear layers with a bias")
    D, A = lin[0].in_features, lin[2].out_features
    if D > MAX_OBS:
        raise NotImplementedError(f"{who} supports an observation width <= {MAX_OBS}, not {D}")
    if A % 2 or A > MAX_ACT:
        raise NotImplementedError(f"{who} supports an even action width <= {MAX_ACT}, not {A}")
    if torch.as_tensor(log_std).numel() != A:
        raise NotImplementedError(f"log_std has {torch.as_tensor(log_std).numel()} entries, mu_net {A} outputs")
    order = [tuple(p.shape) for p in pi.parameters()]
    if order != [(A,), (HIDDEN, D), (HIDDEN,), (HIDDEN, HIDDEN), (HIDDEN,), (A, HIDDEN), (A,)]:
        raise NotImplementedError(f"{who} supports an actor whose parameters() are log_std, then mu_net's weights and biases")
    return D, A


def flat_params(pi, device=None):
    """The learners' flat vector of `pi` (get_net_param_np_vec: torch.cat of parameters(), log_std first) as a float32
    tensor on `device` (default: where the parameters are)."""
    flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in pi.parameters()])
    return flat.to(device) if device is not None else flat


def param_count(D, A, h=HIDDEN):
    return A + h * D + h + h * h + h + A * h + A


def _stream(device):
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def _checked(name, x, shape, device):
    """x as it is if it is a contiguous float32 tensor of `shape` (None: any size) on `device` (None: any cuda device);
    ValueError otherwise, before anything is launched"""
    if not (torch.is_tensor(x) and x.dtype == torch.float32):
        raise ValueError(f"FisherOperator: {name} must be a float32 tensor")
    if x.dim() != len(shape) or any(want is not None and have != want for have, want in zip(x.shape, shape)):
        want = "(" + ", ".join("B" if n is None else str(n) for n in shape) + ("," if len(shape) == 1 else "") + ")"
        raise ValueError(f"FisherOperator: {name} must be {want}, got {tuple(x.shape)}")
    if not x.is_contiguous():
        raise ValueError(f"FisherOperator: {name} must be contiguous")
    if not x.is_cuda or (device is not None and x.device != device):
        raise ValueError(f"FisherOperator: {name} lives on {x.device}; it must be on " +
                         ("a cuda device" if device is None else f"{device}, where obs is"))
    return x


class FisherOperator:
    """y = H x (+ damping x) of the KL of `pi` at its own parameters over the rows of `obs`.

    `pi`: anything with .mu_net (Linear/Tanh/Linear/Tanh/Linear[/Identity], hidden width 64) and .log_std; packed once, at
    construction.  `obs`: (B, D) float32, contiguous, on a cuda device: what *_rollout_batch(...)['obs'] is; it is kept by
    reference, not copied.  `eps`: the learners' EPS.  `damping`: y += damping x (the reference has none).
    `workgroups`: the size of the product's grid, 0 = the default for the device (a test hook; the result depends on it
    in the last bits only).

    F(x): x a cuda float32 (P,) tensor -> a new cuda tensor; a numpy vector -> a numpy float32 vector (a drop-in for
    the learners' Hx).  F.solve(g, iters): the learners' cg and s, all on the device."""

    def __init__(self, pi, obs, eps=1e-8, damping=0.0, workgroups=0):
        D, A = _layers(pi)
        _checked("obs", obs, (None, D), None)
        if obs.shape[0] < 1 or obs.shape[0] >= 2 ** 31:
            raise ValueError(f"FisherOperator: obs must have 1 .. 2^31 - 1 rows, got {obs.shape[0]}")
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError("FisherOperator: workgroups must be 0 (the default) .. 4096")
        self.obs, self.B, self.D, self.A = obs, int(obs.shape[0]), D, A
        self.P = param_count(D, A)
        self.eps, self.damping, self.workgroups = float(eps), float(damping), int(workgroups)
        self.device = obs.device
        self.theta = flat_params(pi, self.device).contiguous()
        self._lib = _n.load()
        nbytes = int(self._lib.gxf_work_bytes(self.B, D, A, self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"FisherOperator: {_n.load().gxf_last_error().decode()}")
        self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)

    def _vector(self, name, x):
        return _checked(name, x, (self.P,), self.device)

    def __call__(self, x):
        if isinstance(x, np.ndarray):
            if x.shape != (self.P,):
                raise ValueError(f"FisherOperator: x must be ({self.P},), got {x.shape}")
            xd = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(self.device)
            return self(xd).cpu().numpy()
        x = self._vector("x", x)
        y = torch.empty_like(x)
        _n.check(self._lib.gxf_fvp(self.B, self.D, self.A, HIDDEN, self.obs.data_ptr(), self.theta.data_ptr(), x.data_ptr(),
                                   self.eps, self.damping, self.workgroups, self._work.data_ptr(), y.data_ptr(),
                                   _stream(self.device)))
        return y

    def solve(self, g, iters=100):
        """The learners' x_hat = cg(Hx, g, cg_iters=iters) and s = x_hat' H x_hat: (x_hat (P,), s 0-dim float32,
        info) with info['iters'] (int32: iterations done before the early stop) and info['r_dot'] (the final r.r), all on
        the device; nothing here synchronises.  g = 0 gives x_hat = 0 after 0 iterations."""
        g = self._vector("g", g)
        if not (int(iters) == iters and iters >= 0):
            raise ValueError("FisherOperator.solve: iters must be a non-negative integer")
        x_hat = torch.empty_like(g)
        scal = torch.empty(2, dtype=torch.float32, device=self.device)
        done = torch.empty(1, dtype=torch.int32, device=self.device)
        _n.check(self._lib.gxf_cg(self.B, self.D, self.A, HIDDEN, self.obs.data_ptr(), self.theta.data_ptr(), g.data_ptr(),
                                  self.eps, self.damping, int(iters), self.workgroups, self._work.data_ptr(),
                                  x_hat.data_ptr(), scal.data_ptr(), scal.data_ptr() + 4, done.data_ptr(),
                                  _stream(self.device)))
        return x_hat, scal[0], {'iters': done[0], 'r_dot': scal[1]}
