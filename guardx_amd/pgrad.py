"""What opens the TRPO family's update() on the device path: `SurrogateGradient(ac.pi, data).gradient()` is their
`g = auto_grad(loss_pi, ac.pi)` and, with data['adc'], CPO's `b = auto_grad(surr_cost, ac.pi)` (safe_rl_libX trpo/trpo.py and
the same lines of trpolag, trpoipo, trpofac, safelayer, usl, lpg; cpo/cpo.py:445-446, scpo and pdo) from one forward pass (two past D = 72)
and without an autograd graph; `cpo_direction(F, g, b, c, target_kl)` is cpo/cpo.py:459-525, the two solves and the ladder of
`if`s that picks optim_case, lam, nu and x_direction, as stream-ordered device work, and `trpo_direction(F, g, target_kl)` the
one line trpo has in its place (libguardx_pgrad.so, include/guardx_pgrad.h; INTEGRATION.md, "Surrogate gradients and the
CPO step on the device path").

The gradients are taken in closed form over the Gaussian MLP actor (hidden width 64, tanh, a linear mean, a free log_std);
ratio = exp(logp - logp_old) is computed, not taken as 1.  Vectors are in the order of ac.pi.parameters(), log_std first, as
get_net_param_np_vec has them (fisher.flat_params).

A loss with a Lagrangian term, trpolag's and trpofac's loss_pi = -mean(ratio adv) + lmd mean(ratio adc), is linear in the
row weight: pass adv - lmd adc as adv, as for the line search.

Not served: mpi_avg_grads (several ranks averaging their gradients), apo's variance loss, pcpo's direction (its ladder
projects with H^-1 b onto the constraint instead of solving CPO's dual).  PPO's clipped loss and its Adam loop on the actor
are guardx_amd.pifit: the same kernel with a clipped row weight.
"""
import torch

from . import _pgrad_native as _n
from . import fisher as _fisher

HIDDEN = _fisher.HIDDEN
EPS = 1e-8
DIRECTION = ('lam', 'nu', 'q', 'r', 's', 'A', 'B')      # the order of gxg_cpo_direction's seven float64


def _checked(name, x, shape, device, who="SurrogateGradient"):
    """fisher._checked in this module's names"""
    try:
        return _fisher._checked(name, x, shape, device)
    except ValueError as e:
        raise ValueError(str(e).replace("FisherOperator", who, 1)) from None


def _scalar(who, name, v, device):
    """a Python number, or a tensor of one element on the device -> 0-dim float64 on the device, without a synchronisation"""
    if torch.is_tensor(v):
        if v.numel() != 1:
            raise ValueError(f"{who}: {name} must be a number or a tensor of one element, got {tuple(v.shape)}")
        if v.device != device:
            raise ValueError(f"{who}: {name} lives on {v.device}; it must be a number or on {device}, where the vectors are")
        return v.detach().reshape(()).to(torch.float64)
    return torch.full((), float(v), dtype=torch.float64, device=device)     # a fill kernel: no copy from the host


class SurrogateGradient:
    """`pi`: an actor FisherOperator serves (.mu_net Linear/Tanh/Linear/Tanh/Linear[/Identity], hidden width 64, D <= 128, an
    even A <= 16, and .log_std); its parameters are read at every call.  `data`: a mapping with obs (B, D), act (B, A),
    adv (B,), logp (B,) and, optionally, adc (B,), float32, contiguous, on one cuda device: what *_rollout_batch gives and
    LineSearch takes (mu and logstd are not needed); kept by reference, not copied.  `workgroups`: the size of the grid,
    0 = the default for the device (a test hook; the result depends on it in the last bits only)."""

    def __init__(self, pi, data, workgroups=0):
        try:
            D, A = _fisher._layers(pi)
        except NotImplementedError as e:
            raise NotImplementedError(str(e).replace("FisherOperator", "SurrogateGradient")) from None
        if not (int(workgroups) == workgroups and 0 <= workgroups <= 4096):
            raise ValueError("SurrogateGradient: workgroups must be 0 (the default) .. 4096")
        for key in ('obs', 'act', 'adv', 'logp'):
            if key not in data:
                raise ValueError(f"SurrogateGradient: data has no '{key}'")
        obs = _checked("obs", data['obs'], (None, D), None)
        B = int(obs.shape[0])
        if B < 1 or B >= 2 ** 31:
            raise ValueError(f"SurrogateGradient: obs must have 1 .. 2^31 - 1 rows, got {B}")
        self.device = obs.device
        self.pi, self.obs, self.B, self.D, self.A = pi, obs, B, D, A
        self.act = _checked("act", data['act'], (B, A), self.device)
        self.adv = _checked("adv", data['adv'], (B,), self.device)
        self.logp = _checked("logp", data['logp'], (B,), self.device)
        self.adc = _checked("adc", data['adc'], (B,), self.device) if data.get('adc') is not None else None
        self.P = _fisher.param_count(D, A)
        self.workgroups = int(workgroups)
        self._lib = _n.load()
        nbytes = int(self._lib.gxg_work_bytes(B, D, A, self.workgroups))
        if nbytes < 0:
            raise NotImplementedError(f"SurrogateGradient: {self._lib.gxg_last_error().decode()}")
        self._work = torch.empty((nbytes + 7) // 8, dtype=torch.float64, device=self.device)

    def gradient(self):
        """(g (P,) float32, b (P,) float32 or None without adc, info) at pi's current parameters: the flat gradients of
        loss_pi = -(ratio * adv).mean() and surr_cost = (ratio * adc).mean().  info, 0-dim float64 device tensors: `pi_l`
        and `surr_cost` (the learners' pi_l_old and surr_cost_old; surr_cost is 0 without adc), `approx_kl` =
        mean(logp_old - logp) and `ent`, the policy's entropy.  Nothing here synchronises."""
        theta = _fisher.flat_params(self.pi, self.device).contiguous()
        g = torch.empty_like(theta)
        b = torch.empty_like(theta) if self.adc is not None else None
        means = torch.empty(4, dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):                    # the launch goes to the data's device, whichever is current
            _n.check(self._lib.gxg_gradient(self.B, self.D, self.A, HIDDEN, theta.data_ptr(), self.obs.data_ptr(),
                                            self.act.data_ptr(), self.adv.data_ptr(), self.logp.data_ptr(),
                                            self.adc.data_ptr() if self.adc is not None else None, self.workgroups,
                                            self._work.data_ptr(), g.data_ptr(), b.data_ptr() if b is not None else None,
                                            means.data_ptr(), _fisher._stream(self.device)))
        return g, b, {'pi_l': means[0], 'surr_cost': means[1], 'approx_kl': means[2], 'ent': means[3]}


def _direction_from(b, Hinv_g, Hinv_b, approx_g, s, c, target_kl):
    """gxg_cpo_direction on supplied vectors: what cpo_direction runs after its two solves, and the tests' way in.  b,
    Hinv_g, Hinv_b, approx_g: (P,) float32 on one cuda device; s: a float32 tensor of one element there; c, target_kl:
    numbers or tensors of one element there.  -> (x_direction, info) as cpo_direction."""
    who = "cpo_direction"
    b = _checked("b", b, (None,), None, who)
    device, P = b.device, int(b.shape[0])
    Hinv_g = _checked("Hinv_g", Hinv_g, (P,), device, who)
    Hinv_b = _checked("Hinv_b", Hinv_b, (P,), device, who)
    approx_g = _checked("approx_g", approx_g, (P,), device, who)
    s = _checked("s", s.reshape(1) if torch.is_tensor(s) and s.numel() == 1 else s, (1,), device, who)
    crit = torch.stack([_scalar(who, "c", c, device), _scalar(who, "target_kl", target_kl, device)])
    x = torch.empty_like(b)
    case = torch.empty(1, dtype=torch.int32, device=device)
    out = torch.empty(len(DIRECTION), dtype=torch.float64, device=device)
    lib = _n.load()
    with torch.cuda.device(device):
        _n.check(lib.gxg_cpo_direction(P, b.data_ptr(), Hinv_g.data_ptr(), Hinv_b.data_ptr(), approx_g.data_ptr(), s.data_ptr(),
                                       crit.data_ptr(), x.data_ptr(), case.data_ptr(), out.data_ptr(), _fisher._stream(device)))
    info = {'optim_case': case[0], 'need_loss': case[0] > 1}
    info.update({k: out[i] for i, k in enumerate(DIRECTION)})
    return x, info


def cpo_direction(F, g, b, c, target_kl, cg_iters=100):
    """cpo/cpo.py:459-525 on the device: Hinv_g = F.solve(g), approx_g = F(Hinv_g), Hinv_b and s = F.solve(b), then one
    single-workgroup kernel for q, r, A, B, optim_case, lam, nu and x_direction.  `F`: a fisher.FisherOperator; g, b: (P,)
    float32 on its device; `c` (the learners' (EpCost - target_cost) / (EpLen + EPS)) and `target_kl`: Python numbers or 0-dim
    tensors on the device.  The second solve always runs: where b.b <= 1e-8 and c < 0 (the reference skips it and takes case
    4) its result is not read.  -> (x_direction (P,) float32, info): `optim_case` (int32), `lam`, `nu`, `q`, `r`, `s`, `A`, `B`
    (float64) and `need_loss` = optim_case > 1 (bool), all 0-dim on the device, ready for LineSearch.search.  Nothing here
    synchronises."""
    Hinv_g, _, _ = F.solve(g, iters=cg_iters)
    approx_g = F(Hinv_g)
    Hinv_b, s, _ = F.solve(b, iters=cg_iters)
    return _direction_from(b, Hinv_g, Hinv_b, approx_g, s, c, target_kl)


def trpo_direction(F, g, target_kl, cg_iters=100):
    """trpo's x_direction = sqrt(2 target_kl / (s + EPS)) x_hat with x_hat, s = F.solve(g) -> (x_direction (P,) float32,
    info with `s` (float32) and the solve's `iters` and `r_dot`), on the device; nothing here synchronises."""
    x_hat, s, info = F.solve(g, iters=cg_iters)
    tkl = _scalar("trpo_direction", "target_kl", target_kl, x_hat.device).reshape(1)
    x = torch.empty_like(x_hat)
    with torch.cuda.device(x_hat.device):
        _n.check(_n.load().gxg_trpo_direction(int(x_hat.shape[0]), x_hat.data_ptr(), s.reshape(1).data_ptr(), tkl.data_ptr(),
                                             x.data_ptr(), _fisher._stream(x_hat.device)))
    return x, dict(info, s=s)
