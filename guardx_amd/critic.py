"""The cost critic `ac.vc` of the CPO-family learners (safe_rl_libX/cpo/cpo_core.py) on the device:
`critic_values(params, x)` = Vc(x) over rows of observations, in one batched HIP pass (libguardx_critic.so,
include/guardx_critic.h) on torch's current stream, with the bits of the fused rollout's value head.
`params` = Engine.pack_critic(ac.vc)."""
import ctypes as C

import torch

from . import _critic_native

HIDDEN = (64, 128, 192, 256)


def critic_floats(D, h):
    """floats of one packed critic: W1[h][D] b1[h] W2[h][h] b2[h] W3[1][h] b3[1]"""
    return h * D + h + h * h + h + h + 1


def critic_hidden(D, n):
    """the hidden width of a packed critic of `n` floats on D inputs (unique: the size grows with h), or None"""
    return next((h for h in HIDDEN if critic_floats(D, h) == n), None)


def critic_values(params, x, out=None):
    """Vc(x) for x (..., D) float32 on the device; returns (...) float32 (into `out` when given)."""
    if not (torch.is_tensor(x) and x.is_cuda):
        raise ValueError("critic_values: x must be a device tensor")
    if x.dim() < 1 or x.shape[-1] < 1:
        raise ValueError(f"critic_values: x must be (..., D) with D >= 1, got {tuple(x.shape)}")
    D = int(x.shape[-1])
    x = x.to(torch.float32).contiguous()
    params = params.to(device=x.device, dtype=torch.float32).contiguous()
    h = critic_hidden(D, params.numel())
    if h is None:
        raise ValueError(f"critic has {params.numel()} floats; expected one of "
                         f"{[critic_floats(D, h) for h in HIDDEN]} (hidden {HIDDEN}) for D = {D}")
    shape = tuple(x.shape[:-1])
    M = x.numel() // D
    if M >= 2 ** 31:
        raise ValueError("critic_values: more than 2^31 - 1 rows")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=x.device)
    elif tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != x.device or not out.is_contiguous():
        raise ValueError(f"critic_values: out must be a contiguous float32 {shape} tensor on {x.device}")
    if M == 0:
        return out
    lib = _critic_native.load()
    work = torch.empty(int(lib.gxc_critic_work_floats(D, h)), dtype=torch.float32, device=x.device)
    stream = C.c_void_p(torch._C._cuda_getCurrentRawStream(x.device.index))
    _critic_native.check(lib.gxc_critic_values(M, D, h, params.data_ptr(), x.data_ptr(), out.data_ptr(),
                                               work.data_ptr(), stream))
    return out
