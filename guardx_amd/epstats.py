"""The episode bookkeeping of the reset_done learners over what a fused rollout returned: `episode_stats(out)` gives what
their collection loops log as EpRet, EpCost, EpLen, EpCostRet, MaxEpLenRet, VVals and CumulativeCost (safe_rl_libX
trpo/trpo.py:455-541, cpo/cpo.py:596-670 and the same blocks of trpolag, pcpo, pdo, scpo, safelayer, usl, lpg), reduced
the way the logger reduces them (utils/mpi_tools.py:70-92), in one call and, on the device, without a host
synchronisation (libguardx_epstats.so, include/guardx_epstats.h).  The sibling of rollout_buffer.gae_rollout.

The definition ("Episode statistics on the fused path") in short.  Per env, for every step t of the call
(epoch step t0 + t), float64 accumulators fed with the float32 inputs, one add per step:
    ep_ret += rew; ep_cost += cost; epoch_ret += rew; ep_len += 1; with gamma: ep_cost_ret += cost * g[t0 + t]
    on the time-out step (t0 + t + 1 == max_ep_len): an env emits its episode only if ep_len == max_ep_len, every env
    emits epoch_ret as a MaxEpLenRet entry, everything is cleared; otherwise an env with done == 1 emits and clears
    ep_ret, ep_cost, ep_cost_ret, ep_len.
Emitted episodes are ordered by step and within a step by env.  Per key the entries are rounded to float32, then in
float64: n, S (sum), mean = S / n, Q = sum (x - mean)^2, std = sqrt(Q / n), min, max.  S and Q add entry i into slot
i mod 256 in increasing i and fold the slots pairwise with strides 128 .. 1, on the device and here alike, so both give
the same bits.

Host tensors run the same definition in numpy below, operation for operation.
"""
import ctypes as C
import math

import numpy as np
import torch

from . import _epstats_native as _n

SLOTS = 256
KEYS = ('EpRet', 'EpCost', 'EpLen', 'EpCostRet', 'MaxEpLenRet', 'VVals')
_ROW = {'EpRet': _n.GXT_KEY_EP_RET, 'EpCost': _n.GXT_KEY_EP_COST, 'EpLen': _n.GXT_KEY_EP_LEN,
        'EpCostRet': _n.GXT_KEY_EP_COST_RET, 'MaxEpLenRet': _n.GXT_KEY_MAX_RET, 'VVals': _n.GXT_KEY_VVALS}
EPISODE_ARRAYS = ('env', 't_end', 'ep_ret', 'ep_cost', 'ep_cost_ret', 'ep_len')


def discount_table(gamma, max_ep_len):
    """g[k] = gamma ** k as the learners compute it (cpo.py:612: Python's `**` on the epoch's step), float64"""
    return np.array([float(gamma) ** k for k in range(int(max_ep_len))], dtype=np.float64)


# ---------------------------------------------------------------------------------------------------------------------
# the host statement
# ---------------------------------------------------------------------------------------------------------------------
def slot_sum(x):
    """the float64 sum of x in the fixed order: entry i into slot i mod 256 in increasing i, slots folded pairwise"""
    x = np.asarray(x, dtype=np.float64).reshape(-1)
    rows = -(-x.size // SLOTS)
    pad = np.zeros(rows * SLOTS, np.float64)       # + 0.0 leaves a slot as it is (a slot is never -0.0: it starts at +0.0)
    pad[:x.size] = x
    acc = np.zeros(SLOTS, np.float64)
    with np.errstate(all='ignore'):
        for row in pad.reshape(rows, SLOTS):
            acc = acc + row
        stride = SLOTS // 2
        while stride >= 1:
            acc[:stride] = acc[:stride] + acc[stride:2 * stride]
            stride //= 2
    return acc[0]


def moments_host(x, as_logged=True):
    """(n, S, mean, Q, min, max, std) of the entries x; as_logged: each rounded to float32 first"""
    x = np.asarray(x).reshape(-1)
    x = x.astype(np.float32).astype(np.float64) if as_logged else x.astype(np.float64)
    n = x.size
    with np.errstate(all='ignore'):
        S = slot_sum(x)
        mean = np.float64(S) / np.float64(n)
        d = x - mean
        Q = slot_sum(d * d)
        mn, mx = (x.min(), x.max()) if n else (np.inf, -np.inf)
        if n and mn == 0 and np.signbit(x[x == 0]).any():      # minimum(-0, +0) = -0, maximum = +0, whatever the order
            mn = -0.0
        if n and mx == 0 and not np.signbit(x[x == 0]).all():
            mx = 0.0
        std = np.sqrt(np.float64(Q) / np.float64(n))
    return np.array([n, S, mean, Q, mn, mx, std], dtype=np.float64)


def _scan_host(rew, cost, done, g, acc, ln, t0, max_ep_len):
    """the learner loop over (T, N) float32 arrays; acc (4, N) float64 and ln (N,) int32 are updated in place"""
    T, N = rew.shape
    ep = {k: [] for k in EPISODE_ARRAYS}
    cost_env, max_ret = np.zeros(N, np.float64), None
    with np.errstate(all='ignore'):
        for t in range(T):
            acc[0] += rew[t]
            acc[1] += cost[t]
            acc[3] += rew[t]
            cost_env += cost[t]
            ln += 1
            if g is not None:
                acc[2] += cost[t].astype(np.float64) * g[t0 + t]
            timeout = t0 + t + 1 == max_ep_len
            idx = np.nonzero(ln == max_ep_len)[0] if timeout else np.nonzero(done[t] == 1)[0]
            ep['env'].append(idx.astype(np.int32))
            ep['t_end'].append(np.full(idx.size, t0 + t, np.int32))
            ep['ep_ret'].append(acc[0, idx].copy())
            ep['ep_cost'].append(acc[1, idx].copy())
            ep['ep_cost_ret'].append(acc[2, idx].copy())
            ep['ep_len'].append(ln[idx].copy())
            if timeout:
                max_ret = acc[3].copy()
                acc[:] = 0
                ln[:] = 0
            else:
                acc[:3, idx] = 0
                ln[idx] = 0
    cat = lambda k, dt: np.concatenate(ep[k]).astype(dt) if ep[k] else np.zeros(0, dt)   # noqa: E731
    ep = {k: cat(k, np.float64 if k in ('ep_ret', 'ep_cost', 'ep_cost_ret') else np.int32) for k in EPISODE_ARRAYS}
    return ep, max_ret, cost_env


# ---------------------------------------------------------------------------------------------------------------------
# the public call
# ---------------------------------------------------------------------------------------------------------------------
MOMENTS = 7
_FIELDS = ('n', 'S', 'mean', 'Q', 'min', 'max', 'std')    # a row of moments


def _key_stats(row):
    n, S, mean, Q, mn, mx, std = row.unbind(0)
    return {'n': n, 'S': S, 'mean': mean, 'Q': Q, 'std': std, 'min': mn, 'max': mx}


def _std(Q, n):
    """sqrt(Q / n), correctly rounded (torch's float64 sqrt on the host is not: numpy's is, and so is the device's)"""
    x = Q / n
    if x.is_cuda:
        return torch.sqrt(x)
    with np.errstate(all='ignore'):
        return torch.from_numpy(np.asarray(np.sqrt(x.numpy())))


_TABLES = {}


def _table(gamma, max_ep_len, device):
    key = (float(gamma), int(max_ep_len), str(device))
    if key not in _TABLES:
        if len(_TABLES) > 16:
            _TABLES.clear()
        _TABLES[key] = torch.from_numpy(discount_table(gamma, max_ep_len)).to(device)
    return _TABLES[key]


def _stream(device):
    return C.c_void_p(torch._C._cuda_getCurrentRawStream(device.index))


def _check_carry(carry, N, device):
    if not (isinstance(carry, dict) and {'acc', 'len', 't'} <= set(carry)):
        raise ValueError("episode_stats: carry must be the 'carry' entry of an earlier result")
    acc, ln = carry['acc'], carry['len']
    if tuple(acc.shape) != (4, N) or acc.dtype != torch.float64 or tuple(ln.shape) != (N,) or ln.dtype != torch.int32:
        raise ValueError(f"episode_stats: carry holds {tuple(acc.shape)} {acc.dtype} / {tuple(ln.shape)} {ln.dtype}; "
                         f"expected (4, {N}) float64 / ({N},) int32")
    if acc.device != device or ln.device != device:
        raise ValueError(f"episode_stats: carry lives on {acc.device}, the rollout on {device}")
    return acc.contiguous(), ln.contiguous(), int(carry['t'])


def episode_stats(out_or_rew, cost=None, done=None, *, val=None, max_ep_len=None, gamma=None, carry=None, episodes=False):
    """The learners' episode statistics of one rollout.

    `out_or_rew`: a rollout dict (rollout_policy, _statewise, _safelayer, _usl, _lpg: its rew, cost, done and, unless
    val=False, its val), or `rew` with `cost` and `done` (Engine.rollout's tuple: episode_stats(rew, cost, done)); all
    time-major (T, N) float32.  A dict that carries first_done (rollout_episode, episode=True) takes the one-episode
    form below.  `val` (T, N): every element is a VVals entry.  `max_ep_len`: the epoch's length, default T.  `gamma`:
    also EpCostRet, the cost discounted by the EPOCH's step as cpo.py:612 has it.  `carry`: the 'carry' of the previous
    call of the same epoch; the call then covers the epoch steps [t0, t0 + T).  t0 + T > max_ep_len raises ValueError.

    Returns a dict of tensors on the inputs' device: per key (EpRet, EpCost, EpLen; EpCostRet with gamma; MaxEpLenRet
    when the call holds the time-out step; VVals with val) a dict of 0-dim float64 n, mean, std, min, max (and S, Q:
    what combine_episode_stats gathers); cost_sum (float64: the sum of cost over the call; the reference's cum_cost is
    a float32 scalar that stops counting units past 2^24, which is not copied); n_episodes (int32); carry.  With
    episodes=True also the emitted episodes in logger order: env, t_end, ep_len (int32), ep_ret, ep_cost, ep_cost_ret
    (float64), sliced to n_episodes with one .item().  Without it the call never synchronises.
    n == 0 gives mean = std = NaN, min = +inf, max = -inf; a NaN entry makes mean, std, min and max NaN.

    One-episode form: the entries are the N envs (ppo_one_episode/ppo.py:419-425): EpRet = out['ep_ret'], EpCost =
    out['ep_cost'], EpLen = first_done, or t0 + T where that is 0, MaxEpLenRet = the one value
    mean(ep_ret / (t0 + T)) * 1000 (the mean in float64, in the slot order).  No carry, no cost_sum."""
    if isinstance(out_or_rew, dict):
        out = out_or_rew
        if cost is not None or done is not None:
            raise ValueError("episode_stats: pass a rollout dict alone, or rew, cost and done")
        if 'first_done' in out:
            return _one_episode(out)
        for k in ('rew', 'cost', 'done'):
            if k not in out:
                raise KeyError(f"episode_stats needs out['{k}']")
        rew, cost, done = out['rew'], out['cost'], out['done']
        if val is None and 'val' in out:
            val = out['val']
    else:
        rew = out_or_rew
        if cost is None or done is None:
            raise ValueError("episode_stats: pass a rollout dict alone, or rew, cost and done")
    if val is False:
        val = None
    for name, x in (('rew', rew), ('cost', cost), ('done', done), ('val', val)):
        if x is None:
            continue
        if not torch.is_tensor(x) or x.dim() != 2:
            raise ValueError(f"episode_stats: {name} must be a (T, N) tensor")
        if tuple(x.shape) != tuple(rew.shape):
            raise ValueError(f"episode_stats: {name} is {tuple(x.shape)}, rew {tuple(rew.shape)}")
        if x.device != rew.device:
            raise ValueError(f"episode_stats: {name} lives on {x.device}, rew on {rew.device}")
    T, N = (int(s) for s in rew.shape)
    dev = rew.device
    acc, ln, t0 = (None, None, 0) if carry is None else _check_carry(carry, N, dev)   # read, never written
    if max_ep_len is None:                              # a later call of an epoch: the length its first call was given
        max_ep_len = carry.get('max_ep_len', T) if carry is not None else T
    max_ep_len = int(max_ep_len)
    if t0 < 0 or t0 + T > max_ep_len:
        raise ValueError(f"episode_stats: the call covers the epoch steps [{t0}, {t0 + T}), past max_ep_len = {max_ep_len}")
    f = lambda x: x if x.dtype == torch.float32 and x.is_contiguous() else x.to(torch.float32).contiguous()   # noqa: E731
    rew, cost, done = f(rew), f(cost), f(done)
    val = None if val is None else f(val)
    timeout = T > 0 and t0 + T == max_ep_len
    if dev.type != 'cuda' or N == 0 or T == 0:
        g = None if gamma is None else discount_table(gamma, max_ep_len)
        a = np.zeros((4, N), np.float64) if acc is None else acc.cpu().numpy().copy()
        l_ = np.zeros(N, np.int32) if ln is None else ln.cpu().numpy().copy()
        ep, max_ret, cost_env = _scan_host(rew.cpu().numpy(), cost.cpu().numpy(), done.cpu().numpy(), g, a, l_, t0, max_ep_len)
        rows = np.zeros((_n.GXT_KEYS, MOMENTS), np.float64)
        rows[_n.GXT_KEY_EP_RET] = moments_host(ep['ep_ret'])
        rows[_n.GXT_KEY_EP_COST] = moments_host(ep['ep_cost'])
        rows[_n.GXT_KEY_EP_LEN] = moments_host(ep['ep_len'])
        rows[_n.GXT_KEY_EP_COST_RET] = moments_host(ep['ep_cost_ret'])
        if timeout:
            rows[_n.GXT_KEY_MAX_RET] = moments_host(max_ret)
        if val is not None:
            rows[_n.GXT_KEY_VVALS] = moments_host(val.cpu().numpy())
        rows[_n.GXT_KEY_COST_SUM] = moments_host(cost_env, as_logged=False)
        moments = torch.from_numpy(rows).to(dev)
        acc, ln = torch.from_numpy(a).to(dev), torch.from_numpy(l_).to(dev)
        count = torch.tensor(ep['env'].size, dtype=torch.int32, device=dev)
        arrays = {k: torch.from_numpy(v).to(dev) for k, v in ep.items()}
    else:
        lib = _n.load()
        nbytes = int(lib.gxt_work_bytes(N, T))
        if nbytes < 0:
            raise ValueError(f"episode_stats: T * N = {T} * {N} is more than the device path indexes (31 bits)")
        # two allocations, the float64 and the int32 results, carved by address (the workspace last: 8-byte aligned);
        # views are made only of what is returned
        cap, nm = T * N, _n.GXT_KEYS * MOMENTS
        f64 = torch.empty(nm + 5 * N + 3 * cap + (nbytes + 7) // 8, dtype=torch.float64, device=dev)
        i32 = torch.empty(1 + N + 3 * cap, dtype=torch.int32, device=dev)
        p64, p32, at = f64.data_ptr(), i32.data_ptr(), nm + 5 * N
        g = None if gamma is None else _table(gamma, max_ep_len, dev)
        _n.check(lib.gxt_episode_stats(
            N, T, t0, max_ep_len, rew.data_ptr(), cost.data_ptr(), done.data_ptr(), None if val is None else val.data_ptr(),
            None if g is None else g.data_ptr(), None if acc is None else acc.data_ptr(), None if ln is None else ln.data_ptr(),
            p64 + 8 * nm, p32 + 4, p64 + 8 * (at + 3 * cap), p32 + 4 * (1 + N), p32 + 4 * (1 + N + cap), p64 + 8 * at,
            p64 + 8 * (at + cap), p64 + 8 * (at + 2 * cap), p32 + 4 * (1 + N + 2 * cap), p32, p64 + 8 * (nm + 4 * N), p64,
            _stream(dev)))
        moments, count = f64[:nm], i32[0]
        if episodes:
            arrays = {k: f64[at + j * cap:at + (j + 1) * cap] for j, k in enumerate(('ep_ret', 'ep_cost', 'ep_cost_ret'))}
            arrays.update({k: i32[1 + N + j * cap:1 + N + (j + 1) * cap] for j, k in enumerate(('env', 't_end', 'ep_len'))})
        acc_out, ln_out = f64[nm:nm + 4 * N].view(4, N), i32[1:1 + N]
        acc, ln = acc_out, ln_out
    res = {}
    cells = moments.reshape(-1).unbind(0)               # every 0-dim result in one operation
    for k in KEYS:
        if (k == 'EpCostRet' and gamma is None) or (k == 'MaxEpLenRet' and not timeout) or (k == 'VVals' and val is None):
            continue
        res[k] = dict(zip(_FIELDS, cells[MOMENTS * _ROW[k]:MOMENTS * (_ROW[k] + 1)]))
    res['cost_sum'] = cells[MOMENTS * _n.GXT_KEY_COST_SUM + 1]
    res['n_episodes'] = count
    res['carry'] = {'acc': acc, 'len': ln, 't': 0 if timeout else t0 + T, 'max_ep_len': max_ep_len}
    if episodes:
        k_ = int(count.item())
        res.update({k: arrays[k][:k_] for k in EPISODE_ARRAYS})
    return res


def _one_episode(out):
    for k in ('ep_ret', 'ep_cost', 'first_done', 'rew', 't0'):
        if k not in out:
            raise KeyError(f"episode_stats (one-episode form) needs out['{k}']")
    ep_ret, ep_cost, fd = out['ep_ret'], out['ep_cost'], out['first_done']
    N = int(fd.shape[0])
    if tuple(ep_ret.shape) != (N,) or tuple(ep_cost.shape) != (N,):
        raise ValueError(f"episode_stats: ep_ret {tuple(ep_ret.shape)} / ep_cost {tuple(ep_cost.shape)} are not ({N},)")
    L = int(out['t0']) + int(out['rew'].shape[0])
    dev = fd.device
    ep_len = torch.where(fd > 0, fd, torch.full_like(fd, L)).to(torch.float32)
    x = torch.stack([ep_ret.to(torch.float32), ep_cost.to(torch.float32), ep_len]).contiguous()
    y = (ep_ret.to(torch.float64) / float(L)).contiguous()           # ep_ret / ep_len: ep_len is t0 + T for every env
    if dev.type != 'cuda' or N == 0:
        rows = np.stack([moments_host(r) for r in x.cpu().numpy()] + [moments_host(y.cpu().numpy(), as_logged=False)])
        moments = torch.from_numpy(rows).to(dev)
    else:
        lib = _n.load()
        moments = torch.empty((4, MOMENTS), dtype=torch.float64, device=dev)
        _n.check(lib.gxt_moments(3, N, 0, x.data_ptr(), moments.data_ptr(), _stream(dev)))
        _n.check(lib.gxt_moments(1, N, 1, y.data_ptr(), moments[3].data_ptr(), _stream(dev)))
    res = {k: _key_stats(moments[i]) for i, k in enumerate(('EpRet', 'EpCost', 'EpLen'))}
    v = (moments[3, 2] * 1000.0).to(torch.float32).to(torch.float64)  # the one logged value, as the logger rounds it
    one = torch.ones_like(v)
    res['MaxEpLenRet'] = _key_stats(torch.stack([one, v, v / one, (v - v) * (v - v), v, v, _std((v - v) * (v - v), one)]))
    res['n_episodes'] = torch.tensor(N, dtype=torch.int32, device=dev)
    return res


def _stat_keys(stats):
    return [k for k in KEYS if k in stats]


def combine_episode_stats(stats):
    """The statistics of all ranks' entries from each rank's episode_stats result: one all_gather of (n, S, Q, min, max)
    per key (float64, all keys in one tensor, with cost_sum and n_episodes), over the process group's backend (gloo on
    host tensors, RCCL on device tensors).  n = sum n_r, mean = sum S_r / n, Q = sum_r [Q_r + n_r (S_r / n_r - mean)^2],
    added in rank order; ranks with n_r = 0 are skipped.  Every rank must hold the same keys.  Without a process group of
    more than one rank the input is returned as it is."""
    from . import dist as _gxd
    import torch.distributed as dist
    if not _gxd._collective():
        return stats
    keys = _stat_keys(stats)
    extras = [k for k in ('cost_sum', 'n_episodes') if k in stats]      # plain sums: rows (1, value, 0, 0, 0)
    any_ = stats[keys[0]]['n']
    one, nil = torch.ones_like(any_), torch.zeros_like(any_)
    mine = torch.stack([torch.stack([stats[k][f] for f in ('n', 'S', 'Q', 'min', 'max')]) for k in keys] +
                       [torch.stack([one, stats[k].to(torch.float64), nil, nil, nil]) for k in extras]).contiguous()
    world = dist.get_world_size()
    every = torch.empty((world,) + tuple(mine.shape), dtype=torch.float64, device=mine.device)
    dist.all_gather_into_tensor(every.view((world * mine.shape[0],) + tuple(mine.shape[1:])), mine)
    n_r, S_r, Q_r, mn_r, mx_r = every.unbind(-1)                     # each (world, rows)
    zero = torch.zeros_like(n_r[0])
    has = n_r > 0
    n, S = zero.clone(), zero.clone()
    for r in range(world):
        n = n + n_r[r]
        S = S + torch.where(has[r], S_r[r], zero)
    mean = S / n
    Q = zero.clone()
    for r in range(world):
        dev_r = S_r[r] / n_r[r] - mean
        Q = Q + torch.where(has[r], Q_r[r] + n_r[r] * (dev_r * dev_r), zero)
    nan = torch.isnan(mn_r).any(0)
    nanv = torch.full_like(zero, float('nan'))
    mn = torch.where(nan, nanv, torch.where(torch.isnan(mn_r), torch.full_like(mn_r, math.inf), mn_r).min(0).values)
    mx = torch.where(nan, nanv, torch.where(torch.isnan(mx_r), torch.full_like(mx_r, -math.inf), mx_r).max(0).values)
    std = _std(Q, n)
    res = dict(stats)
    for i, k in enumerate(keys):
        res[k] = _key_stats(torch.stack([n[i], S[i], mean[i], Q[i], mn[i], mx[i], std[i]]))
    for i, k in enumerate(extras, len(keys)):
        res[k] = S[i].to(stats[k].dtype)
    return res


def constraint_value(stats, target_cost, eps=1e-8):
    """c of the CPO-family update (cpo.py:449-456): (EpCost.mean - target_cost) / (EpLen.mean + eps)"""
    return (stats['EpCost']['mean'] - target_cost) / (stats['EpLen']['mean'] + eps)
