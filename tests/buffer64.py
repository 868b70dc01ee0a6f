"""float64 restatement of the kernels that turn a rollout into the learner's batch (guardx_amd/csrc/gx_gae.hip and the
two kernels of gxe_finish / guardx_episode_finish_cols in gx_episode.hip), with a first-order forward error bound for a
float32 implementation of the documented operation order.  Plain numpy, vectorised over envs: the only Python loops run
over time steps.

What is the definition and what is the error.  Inputs are the float32 data taken as exact.  The coefficients are the
values the kernels really use:
  gxe_finish   gamma and lambda rounded to float32, then used as doubles (coef_episode)
  gx_gae_*     gamma as float32 in delta; gamma and gamma lambda as doubles in the two filters (coef_gae)
  _gae_host    plain float32 throughout: float32(gamma) in delta and in the returns' filter, float32(gamma lambda)
               in the advantages' (coef_host, with f32_filters=True)
Everything else (the float32 delta, the cast of the two filters' states to float32, the float32 sums of mean and
deviation in whatever order) is error, bounded with u = 2^-24:
  per step       e_t = u (|g v'| + |r + g v'| + |delta|)              product, sum, difference of the float32 delta
  advantages     E_a[t] = e_t + g lam E_a[t + 1], 0 past the end of a path;  B_adv = E_a + u |a|  (the cast)
  returns        B_ret = u |ret|                                      (a double filter: the cast alone)
  f32_filters    the filters themselves run in float32, so their roundings propagate:
                 E_a[t] = e_t + u |g lam a'| + u |a| + g lam E_a[t + 1],  E_r[t] = u |g r'| + u |r| + g E_r[t + 1]
  mean           mean(B) + u (T - 1) mean|x| + u |mean|               any summation order, so the butterfly too
  d = x - mean   B + E_mean + u |d|
  q = mean(d^2)  (sum(2 |d| E_d + u d^2) + (T - 1) u sum d^2) / T + u q
  sd = sqrt(q)   E_q / (2 sd) + u sd
  d / sd         E_d / sd + |d| E_sd / sd^2 + u |d / sd|
  targetc        u |g qc'| + u |targetc|                              one product, one sum
A comparison passes when |got - ref| <= FACTOR x bound elementwise.  FACTOR = 2 is a fixed condition that covers the
second-order terms and the float64 accumulation; it is not a tuned number (see `ratio`).

The keyword arguments listed under "planted mistakes" build a deliberately WRONG reference; the tests use them to show
that the comparison can fail.
"""
import numpy as np

U = 2.0 ** -24
FACTOR = 2.0
f64 = np.float64


def coef_episode(gamma, lam):
    """gxe_finish: (gamma in delta, gamma of the returns, gamma lambda of the advantages)"""
    g, l = f64(np.float32(gamma)), f64(np.float32(lam))
    return g, g, g * l


def coef_gae(gamma, lam):
    """gx_gae_finish_path / gx_gae_rollout"""
    return f64(np.float32(gamma)), f64(gamma), f64(gamma) * f64(lam)


def coef_host(gamma, lam):
    """rollout_buffer._gae_host: python scalars times float32 tensors"""
    return f64(np.float32(gamma)), f64(np.float32(gamma)), f64(np.float32(f64(gamma) * f64(lam)))


def gae64(rew, val, close, boot, coef, live=None, f32_filters=False):
    """One GAE channel over time-major (T, N) data.  close[t, e]: step t is the last of a path of env e, which is then
    closed with boot[t, e] (value and return past the end).  live[t, e] (default: all): step t belongs to a path at all;
    the other entries are 0 with bound 0.  coef = (g in delta, g of the returns, g lambda of the advantages); the last
    may be a (T,) array (a planted mistake changes it at one step).
    Returns adv, ret, B_adv, B_ret, float64 (T, N)."""
    T, N = rew.shape
    rew, val, boot = np.asarray(rew, f64), np.asarray(val, f64), np.asarray(boot, f64)
    gd, gr = coef[0], coef[1]
    ga = np.broadcast_to(np.asarray(coef[2], f64), (T,))
    adv, ret, Ba, Br = (np.zeros((T, N)) for _ in range(4))
    a_n, r_n, v_n, Ea_n, Er_n = (np.zeros(N) for _ in range(5))
    for t in range(T - 1, -1, -1):
        c = close[t]
        v1, r1 = np.where(c, boot[t], v_n), np.where(c, boot[t], r_n)
        a1, Ea1, Er1 = np.where(c, 0.0, a_n), np.where(c, 0.0, Ea_n), np.where(c, 0.0, Er_n)
        gv = gd * v1
        delta = rew[t] + gv - val[t]
        a = delta + ga[t] * a1
        r = rew[t] + gr * r1
        e = U * (np.abs(gv) + np.abs(rew[t] + gv) + np.abs(delta))
        if f32_filters:
            Ea = e + U * np.abs(ga[t] * a1) + U * np.abs(a) + ga[t] * Ea1
            Er = U * np.abs(gr * r1) + U * np.abs(r) + gr * Er1
            ba, br = Ea, Er
        else:
            Ea, Er = e + ga[t] * Ea1, np.zeros(N)
            ba, br = Ea + U * np.abs(a), U * np.abs(r)
        m = np.ones(N, bool) if live is None else live[t]
        adv[t], ret[t], Ba[t], Br[t] = np.where(m, a, 0.0), np.where(m, r, 0.0), np.where(m, ba, 0.0), np.where(m, br, 0.0)
        a_n, r_n, v_n, Ea_n, Er_n = a, r, val[t], Ea, Er
    return adv, ret, Ba, Br


def normalize64(x, B, scale, count=None, ddof=0):
    """Mean, centring, population deviation and normalisation over all T entries of each row of x (N, T) whose entries
    carry the bound B.  scale=0: centred only.  Returns (value, bound).
    Planted mistakes: count (N,) = the statistics over the first count[e] entries only; ddof=1 = the sample deviation."""
    x, B = np.asarray(x, f64), np.asarray(B, f64)
    N, T = x.shape
    if count is None:
        w, n = np.ones((N, T)), np.full((N, 1), float(T))
    else:
        w, n = (np.arange(T)[None, :] < count[:, None]).astype(f64), count[:, None].astype(f64)
    mean = (w * x).sum(1, keepdims=True) / n
    E_mean = (w * B).sum(1, keepdims=True) / n + U * (T - 1) * (w * np.abs(x)).sum(1, keepdims=True) / n + U * np.abs(mean)
    d = x - mean
    E_d = B + E_mean + U * np.abs(d)
    if not scale:
        return d, E_d
    sq = (w * d * d).sum(1, keepdims=True)
    q = sq / (n - ddof)
    E_q = ((w * (2 * np.abs(d) * E_d + U * d * d)).sum(1, keepdims=True) + (T - 1) * U * sq) / n + U * q
    sd = np.sqrt(q)
    with np.errstate(divide='ignore', invalid='ignore'):      # (a constant row: 0 / 0, nothing to compare)
        E_sd = E_q / (2 * sd) + U * sd
        y = d / sd
        return y, E_d / sd + np.abs(d) * E_sd / sd ** 2 + U * np.abs(y)


def normalize_one_pass_f32(x):
    """A planted mistake, in float32 because that is where it goes wrong: the variance as E[x^2] - mean^2 from one pass
    of sequential float32 sums.  x (N, T) float32 -> (x - mean) / sd, float32."""
    x = np.asarray(x, np.float32)
    N, T = x.shape
    s, s2 = np.zeros(N, np.float32), np.zeros(N, np.float32)
    for t in range(T):
        s, s2 = s + x[:, t], s2 + x[:, t] * x[:, t]
    mean = s / np.float32(T)
    sd = np.sqrt(s2 / np.float32(T) - mean * mean)
    return (x - mean[:, None]) / sd[:, None]


def targetc64(cost, qc, end, gamma):
    """targetc[t] = cost[t] + gamma32 qc[t + 1], the product taken as 0 where end[t] (step t is the last of a path).
    Returns (value, bound), (T, N)."""
    cost, qc = np.asarray(cost, f64), np.asarray(qc, f64)
    nxt = np.zeros_like(qc)
    nxt[:-1] = f64(np.float32(gamma)) * qc[1:]
    nxt = np.where(end, 0.0, nxt)
    tc = cost + nxt
    return tc, U * np.abs(nxt) + U * np.abs(tc)


def rollout_paths(done, last_val=None):
    """gae_rollout's paths: closed with 0 where done == 1, the tape's end closed with last_val.  -> close, boot (T, N)"""
    T, N = done.shape
    close = np.asarray(done) == 1
    boot = np.zeros((T, N))
    if last_val is not None:
        boot[T - 1] = np.where(close[T - 1], 0.0, np.asarray(last_val, f64))
    close = close.copy()
    close[T - 1] = True
    return close, boot


# ---------------------------------------------------------------------------------------------------------------------
# the one-episode batch (gxe_finish / guardx_episode_finish_cols; rollout_buffer.episode_rollout_batch)
# ---------------------------------------------------------------------------------------------------------------------
def episode_lengths(first_done, T, unclamped=False):
    fd = np.asarray(first_done).astype(np.int64)
    return np.where(fd > 0, fd if unclamped else np.minimum(fd, T), T)


def compaction(L, shift_from=None):
    """The (env, t) rows in env-major order and where each lands.  -> env, t, dest (each (sum L,)), n_valid.
    Planted mistake: shift_from = b takes, from env 256 b on, the offset of the env before."""
    N = len(L)
    off = np.concatenate([[0], np.cumsum(L)[:-1]]).astype(np.int64)
    env = np.repeat(np.arange(N), L)
    t = np.arange(int(L.sum())) - np.repeat(off, L)
    if shift_from is not None:
        off = off.copy()
        off[256 * shift_from:] = np.concatenate([[0], off])[256 * shift_from:N]
    return env, t, np.repeat(off, L) + t, int(L.sum())


def gather(x, env, t, dest, n_valid):
    """time-major x (T, N, ...) -> the compacted rows (n_valid, ...)"""
    out = np.zeros((n_valid,) + x.shape[2:], x.dtype)
    out[dest] = x[t, env]
    return out


EXACT = ('obs', 'act', 'mu', 'logp', 'act_safe', 'cost', 'prev_cost')


def episode64(g, gamma=0.99, lam=0.95, boot_finished=False, no_boot=False, drop_lam_at=None, mean_over_L=False, ddof=0,
              targetc_across=False, shift_from=None, unclamped=False):
    """The batch of episode_rollout_batch from the numpy dict g (the keys of an Engine.rollout_episode result).
    -> dict: n_valid; the exact columns (those of EXACT that the form has); 'ret', 'adv' (+ 'cost_ret', 'adc' with g['vc'];
    'targetc' with g['qc']) as (value, bound) pairs over the compacted rows.
    Planted mistakes: boot_finished (a bootstrap for a finished env), no_boot (none for an unfinished one), drop_lam_at=t
    (lambda missing at step t), mean_over_L / ddof=1 (the statistics), targetc_across (gamma qc carried across the end of
    a path), shift_from (see compaction), unclamped (first_done > T counted as it stands: only n_valid is affected)."""
    T, N = g['rew'].shape
    L = episode_lengths(g['first_done'], T)
    finished = np.asarray(g['first_done']) > 0
    steps = np.arange(T)[:, None]
    live, close = steps < L[None, :], steps == (L - 1)[None, :]
    env, t, dest, n_valid = compaction(L, shift_from)
    out = dict(n_valid=int(episode_lengths(g['first_done'], T, True).sum()) if unclamped else n_valid)
    pick = lambda x: gather(x, env, t, dest, n_valid)   # noqa: E731
    cols = [k for k in EXACT if k in g and (k != 'cost' or 'prev_cost' in g or 'qc' in g)]
    out.update({k: pick(np.asarray(g[k], np.float32)) for k in cols})
    coef = coef_episode(gamma, lam)
    if drop_lam_at is not None:
        ga = np.full(T, coef[2])
        ga[drop_lam_at] = coef[0]
        coef = (coef[0], coef[1], ga)

    def channel(rew, val, last, scale):
        use = np.ones(N, bool) if boot_finished else (np.zeros(N, bool) if no_boot else ~finished)
        boot = np.broadcast_to(np.where(use, np.asarray(last, f64), 0.0), (T, N))
        adv, ret, Ba, Br = gae64(rew, val, close, boot, coef, live)
        y, By = normalize64(adv.T, Ba.T, scale, L if mean_over_L else None, ddof)
        return (pick(y.T.copy()), pick(By.T.copy())), (pick(ret), pick(Br))
    out['adv'], out['ret'] = channel(g['rew'], g['val'], g['val_last'], 1)
    if 'vc' in g:
        out['adc'], out['cost_ret'] = channel(g['cost'], g['vc'], g['vc_last'], 0)
    if 'qc' in g:
        tc, Bt = targetc64(g['cost'], g['qc'], np.zeros((T, N), bool) if targetc_across else close, gamma)
        out['targetc'] = (pick(tc), pick(Bt))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# comparing
# ---------------------------------------------------------------------------------------------------------------------
RATIOS = {}      # (who, output) -> (largest error / bound seen, the case it came from)


def ratio(got, ref, bound):
    """the largest |got - ref| / bound; an error where the bound is 0 counts as infinite"""
    err = np.abs(np.asarray(got, f64) - ref)
    if err.size == 0:
        return 0.0
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r))      # (a NaN in `got` gives NaN, which no assertion below lets through)


def check(got, ref_bound, who, output, case):
    """assert |got - ref| <= FACTOR x bound elementwise; the ratio is printed first and kept in RATIOS"""
    ref, bound = ref_bound
    got = np.asarray(got)
    assert got.shape == ref.shape, (who, output, case, got.shape, ref.shape)
    r = ratio(got, ref, bound)
    print(f"error/bound {who:28s} {output:9s} {r:8.3f}  {case}")
    if not RATIOS.get((who, output), (-1.0, None))[0] >= r:
        RATIOS[(who, output)] = (r, case)
    assert r <= FACTOR, f"{who} {output} [{case}]: error / bound = {r} > {FACTOR}"
    return r


def outside(got, ref_bound):
    """a planted mistake is noticed: some element lies outside FACTOR x bound.  Returns the ratio."""
    ref, bound = ref_bound
    if np.asarray(got).shape != ref.shape:
        return float('inf')
    r = ratio(got, ref, bound)
    if r != r:
        return float('inf')      # (a wrong reference that divides by a zero deviation is as wrong as can be)
    return r if r > FACTOR else 0.0


# ---------------------------------------------------------------------------------------------------------------------
# the inputs: synthetic, and shared by the CPU tests (host paths) and the GPU tests (kernels)
# ---------------------------------------------------------------------------------------------------------------------
FORMS = ('plain', 'cost', 'safelayer', 'usl')


def encoded(T, N, K, tag):
    """(T, N, K) float32 whose entries name their own (env, t, k): ((env T + t) 8 + k) + tag / 4, exact in float32"""
    assert K <= 8 and N * T * 8 < 2 ** 21 and tag in (0, 1, 2, 3)
    e, t, k = np.arange(N)[None, :, None], np.arange(T)[:, None, None], np.arange(K)[None, None, :]
    return (((e * T + t) * 8 + k) + tag / 4).astype(np.float32)


def episode_inputs(N, T, D, A, first_done, form='plain', seed=0, mean100=False):
    """a rollout_episode result as numpy, in one of the four forms episode_rollout_batch serves"""
    assert form in FORMS
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)   # noqa: E731
    g = dict(obs=encoded(T, N, D, 0), act=encoded(T, N, A, 1), mu=encoded(T, N, A, 2), logp=r(T, N),
             rew=(100 + r(T, N)) if mean100 else r(T, N), val=r(T, N), val_last=(r(N) + np.float32(2.0)),
             logstd=np.linspace(-0.5, 0.1, A).astype(np.float32), first_done=np.asarray(first_done, np.int32))
    assert g['first_done'].shape == (N,)
    if form == 'cost':
        g.update(cost=rng.random((T, N)).astype(np.float32), vc=r(T, N), vc_last=(r(N) - np.float32(2.0)))
    if form in ('safelayer', 'usl'):
        g.update(act_safe=encoded(T, N, A, 3), cost=rng.random((T, N)).astype(np.float32))
        g.update(prev_cost=rng.random((T, N)).astype(np.float32)) if form == 'safelayer' else g.update(qc=(r(T, N) + np.float32(1.5)))
    return g


def cycle(values, N):
    return np.asarray([values[e % len(values)] for e in range(N)], np.int32)


def partition_first_done(N, T=5):
    """0, 1, T - 1, T, T + 4 with period 5, which does not divide 256: envs 255 and 256 get lengths T and 1"""
    return cycle((0, 1, T - 1, T, T + 4), N)


PARTITION_N = (1, 255, 256, 257, 513)
BSUM_N = 256 * 257 + 3           # the smallest N at which an env's offset loop takes a second turn over bsum


def episode_cases():
    """(name, kwargs of episode_inputs) of every gxe_finish case but the block partition's (PARTITION_N x FORMS, T = 5) and
    the callers' dtypes"""
    rng = np.random.default_rng(11)
    return [
        ('bsum-stride', dict(N=BSUM_N, T=2, D=1, A=1, first_done=rng.integers(0, 4, BSUM_N), form='usl', seed=1)),
        ('gather-stride-a', dict(N=3, T=600, D=5, A=3, first_done=(0, 257, 600), form='cost', seed=2)),
        ('gather-stride-b', dict(N=3, T=600, D=5, A=3, first_done=(600, 1, 0), form='usl', seed=3, mean100=True)),
        ('all-length-1', dict(N=7, T=4, D=5, A=3, first_done=(1,) * 7, form='cost', seed=4)),
        ('all-unfinished', dict(N=7, T=4, D=5, A=3, first_done=(0,) * 7, form='safelayer', seed=5)),
        ('one-env', dict(N=1, T=6, D=1, A=1, first_done=(0,), form='usl', seed=6)),
    ]


def partition_case(N, form):
    D, A = (5, 3) if (FORMS.index(form) + PARTITION_N.index(N)) % 2 else (1, 1)
    return dict(N=N, T=5, D=D, A=A, first_done=partition_first_done(N), form=form, seed=100 + N)


def done_pattern(kind, T, N):
    d = np.zeros((T, N), np.float32)
    if kind == 'every':
        d[:] = 1
    elif kind == 'first':
        d[0] = 1
    elif kind == 'last':
        d[T - 1] = 1
    else:
        assert kind == 'none'
    return d


GAE_N, GAE_T, GAE_DONE = (1, 63, 64, 65), (1, 2, 70), ('none', 'every', 'first', 'last')


def gae_inputs(N, T, kind, seed=0, mixed=False):
    """rew, val, done (T, N) and a last_val of magnitude >= 1.  mixed: done at random steps (p = 0.1) instead"""
    rng = np.random.default_rng(1000 * N + 10 * T + seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)   # noqa: E731
    done = (rng.random((T, N)) < 0.1).astype(np.float32) if mixed else done_pattern(kind, T, N)
    lv = r(N)
    return r(T, N), r(T, N), done, (np.sign(lv) + (lv == 0) + lv).astype(np.float32)


NORM_T, NORM_N = (2, 63, 64, 65, 129, 1000), (1, 3, 4, 5)


def norm_rows(N, T, mean100, seed=0):
    rng = np.random.default_rng(7000 + 10 * T + N + seed)
    x = rng.normal(size=(N, T))
    return ((100.0 + x) if mean100 else x).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------------
# whole batches against the restatement
# ---------------------------------------------------------------------------------------------------------------------
def rollout64(rew, val, done, last_val, coef, scale=1, f32_filters=False):
    """gae_rollout + the per-env normalisation: -> (adv (N, T), bound), (ret (T, N), bound), (raw adv (T, N), bound)"""
    close, boot = rollout_paths(done, last_val)
    adv, ret, Ba, Br = gae64(rew, val, close, boot, coef, None, f32_filters)
    return normalize64(adv.T, Ba.T, scale), (ret, Br), (adv, Ba)


def check_episode(got, ref, who, case):
    """a batch of episode_rollout_batch (numpy) against episode64's: n_valid, every gathered column exactly, the computed
    ones within FACTOR x bound"""
    assert got['n_valid'] == ref['n_valid'], (who, case, got['n_valid'], ref['n_valid'])
    computed = [k for k in ('ret', 'adv', 'cost_ret', 'adc', 'targetc') if k in ref]
    exact = [k for k in EXACT if k in ref]
    assert set(got) == set(computed) | set(exact) | {'n_valid', 'logstd'}, (who, case, sorted(got))
    for k in exact:
        assert got[k].shape == ref[k].shape, (who, case, k)
        bad = np.argwhere(got[k] != ref[k])
        assert len(bad) == 0, f"{who} [{case}] {k}: row {bad[0]} holds {got[k][tuple(bad[0])]}, expected {ref[k][tuple(bad[0])]}"
    for k in computed:
        check(got[k], ref[k], who, k, case)


def to_torch(g, device=None):
    import torch
    out = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in g.items()}
    if device is not None:
        out = {k: v.to(device) for k, v in out.items()}
    out['t0'] = 0
    return out


def to_numpy(batch):
    return {k: (v.detach().cpu().numpy() if hasattr(v, 'detach') else v) for k, v in batch.items()}


def rollout_out(N, T, D, A, rew, val, done, seed=0):
    """a rollout result (numpy) with every key the *_rollout_batch helpers ask for; obs / act / mu / act_safe encoded"""
    rng = np.random.default_rng(seed)
    r = lambda *s: rng.normal(size=s).astype(np.float32)   # noqa: E731
    return dict(obs=encoded(T, N, D, 0), act=encoded(T, N, A, 1), mu=encoded(T, N, A, 2), act_safe=encoded(T, N, A, 3),
                logp=r(T, N), rew=rew, val=val, done=done, logstd=np.linspace(-0.5, 0.1, A).astype(np.float32),
                cost=rng.random((T, N)).astype(np.float32), prev_cost=rng.random((T, N)).astype(np.float32),
                qc=(r(T, N) + np.float32(1.5)), vc=r(T, N), cost_inc=rng.random((T, N)).astype(np.float32),
                M=rng.random((T, N)).astype(np.float32), val_last=(r(N) + np.float32(2.0)), vc_last=(r(N) - np.float32(2.0)))


def env_major(x):
    """(T, N, ...) -> (N T, ...), the order every *_rollout_batch returns"""
    return np.ascontiguousarray(np.swapaxes(x, 0, 1)).reshape((-1,) + x.shape[2:])
