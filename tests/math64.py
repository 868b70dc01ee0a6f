"""The input sets, the float64 references, the error measures and the bounds for the fp32 math primitives
(guardx_amd/csrc/gx_device.h: sincos_f, atan2_f, exp_f, log_f, tanh_f, rcp_unscaled, div_bin16; gx_policy.h: normal_pair; and
the compiler's `/` and sqrtf), shared by tests/test_math64.py (the C checker's twins, CPU) and tests/test_gpu_math64.py
(the device's).  Every generator is seeded, so both see the same arrays.

The sets
  * binade sets: for every exponent of a function's domain PER random mantissas plus the first two and the last two values
    of the binade, both signs where the function takes them;
  * tie sets: fl(p) and its two fp32 neighbours for the points p at which a range reduction switches (multiples of pi / 2;
    (k + 1/2) ln 2), around the m > 1.41421356f split of log_f, around |x| = 9 of tanh_f, -87 / 88 of exp_f, 2^-100 and
    2 pi of div_bin16;
  * SPECIALS: +-0, +-inf, NaN, +-FLT_MIN, the smallest and the largest denormal (both signs), +-FLT_MAX -- 13 values, and
    their 13 x 13 grid for the two-operand functions.

The references are numpy's float64 sin, cos, arctan2, exp, log, tanh and oracle/policy64.normal_pair.  For x / y, 1 / x,
sqrt, rcp_unscaled and div_bin16 the reference is EXACT: numpy's float32 operation, which is correctly rounded on the CPU
(and equals the float64 result rounded once: 53 >= 2 * 24 + 2; tests/test_math64.py checks that).

BOUNDS: the worst error of the C CHECKER (oracle.math_probe / math_probe2) over these sets, measured on the CPU, times 1.25
and rounded up to two digits.  The sets are samples of the domains; the quarter is for the inputs not sampled, and is no
larger so that a bound stays within a factor of two of what the algorithm does.  The device's results are never the source
of a bound.  `python tests/math64.py` prints the measured values.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

F32, U32 = np.float32, np.uint32
PER = 4092                       # random mantissas per binade and sign (+ 4 edge values = 4096)
EDGE = 4                         # first two and last two values of a binade
FLT_MIN, FLT_MAX = F32(2.0 ** -126), np.finfo(F32).max
DEN_MIN, DEN_MAX = F32(2.0 ** -149), np.uint32(0x007FFFFF).view(F32)
TWO_PI_F = F32(6.2831854820251465)
BIN_SIZE16 = F32(float.fromhex("0x1.921fb6p-2"))          # gx_device.h:kBinSize16
LOG_SPLIT = F32(1.41421356)                               # gx_device.h:log_f, `m > 1.41421356f`
SPECIALS = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MIN, -FLT_MIN, DEN_MIN, -DEN_MIN, DEN_MAX, -DEN_MAX,
                     FLT_MAX, -FLT_MAX], F32)
MAX_SET = 1 << 23                # no set is larger


def f2u(x):
    return np.ascontiguousarray(x, F32).view(U32)


def u2f(u):
    return np.ascontiguousarray(u, U32).view(F32)


def neighbours(p, k=1):
    """fl(p) with its k fp32 neighbours on either side (p: float64 array) -> float32, 2 k + 1 values per point"""
    c = np.asarray(p, np.float64).astype(F32).reshape(-1)
    out, lo, hi = [c], c, c
    for _ in range(k):
        lo = np.nextafter(lo, F32(-np.inf))
        hi = np.nextafter(hi, F32(np.inf))
        out += [lo, hi]
    return np.stack(out, 1).reshape(-1)


def binade_bits(e):
    """(first, last) bit pattern of the positive floats in [2^e, 2^(e+1)): e in -149 .. 127 (denormals below -126)"""
    if e >= -126:
        lo = (e + 127) << 23
        return lo, lo | 0x7FFFFF
    return 1 << (e + 149), (1 << (e + 150)) - 1


def binade_count(e, per=PER):
    lo, hi = binade_bits(e)
    return min(per + EDGE, hi - lo + 1)


def binades(exps, rng, signs=(0, 1), per=PER):
    """per random values plus the first two and the last two of every binade 2^e, e in exps (all of a binade with fewer
    values), for each sign"""
    out = []
    for e in exps:
        lo, hi = binade_bits(e)
        if hi - lo + 1 <= per + EDGE:
            b = np.arange(lo, hi + 1, dtype=np.uint64)
        else:
            b = np.concatenate([rng.integers(lo, hi + 1, per, dtype=np.uint64),
                                np.array([lo, lo + 1, hi - 1, hi], np.uint64)])
        for s in signs:
            out.append((b | np.uint64(s << 31)).astype(U32))
    return u2f(np.concatenate(out))


def both_signs(x):
    return np.concatenate([x, -x])


def _sized(x):
    x = np.ascontiguousarray(x, F32)
    assert x.size <= MAX_SET
    return x


# ---------------------------------------------------------------------------------------------------------------------
# the sets
# ---------------------------------------------------------------------------------------------------------------------
SINCOS_EXPS = range(-126, 24)                 # 2^-126 .. 2^24 (kFinite's domain is |x| <= 2^24)
SINCOS_K_SEQ, SINCOS_K_RAND = 200000, 300000
SINCOS_K_MAX = int(2.0 ** 24 / (np.pi / 2))   # 10680707


def sincos_ties():
    """k pi / 2 (k = 1 .. 2e5 and 3e5 random k up to 2^24 / (pi / 2)) with both fp32 neighbours, both signs; none above 2^24"""
    rng = np.random.default_rng(101)
    k = np.concatenate([np.arange(1, SINCOS_K_SEQ + 1), rng.integers(SINCOS_K_SEQ + 1, SINCOS_K_MAX + 1, SINCOS_K_RAND)])
    t = neighbours(k.astype(np.float64) * (np.pi / 2))
    return both_signs(np.minimum(t, F32(2.0 ** 24)))


SINCOS_DENSE = 1 << 19                        # per band: most of the binades lie below 1, where there is little to get wrong


def sincos_set():
    rng = np.random.default_rng(100)
    dense = [np.linspace(-np.pi, np.pi, SINCOS_DENSE), rng.uniform(-1e4, 1e4, SINCOS_DENSE), rng.uniform(-1e5, 1e5, SINCOS_DENSE)]
    return _sized(np.concatenate([binades(SINCOS_EXPS, rng), F32([2.0 ** 24, -2.0 ** 24]), sincos_ties(), SPECIALS] +
                                 [d.astype(F32) for d in dense]))


EXP_LO, EXP_HI = F32(-87.0), F32(88.0)
EXP_EXPS = range(-126, 7)
EXP_K = range(-126, 128)                      # rint(x log2 e) over [-87, 88]
EXP_LIN = 1 << 18


def exp_ties():
    """(k + 1/2) ln 2 for every k of exp_f's range (where rint(x log2 e) switches), with both neighbours, inside [-87, 88]"""
    p = (np.arange(EXP_K.start, EXP_K.stop - 1) + 0.5) * np.log(2.0)
    t = neighbours(p)
    return t[(t >= EXP_LO) & (t <= EXP_HI)]


def exp_set():
    rng = np.random.default_rng(110)
    b = np.clip(binades(EXP_EXPS, rng), EXP_LO, EXP_HI)
    return _sized(np.concatenate([b, np.linspace(-87.0, 88.0, EXP_LIN).astype(F32), exp_ties(),
                                  neighbours([-87.0, 88.0], 4), SPECIALS]))


LOG_EXPS = range(-126, 128)
LOG_SPLIT_EXPS = (-126, -64, -1, 0, 1, 64, 127)


def log_ties():
    """the mantissas within 8 ulp of 1.41421356f (where log_f halves m) in several binades"""
    m = f2u(LOG_SPLIT) & U32(0x7FFFFF)
    d = np.arange(-8, 9)
    return u2f(np.concatenate([((e + 127) << 23) | (int(m[0]) + d) for e in LOG_SPLIT_EXPS]).astype(U32))


def log_set():
    """positive normal floats only: log_f is stated for those"""
    rng = np.random.default_rng(120)
    return _sized(np.concatenate([binades(LOG_EXPS, rng, signs=(0,)), log_ties(), neighbours([1.0], 4),
                                  F32([FLT_MIN, FLT_MAX])]))


TANH_EXPS = range(-126, 5)
TANH_LIN = 1 << 18
TANH_TINY = F32(2.0 ** -26)


def tanh_ties():
    """half of exp_f's tie points (tanh_f doubles its argument) up to |x| = 9.5, both signs, and |x| = 9 with 4 neighbours"""
    p = (np.arange(0, 28) + 0.5) * np.log(2.0) / 2
    return np.concatenate([both_signs(neighbours(p[p <= 9.5])), both_signs(neighbours([9.0], 4))])


def tanh_set():
    rng = np.random.default_rng(130)
    return _sized(np.concatenate([binades(TANH_EXPS, rng), np.linspace(-9.5, 9.5, TANH_LIN).astype(F32), tanh_ties(),
                                  SPECIALS]))


# tanh_act (gx_fisher.hip, the Fisher product's activation; libguardx_fisher.so:gxf_tanh_act): an odd polynomial below
# |x| = 0.625, tanh_f from there on.  Its bound is the figure its source states, in ulp of the result.
TANH_ACT_SPLIT, TANH_ACT_SAT, TANH_ACT_TOP = F32(0.625), F32(9.0), F32(16.0)
TANH_ACT_STRIDE, TANH_ACT_NEAR = 256, 4096
TANH_ACT_BOUND_ULP = 2.3
_TANH_ACT_SET = None


def tanh_act_set():
    """every 256th bit pattern of the positive normal floats below 16 and every pattern within 4096 of 0.625 and of 9,
    with their negatives, and SPECIALS (larger than MAX_SET, so not one of all_sets(); built once, read-only)"""
    global _TANH_ACT_SET
    if _TANH_ACT_SET is None:
        lo, hi = int(f2u(FLT_MIN)[0]), int(f2u(TANH_ACT_TOP)[0])
        near = [np.arange(int(f2u(p)[0]) - TANH_ACT_NEAR, int(f2u(p)[0]) + TANH_ACT_NEAR + 1, dtype=np.int64)
                for p in (TANH_ACT_SPLIT, TANH_ACT_SAT)]
        pos = u2f(np.concatenate([np.arange(lo, hi, TANH_ACT_STRIDE, dtype=np.int64)] + near).astype(U32))
        _TANH_ACT_SET = np.concatenate([both_signs(pos), SPECIALS])
        _TANH_ACT_SET.setflags(write=False)
    return _TANH_ACT_SET


def tanh_act32(x, tanh_f):
    """tanh_act in numpy float32, each fmaf taken through float64 (the product of two float32 is exact there); `tanh_f`:
    the float32 tanh_f it hands |x| >= 0.625 to (the C checker's twin)"""
    x = np.asarray(x, F32)
    d = np.float64
    with np.errstate(all="ignore"):
        fma = lambda a, b, c: (np.asarray(a, F32).astype(d) * np.asarray(b, F32).astype(d) + np.asarray(c, F32).astype(d)).astype(F32)  # noqa: E731
        z = x * x
        p = fma(z, F32(-5.70498872745e-3), F32(2.06390887954e-2))
        p = fma(z, p, F32(-5.37397155531e-2))
        p = fma(z, p, F32(1.33314422036e-1))
        p = fma(z, p, F32(-3.33332819422e-1))
        small = np.copysign(fma(z * x, p, x), x)
        assert z.dtype == F32 and small.dtype == F32
        return np.where(np.abs(x) < TANH_ACT_SPLIT, small, np.asarray(tanh_f(x), F32))


def check_tanh_act(x, y, who):
    """what tests/test_math64.py (the restatement) and tests/test_gpu_fisher.py (the device) both ask of y = tanh_act(x)
    over tanh_act_set(); prints and returns the worst error of each branch in ulp of the result"""
    x, y = np.asarray(x, F32), np.asarray(y, F32)
    assert x.shape == y.shape and y.dtype == F32
    nan = np.isnan(x)
    assert nan.sum() >= 1 and np.isnan(y[nan]).all() and not np.isnan(y[~nan]).any()            # NaN in, NaN out, only there
    assert (y[x == np.inf] == 1).all() and (y[x == -np.inf] == -1).all() and np.isinf(x).sum() >= 2
    zero = x == 0
    assert zero.sum() >= 2 and (f2u(y[zero]) == f2u(x[zero])).all(), "+-0 keeps its sign"
    den = (x != 0) & (np.abs(x) < FLT_MIN)
    assert den.sum() >= 4 and (f2u(y[den]) == f2u(x[den])).all(), "denormals are kept: tanh_act(x) = x there"
    # odd: the set holds -x for every x
    ub, first = np.unique(f2u(x[~nan]), return_index=True)
    yb = f2u(y[~nan])[first]
    neg = ub ^ U32(0x80000000)
    at = np.searchsorted(ub, neg)
    assert (ub[at] == neg).all()
    assert (yb[at] == yb ^ U32(0x80000000)).all(), "tanh_act(-x) = -tanh_act(x), bit for bit"
    assert (np.abs(y[~nan]) <= 1).all()
    fin = np.isfinite(x)                                       # (+-inf and NaN: exact, above)
    x, y = x[fin], y[fin]
    ref = ref_tanh(x)
    ulp = ulp_err(y, ref)
    ax = np.abs(x)
    out = {}
    for name, sel in (("below 0.625", ax < TANH_ACT_SPLIT), ("0.625 and above", ax >= TANH_ACT_SPLIT)):
        i = np.flatnonzero(sel)[np.argmax(ulp[sel])]
        out[name] = float(ulp[i])
        print("%s tanh_act %-16s worst %.3f ulp at x = %r (%08x): got %r, float64 %r; bound %.1f, %d inputs"
              % (who, name, ulp[i], float(x[i]), f2u(x[i:i + 1])[0], float(y[i]), float(ref[i]), TANH_ACT_BOUND_ULP, sel.sum()))
    assert ulp.max() <= TANH_ACT_BOUND_ULP, out
    big = ax >= TANH_ACT_SPLIT
    assert abs_err(y[big], ref[big]).max() <= BOUNDS["tanh"]                                   # tanh_f's own bound
    return out


RCP_EXPS = range(-149, 128)


def rcp_set():
    """every binade, denormals included, both signs: the operand of 1.0f / x and of sqrtf"""
    rng = np.random.default_rng(140)
    return _sized(np.concatenate([binades(RCP_EXPS, rng), SPECIALS]))


RCP_UNSCALED_MAX = F32(2.0 ** 126)


def rcp_unscaled_set():
    """rcp_unscaled's stated domain: +-0, +-inf, NaN and 2^-126 <= |d| <= 2^126 (with the last values below 2^126)"""
    x = np.concatenate([rcp_set(), both_signs(neighbours([2.0 ** 126], 2))])
    a = np.abs(x)
    return _sized(x[(a == 0) | ~np.isfinite(x) | ((a >= FLT_MIN) & (a <= RCP_UNSCALED_MAX))])


PAIR_N, PAIR_EXP = 1 << 19, 120
GRID = np.stack(np.meshgrid(SPECIALS, SPECIALS, indexing="ij"), -1).reshape(-1, 2)


def _rand_floats(rng, e):
    """random sign and mantissa at the exponents e"""
    n = e.size
    b = ((e + 127).astype(np.uint64) << np.uint64(23)) | rng.integers(0, 1 << 23, n, dtype=np.uint64) | \
        (rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(31))
    return u2f(b.astype(U32))


def pair_set():
    """(a, b) operand pairs for a / b and atan2(a, b): independent exponents in +-120 (quotients from 2^-240 to 2^240: every
    overflow, underflow and denormal quotient), exponents within 4 of each other (quotients near 1: the body of atan2's
    polynomial), random bit patterns (denormal operands, NaNs and infinities among them), denormal over small normal, the
    uniform square of the older test, and the grid of SPECIALS"""
    rng = np.random.default_rng(150)
    e1 = rng.integers(-PAIR_EXP, PAIR_EXP + 1, PAIR_N)
    a1, b1 = _rand_floats(rng, e1), _rand_floats(rng, rng.integers(-PAIR_EXP, PAIR_EXP + 1, PAIR_N))
    e2 = rng.integers(-PAIR_EXP, PAIR_EXP + 1, PAIR_N)
    a2, b2 = _rand_floats(rng, e2), _rand_floats(rng, np.clip(e2 + rng.integers(-4, 5, PAIR_N), -126, 127))
    a3, b3 = (u2f(rng.integers(0, 1 << 32, PAIR_N // 2, dtype=np.uint64).astype(U32)) for _ in range(2))
    a4 = both_signs(u2f(rng.integers(1, 1 << 23, PAIR_N // 8, dtype=np.uint64).astype(U32)))     # denormal numerators
    b4 = _rand_floats(rng, rng.integers(-126, 3, PAIR_N // 4))
    a5, b5 = (rng.uniform(-5, 5, PAIR_N // 2).astype(F32) for _ in range(2))
    a = np.concatenate([a1, a2, a3, a4, b4, a5, GRID[:, 0]])
    b = np.concatenate([b1, b2, b3, b4, a4, b5, GRID[:, 1]])
    return _sized(a), _sized(b)


DIV_BIN_MIN = F32(2.0 ** -100)
DIV_BIN_EXPS = range(-100, 3)


def div_bin16_set():
    """div_bin16's stated domain: 2^-100 <= |x| <= 2 pi, +0 and NaN; the first values from 2^-100 and the last up to 2 pi"""
    rng = np.random.default_rng(160)
    x = np.concatenate([binades(DIV_BIN_EXPS, rng), both_signs(neighbours([2.0 ** -100, float(TWO_PI_F)], 4)),
                        F32([0.0, np.nan])])
    a = np.abs(x)
    keep = ((a >= DIV_BIN_MIN) & (a <= TWO_PI_F)) | (f2u(x) == 0) | np.isnan(x)
    return _sized(x[keep])


# normal_pair: the noise seed and a grid of (env, counter) with 0 and 2^32 - 1 in both fields
NOISE_SEED = (0x243F6A88, 0x85A308D3)
_EDGE_U32 = np.array([0, 1, 2, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF], np.uint64)
# Counters (env, ctr) under NOISE_SEED whose first Threefry word b0 has b0 >> 8 == 0xFFFFFF (u1 = 1: radius 0) and
# b0 >> 8 == 0 (u1 = 2^-24: the largest radius, sqrt(48 ln 2) = 5.768).  Found once on the CPU by find_extreme_counters()
# over env < 128, ctr < 2^20 (2^27 counters); tests/test_math64.py re-verifies the property.
U1_ONE_COUNTERS = ((31, 986721), (61, 354013), (65, 886416), (87, 527408), (104, 713875), (108, 603438), (120, 205675),
                   (125, 924313))
U1_MIN_COUNTERS = ((13, 816157), (36, 694784), (43, 524275), (80, 795702), (92, 343977), (126, 991111))


def find_extreme_counters(envs=128, ctrs=1 << 20):
    """the search that produced U1_ONE_COUNTERS / U1_MIN_COUNTERS (about a minute of numpy)"""
    from oracle import policy64
    one, low = [], []
    ctr = np.arange(ctrs, dtype=np.uint64)
    for env in range(envs):
        t = policy64.threefry2x32(NOISE_SEED[0], NOISE_SEED[1], np.uint64(env), ctr)[0] >> 8
        one += [(env, int(c)) for c in ctr[t == 0xFFFFFF]]
        low += [(env, int(c)) for c in ctr[t == 0]]
    return tuple(one), tuple(low)


def normal_pair_set():
    """(env, ctr) uint32 arrays: the edge grid, a dense block of small counters (the rollouts' own: env < 256,
    ctr = step * 16 + pair), random 32-bit counters and the committed extreme ones"""
    rng = np.random.default_rng(170)
    ge, gc = (g.reshape(-1) for g in np.meshgrid(_EDGE_U32, _EDGE_U32, indexing="ij"))
    de, dc = (g.reshape(-1) for g in np.meshgrid(np.arange(256, dtype=np.uint64), np.arange(1024, dtype=np.uint64), indexing="ij"))
    re, rc = (rng.integers(0, 1 << 32, 1 << 18, dtype=np.uint64) for _ in range(2))
    xe, xc = (np.array([c[i] for c in U1_ONE_COUNTERS + U1_MIN_COUNTERS], np.uint64) for i in range(2))
    return np.concatenate([ge, de, re, xe]).astype(U32), np.concatenate([gc, dc, rc, xc]).astype(U32)


# ---------------------------------------------------------------------------------------------------------------------
# error measures: every element is measured; a NaN on one side only, or a wrong infinity, is an infinite error
# ---------------------------------------------------------------------------------------------------------------------
def abs_err(got, ref):
    """|got - ref| elementwise (float64); 0 where both are NaN or the same infinity, inf where only one is / they differ"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore"):
        err = np.abs(got - ref)
    odd = ~np.isfinite(got) | ~np.isfinite(ref)
    same = (np.isnan(got) & np.isnan(ref)) | (got == ref)
    return np.where(odd, np.where(same, 0.0, np.inf), err)


def rel_err(got, ref, floor=0.0):
    """abs_err / max(|ref|, floor); where that denominator is 0 or infinite: 0 if got == ref, else inf"""
    ref = np.asarray(ref, np.float64)
    a = abs_err(got, ref)
    den = np.maximum(np.abs(ref), floor)
    ok = np.isfinite(den) & (den > 0)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(ok, a / np.where(ok, den, 1.0), np.where(a == 0, 0.0, np.inf))


def ulp_err(got, ref):
    """abs_err in units of the fp32 spacing at ref"""
    ref = np.asarray(ref, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        ulp = np.spacing(np.abs(ref).astype(F32)).astype(np.float64)
    return abs_err(got, ref) / ulp


SINCOS_BANDS = (("pi", float(np.pi)), ("1e4", 1e4), ("1e5", 1e5), ("2^24", 2.0 ** 24))


def sincos_band(x):
    """index into SINCOS_BANDS of every x (disjoint: the first band whose edge is >= |x|); -1 beyond 2^24 and for NaN"""
    a = np.abs(np.asarray(x, np.float64))
    idx = np.full(a.shape, -1)
    for i in reversed(range(len(SINCOS_BANDS))):
        idx[a <= SINCOS_BANDS[i][1]] = i
    return idx


def ref_sincos(x):
    """float64 (sin, cos); NaN for NaN and +-inf.  Beyond 2^24 sincos_f states its result instead of computing one: a
    finite |x| > 2^24 is taken as a zero of x's sign, so (+-0, 1) is the reference there"""
    xd = np.asarray(x, np.float64)
    with np.errstate(invalid="ignore"):
        xd = np.where(np.isfinite(xd) & (np.abs(xd) > 2.0 ** 24), np.copysign(0.0, xd), xd)
        return np.sin(xd), np.cos(xd)


def ref_exp(x):
    """float64 exp inside exp_f's range; its stated ends outside: 0 below -87, inf above 88"""
    xd = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        t = np.exp(xd)
    return np.where(xd < -87.0, 0.0, np.where(xd > 88.0, np.inf, t))


def ref_log(x):
    return np.log(np.asarray(x, np.float64))


def ref_tanh(x):
    return np.tanh(np.asarray(x, np.float64))


def ref_atan2(y, x):
    with np.errstate(invalid="ignore"):                   # (signalling NaNs among the random bit patterns)
        return np.arctan2(np.asarray(y, np.float64), np.asarray(x, np.float64))


def exact_div(a, b):
    with np.errstate(all="ignore"):
        return np.asarray(a, F32) / np.asarray(b, F32)


def exact_rcp(x):
    return exact_div(F32(1.0), x)


def exact_sqrt(x):
    with np.errstate(all="ignore"):
        return np.sqrt(np.asarray(x, F32))


def exact_div_bin16(x):
    return exact_div(x, BIN_SIZE16)


def ref_normal_pair(env, ctr):
    """(z0, z1, bound) of oracle/policy64.normal_pair under NOISE_SEED: its bound is the measure it uses for the pair"""
    from oracle import policy64
    return policy64.normal_pair(NOISE_SEED, np.asarray(env, np.uint64), np.asarray(ctr, np.uint64))


def measures(sets, fns):
    """{name: worst error} of the fp32 implementation `fns` over `sets`, in the measures BOUNDS is written in.
    sets: dict of the arrays (see all_sets()); fns: dict of callables
        sincos(x) -> (s, c); atan2(y, x); exp(x); log(x); tanh(x)
    A key of fns that is missing is not measured."""
    out = {}
    if "sincos" in fns:
        x = sets["sincos"]
        s, c = fns["sincos"](x)
        rs, rc = ref_sincos(x)
        es, ec, band = abs_err(s, rs), abs_err(c, rc), sincos_band(x)
        for i, (name, _) in enumerate(SINCOS_BANDS):
            out["sin<=" + name] = es[band == i].max()
            out["cos<=" + name] = ec[band == i].max()
        if (band < 0).any():                                                    # NaN / inf in: NaN out, nothing else
            out["sincos:beyond"] = max(es[band < 0].max(), ec[band < 0].max())
    if "atan2" in fns:
        y, x = sets["pair"]
        out["atan2"] = abs_err(fns["atan2"](y, x), ref_atan2(y, x)).max()
    if "exp" in fns:
        x = sets["exp"]
        out["exp"] = rel_err(fns["exp"](x), ref_exp(x)).max()
    if "log" in fns:
        x = sets["log"]
        got, ref = fns["log"](x), ref_log(x)
        out["log:rel"] = rel_err(got, ref, 1e-3).max()
        out["log:ulp"] = ulp_err(got, ref).max()
    if "tanh" in fns:
        x = sets["tanh"]
        out["tanh"] = abs_err(fns["tanh"](x), ref_tanh(x)).max()
    return out


_SETS = None


def all_sets():
    """every set, built once per process and shared (read-only) by the tests that need it"""
    global _SETS
    if _SETS is None:
        _SETS = dict(sincos=sincos_set(), exp=exp_set(), log=log_set(), tanh=tanh_set(), rcp=rcp_set(),
                     rcp_unscaled=rcp_unscaled_set(), pair=pair_set(), div_bin16=div_bin16_set(),
                     normal_pair=normal_pair_set())
        for v in _SETS.values():
            for a in (v if isinstance(v, tuple) else (v,)):
                a.setflags(write=False)
    return _SETS


def checker_fns(oracle):
    """the C checker's twins (oracle/gx_oracle.c through oracle/gxo.py) in the shape measures() takes"""
    z = lambda x: np.zeros(np.size(x), F32)   # noqa: E731
    return dict(sincos=lambda x: oracle.math_probe(x, z(x))[:2], atan2=lambda y, x: oracle.math_probe(x, y)[2],
                exp=lambda x: oracle.math_probe(x, z(x))[3], log=lambda x: oracle.math_probe2(x)[0],
                tanh=lambda x: oracle.math_probe2(x)[1])


# ---------------------------------------------------------------------------------------------------------------------
# BOUNDS = the checker's measured worst error x 1.25, rounded up to two digits  (measured | bound | the project's older
# bound on the same range, which no bound here exceeds)
# ---------------------------------------------------------------------------------------------------------------------
BOUNDS = {
    # sin / cos, absolute, by |x| (disjoint bands)        checker measured | bound   | older bound
    "sin<=pi": 1.1e-7,       # |x| <= pi                        8.367e-08  | 1.1e-07 | 1.3e-7
    "cos<=pi": 1.2e-7,       #                                  9.016e-08  | 1.2e-07 | 1.3e-7
    "sin<=1e4": 1.2e-7,      # pi < |x| <= 1e4                  9.127e-08  | 1.2e-07 | 1.3e-7
    "cos<=1e4": 1.2e-7,      #                                  9.121e-08  | 1.2e-07 | 1.3e-7
    "sin<=1e5": 1.2e-7,      # 1e4 < |x| <= 1e5                 9.294e-08  | 1.2e-07 | 1e-6
    "cos<=1e5": 1.2e-7,      #                                  9.140e-08  | 1.2e-07 | 1e-6
    # 1e5 < |x| <= 2^24: still 8.0e-8 up to 2^20, then 2.8e-7 to 2^21, 2.3e-6 to 2^22, 6.0e-5 to 2^23, 2.0e-4 to 2^24: the
    # fp32 product x * (2 / pi) has a spacing of 1/2 and then 1 up there, so k = rintf(it) misses the nearest multiple of
    # pi / 2 by one (x = 13110559: 8346440.5 for 8346441.086), |r| reaches 1.7 and the polynomials fitted on pi / 4 are
    # off by 1e-4.  About a thousand times the small-angle error; the angles of the robots never get there.  Written down
    # so that a change of the reduction is held to it.
    "sin<=2^24": 2.6e-4,     #                                  2.000e-04  | 2.6e-04 | none
    "cos<=2^24": 5.1e-5,     #                                  4.045e-05  | 5.1e-05 | none
    "sincos:beyond": 0.0,    # NaN / inf -> NaN, finite beyond 2^24 -> (+-0, 1): exact
    "atan2": 3.3e-7,         # absolute                         2.577e-07  | 3.3e-07 | 3.6e-7
    "exp": 1.1e-7,           # relative, on [-87, 88]           8.231e-08  | 1.1e-07 | 1.6e-7
    "log:rel": 1.9e-7,       # relative to max(|t|, 1e-3)       1.514e-07  | 1.9e-07 | 3e-7
    "log:ulp": 2.3,          # in ulp of the result             1.824      | 2.3     | none
    "tanh": 1.5e-7,          # absolute                         1.179e-07  | 1.5e-07 | 2.5e-7
}
# (the bound of normal_pair is elementwise: the third value of oracle/policy64.normal_pair, as in tests/test_policy64.py)
# what the older tests hold the same functions to (tests/test_oracle_math.py, tests/test_policy_rollout.py)
OLDER_BOUNDS = {"sin<=pi": 1.3e-7, "cos<=pi": 1.3e-7, "sin<=1e4": 1.3e-7, "cos<=1e4": 1.3e-7, "sin<=1e5": 1e-6, "cos<=1e5": 1e-6,
                "atan2": 3.6e-7, "exp": 1.6e-7, "log:rel": 3e-7, "tanh": 2.5e-7}


def bound_from(measured):
    """measured x 1.25 rounded UP to two significant digits"""
    from decimal import Decimal, ROUND_CEILING
    d = Decimal(repr(float(measured))) * Decimal("1.25")
    q = Decimal(1).scaleb(d.adjusted() - 1)
    return float((d / q).to_integral_value(rounding=ROUND_CEILING) * q)


if __name__ == "__main__":
    from oracle import gxo
    gxo.lib()
    for k, v in measures(all_sets(), checker_fns(gxo)).items():
        print("%-14s measured %.4g   x 1.25 -> %.2g" % (k, v, bound_from(v) if np.isfinite(v) and v > 0 else v))
