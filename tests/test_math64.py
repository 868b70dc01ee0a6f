"""The C checker's fp32 sin / cos / atan2 / exp / log / tanh (oracle/gx_oracle.c, the twins of gx_device.h's) against
float64 over whole domains: binade sweeps, the neighbours of every range-reduction tie, the specials (tests/math64.py).
tests/test_gpu_math64.py puts the same arrays through the device's primitives.

The bounds are the checker's own measured worst errors x 1.25 (math64.BOUNDS); this module is where they are measured and
where two deliberate behaviours are written down: tanh has absolute, not relative, accuracy near 0, and sin / cos lose
three digits between 1e5 and 2^24."""
import numpy as np
import pytest

import math64 as m

F32 = np.float32


@pytest.fixture(scope="module")
def sets():
    return m.all_sets()


@pytest.fixture(scope="module")
def measured(oracle, sets):
    return m.measures(sets, m.checker_fns(oracle))


def test_checker_is_within_the_bounds_of_float64(measured):
    for k, v in measured.items():
        print("%-14s measured %.4g  bound %.2g  (%.0f %%)" % (k, v, m.BOUNDS[k], 100 * v / m.BOUNDS[k] if m.BOUNDS[k] else 0))
    assert sorted(measured) == sorted(m.BOUNDS)
    for k, v in measured.items():
        assert v <= m.BOUNDS[k], (k, v, m.BOUNDS[k])


def test_the_bounds_are_the_measured_errors_times_five_quarters(measured):
    """each bound is the checker's worst error over the committed sets x 1.25 rounded up to two digits -- no looser -- and
    none exceeds what the older tests hold the same function to on the same range"""
    for k, v in measured.items():
        want = m.bound_from(v) if v > 0 else 0.0
        assert np.isclose(m.BOUNDS[k], want, rtol=1e-9, atol=0), (k, v, want, m.BOUNDS[k])
    for k, old in m.OLDER_BOUNDS.items():
        assert m.BOUNDS[k] <= old, k
    assert m.bound_from(8.6e-8) == 1.1e-7 and m.bound_from(2.0e-4) == 2.5e-4 and m.bound_from(1.001e-7) == 1.3e-7


def test_the_bounds_notice_one_ulp(oracle, sets):
    """an implementation whose every result lies one fp32 step further from zero than the checker's misses every bound
    but tanh's: the bounds are tight enough to see the last bit.  (tanh's worst errors are at results below 1/2, where the
    steps of fp32 are finer than the 2^-24 its results are made of: one such step stays inside -- 1.497e-7 of 1.5e-7.)"""
    chk = m.checker_fns(oracle)
    out = lambda v: np.nextafter(v, np.where(np.signbit(v), F32(-np.inf), F32(np.inf)))      # noqa: E731
    off = dict(sincos=lambda x: tuple(out(v) for v in chk["sincos"](x)), atan2=lambda y, x: out(chk["atan2"](y, x)),
               exp=lambda x: out(chk["exp"](x)), log=lambda x: out(chk["log"](x)))
    worse = m.measures(sets, off)
    for k in ("sin<=pi", "cos<=pi", "sin<=1e4", "cos<=1e4", "sin<=1e5", "cos<=1e5", "atan2", "exp", "log:rel", "log:ulp"):
        assert worse[k] > m.BOUNDS[k], (k, worse[k])


def test_large_angles_lose_three_digits_and_no_more(measured):
    """1e5 < |x| <= 2^24 has a bound of its own, about 1000 times the small-angle one (math64.BOUNDS says why)"""
    for f in ("sin", "cos"):
        assert measured[f + "<=2^24"] <= m.BOUNDS[f + "<=2^24"]
        assert measured[f + "<=2^24"] > 100 * measured[f + "<=1e5"]          # it is there: not a bound nobody needs
    assert 1000 * m.BOUNDS["sin<=pi"] < m.BOUNDS["sin<=2^24"] < 3000 * m.BOUNDS["sin<=pi"]


def test_tanh_is_absolutely_not_relatively_accurate_near_zero(oracle, sets):
    """tanh of any |x| < 2^-26 is a zero of x's sign or within one 2^-24 step of it: 1 - 2 / (exp(2|x|) + 1) cannot give
    anything finer, and the policy's hidden units do not need it"""
    x = sets["tanh"]
    x = x[np.abs(x) < m.TANH_TINY]
    assert x.size > 2 * 90 * m.PER and (x == 0).sum() == 2 and (np.abs(x) < m.FLT_MIN).sum() >= 6
    t = oracle.math_probe2(x)[1]
    assert (np.signbit(t) == np.signbit(x)).all()
    assert (np.abs(t) <= F32(2.0 ** -24)).all()
    assert (t[x == 0] == 0).all()
    # and the steps are what the results are made of well above that: 2^-24 divides every result below 1/2
    y = sets["tanh"]
    y = y[np.abs(y) < 0.5]
    q = oracle.math_probe2(y)[1].astype(np.float64) * 2.0 ** 24
    assert (q == np.rint(q)).all()


def test_specials_exact(oracle):
    f = oracle.math_probe
    x = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], F32)
    s, c, _, _ = f(x, np.zeros_like(x))
    assert s[0] == 0 and c[0] == 1 and s[1] == 0 and c[1] == 1
    assert np.isnan(s[2:]).all() and np.isnan(c[2:]).all()
    s, c, _, _ = f(F32([m.FLT_MAX, -m.FLT_MAX, 2.0 ** 25]), np.zeros(3, F32))          # beyond 2^24: taken as 0
    assert (s == 0).all() and (c == 1).all()
    # atan2: quadrants, signed zeros, infinities, NaN through
    xs = np.array([1, -1, 0, 0, -1, -1, 0.0, -0.0, np.inf, -np.inf, np.nan, 1.0], F32)
    ys = np.array([0, 0, 1, -1, 0.0, -0.0, 0.0, 0.0, np.inf, np.inf, 1.0, np.nan], F32)
    _, _, a, _ = f(xs, ys)
    want = np.arctan2(ys.astype(np.float64), xs.astype(np.float64))
    np.testing.assert_allclose(a[:-2], want[:-2], atol=3e-7)
    assert np.isnan(a[-2:]).all()
    assert np.signbit(a[5]) and abs(a[5] + np.pi) < 3e-7                                # atan2(-0, -1) = -pi
    assert a[6] == 0 and not np.signbit(a[6]) and abs(a[7] - np.pi) < 3e-7              # atan2(0, +-0)
    assert a[0] == 0 and abs(a[1] - np.pi) < 3e-7 and abs(a[2] - np.pi / 2) < 3e-7 and abs(a[3] + np.pi / 2) < 3e-7
    # exp: flushed below -87, inf above 88, no subnormal and no early inf in between
    xe = np.array([0.0, -87.5, -1000.0, -np.inf, np.nan, 88.5, np.inf, -87.0, 88.0], F32)
    _, _, _, e = f(xe, np.zeros_like(xe))
    assert e[0] == 1 and e[1] == 0 and e[2] == 0 and e[3] == 0 and np.isnan(e[4]) and np.isinf(e[5]) and np.isinf(e[6])
    assert e[7] >= m.FLT_MIN and np.isfinite(e[8])
    # tanh: saturation, signed zeros, NaN through
    xt = np.array([0.0, -0.0, 9.0, -9.0, 9.5, -9.5, 1e30, -1e30, np.inf, -np.inf, np.nan], F32)
    t = oracle.math_probe2(xt)[1]
    assert t[0] == 0 and not np.signbit(t[0]) and t[1] == 0 and np.signbit(t[1])
    assert 0 < 1 - t[2] < 1e-7 and t[3] == -t[2]
    assert list(t[4:10]) == [1, -1, 1, -1, 1, -1] and np.isnan(t[10])
    # log: exact at 1, the ends of the normal range finite
    lg = oracle.math_probe2(F32([1.0, m.FLT_MIN, m.FLT_MAX]))[0]
    assert lg[0] == 0 and abs(lg[1] + 126 * np.log(2)) < 1e-4 and abs(lg[2] - 128 * np.log(2)) < 1e-4


def test_exp_has_no_inf_and_no_subnormal_inside_its_range(oracle, sets):
    x = sets["exp"]
    e = oracle.math_probe(x, np.zeros_like(x))[3]
    inside = (x >= m.EXP_LO) & (x <= m.EXP_HI)
    assert inside.sum() > 1000000
    assert np.isfinite(e[inside]).all() and (e[inside] >= m.FLT_MIN).all()
    assert (e[x < m.EXP_LO] == 0).all() and np.isinf(e[x > m.EXP_HI]).all() and np.isnan(e[np.isnan(x)]).all()


def test_extreme_counters_have_the_stated_threefry_property():
    from oracle import policy64
    assert len(m.U1_ONE_COUNTERS) >= 2 and len(m.U1_MIN_COUNTERS) >= 2
    for counters, top in ((m.U1_ONE_COUNTERS, 0xFFFFFF), (m.U1_MIN_COUNTERS, 0)):
        env, ctr = (np.array([c[i] for c in counters], np.uint64) for i in range(2))
        b0, _ = policy64.threefry2x32(m.NOISE_SEED[0], m.NOISE_SEED[1], env, ctr)
        assert (b0 >> 8 == top).all()
    z0, z1, _ = m.ref_normal_pair(*zip(*m.U1_ONE_COUNTERS))
    assert (z0 == 0).all() and (z1 == 0).all()                                          # u1 = 1: radius 0
    z0, z1, _ = m.ref_normal_pair(*zip(*m.U1_MIN_COUNTERS))
    np.testing.assert_allclose(np.hypot(z0, z1), np.sqrt(48 * np.log(2.0)), rtol=1e-14)   # u1 = 2^-24: the largest radius
    env, ctr = m.all_sets()["normal_pair"]
    have = set(zip(env.tolist(), ctr.tolist()))
    assert set(m.U1_ONE_COUNTERS) | set(m.U1_MIN_COUNTERS) <= have
    assert {(a, b) for a in (0, 0xFFFFFFFF) for b in (0, 0xFFFFFFFF)} <= have


def _has(x, values):
    """every value (by its bits, so that NaN and -0 count) occurs in x"""
    return np.isin(m.f2u(np.asarray(values, F32)), m.f2u(x)).all()


def test_every_set_has_the_size_and_the_points_it_promises(sets):
    nb = lambda exps, signs=2: signs * sum(m.binade_count(e) for e in exps)      # noqa: E731
    S = len(m.SPECIALS)
    assert S == 13 and len({int(b) for b in m.f2u(m.SPECIALS)}) == 13
    assert m.binade_count(-149) == 1 and m.binade_count(-140) == 512 and m.binade_count(-126) == m.PER + m.EDGE == 4096
    # sincos
    x = sets["sincos"]
    assert x.size == nb(m.SINCOS_EXPS) + 2 + 2 * 3 * (m.SINCOS_K_SEQ + m.SINCOS_K_RAND) + S + 3 * m.SINCOS_DENSE
    k = np.array([1, 2, 3, 1000, m.SINCOS_K_SEQ, m.SINCOS_K_MAX], np.float64)
    assert _has(x, m.neighbours(k[:-1] * (np.pi / 2))) and _has(x, -m.neighbours(k[:-1] * (np.pi / 2)))
    assert _has(x, [2.0 ** 24, -2.0 ** 24, np.nextafter(F32(2.0 ** 24), F32(0)), 2.0 ** -126]) and _has(x, m.SPECIALS)
    band = m.sincos_band(x)
    assert [int((band == i).sum()) > 500000 for i in range(4)] == [True] * 4 and (band < 0).sum() == 5
    assert np.abs(x[np.isfinite(x) & (band >= 0)]).max() == 2.0 ** 24
    # exp
    x = sets["exp"]
    ties = m.exp_ties()
    assert x.size == nb(m.EXP_EXPS) + m.EXP_LIN + ties.size + 2 * 9 + S
    assert ties.size >= 3 * (len(m.EXP_K) - 4) and ties.min() < -86.5 and ties.max() > 87.5
    assert _has(x, m.neighbours([-87.0, 88.0], 4)) and _has(x, m.neighbours([0.5 * np.log(2.0), -0.5 * np.log(2.0)]))
    assert _has(x, m.SPECIALS) and (x[np.isfinite(x)] < -87).sum() >= 4 and (x[np.isfinite(x)] > 88).sum() >= 4
    # log
    x = sets["log"]
    assert x.size == nb(m.LOG_EXPS, 1) + 17 * len(m.LOG_SPLIT_EXPS) + 9 + 2
    assert (x >= m.FLT_MIN).all() and np.isfinite(x).all() and _has(x, [m.FLT_MIN, m.FLT_MAX, 1.0])
    assert _has(x, [m.LOG_SPLIT, np.nextafter(m.LOG_SPLIT, F32(2)), np.nextafter(m.LOG_SPLIT, F32(1)),
                    m.LOG_SPLIT * F32(2.0 ** 64), np.nextafter(m.LOG_SPLIT, F32(2)) * F32(2.0 ** -126)])
    # tanh
    x = sets["tanh"]
    ties = m.tanh_ties()
    assert x.size == nb(m.TANH_EXPS) + m.TANH_LIN + ties.size + S and ties.size == 2 * 3 * 27 + 2 * 9
    assert _has(x, m.neighbours([9.0, -9.0], 4)) and _has(x, m.neighbours([0.25 * np.log(2.0), 13.25 * np.log(2.0)]))
    assert _has(x, m.SPECIALS) and np.abs(x[np.isfinite(x)]).max() == m.FLT_MAX and (np.abs(x) > 9).sum() > 1000
    # rcp / sqrt: every binade with its ends, denormals included
    x = sets["rcp"]
    assert x.size == nb(m.RCP_EXPS) + S
    assert _has(x, m.SPECIALS) and (np.abs(x[x != 0]) < m.FLT_MIN).sum() > 2 * 8 * m.PER
    for e in (-149, -148, -127, -126, 0, 126, 127):
        lo, hi = m.binade_bits(e)
        assert _has(x, m.u2f([lo, hi, lo | 0x80000000, hi | 0x80000000])), e
    # rcp_unscaled: its domain and nothing else, with both ends
    x = sets["rcp_unscaled"]
    a = np.abs(x)
    assert ((a == 0) | ~np.isfinite(x) | ((a >= m.FLT_MIN) & (a <= m.RCP_UNSCALED_MAX))).all()
    # (+-2^126 as the first value of its binade; it and the two values below it again as neighbours; +-0, +-inf, NaN, +-FLT_MIN)
    assert x.size == nb(range(-126, 126)) + 2 + 2 * 3 + 7
    assert _has(x, [m.FLT_MIN, -m.FLT_MIN, 2.0 ** 126, -2.0 ** 126, np.nextafter(F32(2.0 ** 126), F32(0)), 0.0, -0.0, np.inf,
                    -np.inf, np.nan])
    # operand pairs
    a, b = sets["pair"]
    assert a.size == b.size == 2 * m.PAIR_N + 3 * (m.PAIR_N // 2) + S * S
    q = m.exact_div(a, b)
    fin = np.isfinite(a) & np.isfinite(b) & (a != 0) & (b != 0)
    den = lambda v: (v != 0) & (np.abs(v) < m.FLT_MIN)      # noqa: E731
    assert (den(q) & fin).sum() > 10000 and (den(a) & fin).sum() > 10000 and (den(b) & fin).sum() > 10000
    assert (np.isinf(q) & fin).sum() > 10000 and ((q == 0) & fin).sum() > 10000 and np.isnan(a).sum() > 100
    assert ((np.abs(q) > 0.25) & (np.abs(q) < 4) & fin).sum() > 100000
    pairs = set(zip(m.f2u(a[-S * S:]).tolist(), m.f2u(b[-S * S:]).tolist()))
    assert len(pairs) == S * S
    # div_bin16: its domain and nothing else, with both ends
    x = sets["div_bin16"]
    a = np.abs(x)
    assert (((a >= m.DIV_BIN_MIN) & (a <= m.TWO_PI_F)) | (m.f2u(x) == 0) | np.isnan(x)).all()
    top = sum(m.binade_count(e) for e in range(-100, 2))
    assert 2 * top + 2 * m.EDGE // 2 < x.size <= 2 * top + 2 * m.binade_count(2) + 2 * 5 + 2 * 9 + 2
    assert _has(x, [2.0 ** -100, -2.0 ** -100, m.TWO_PI_F, -m.TWO_PI_F, np.nextafter(m.TWO_PI_F, F32(0)), 0.0, np.nan])
    assert not _has(x, [-0.0]) and (a > 4).sum() > 2000
    # normal_pair
    env, ctr = sets["normal_pair"]
    assert env.dtype == ctr.dtype == np.uint32
    assert env.size == ctr.size == 49 + 256 * 1024 + (1 << 18) + len(m.U1_ONE_COUNTERS) + len(m.U1_MIN_COUNTERS)
    assert max(v.size if not isinstance(v, tuple) else v[0].size for v in sets.values()) <= m.MAX_SET


def test_the_exact_references_are_float64_rounded_once(sets):
    """numpy's float32 /, 1 / x and sqrt are the correctly rounded results: the float64 operation rounded once to fp32
    (53 >= 2 * 24 + 2), denormal quotients and roots included"""
    a, b = sets["pair"]
    x = sets["rcp"]
    with np.errstate(all="ignore"):
        want_q = (a.astype(np.float64) / b.astype(np.float64)).astype(F32)
        want_r = (1.0 / x.astype(np.float64)).astype(F32)
        want_s = np.sqrt(x.astype(np.float64)).astype(F32)
        want_d = (sets["div_bin16"].astype(np.float64) / float(m.BIN_SIZE16)).astype(F32)
    for got, want in ((m.exact_div(a, b), want_q), (m.exact_rcp(x), want_r), (m.exact_sqrt(x), want_s),
                      (m.exact_div_bin16(sets["div_bin16"]), want_d)):
        nan = np.isnan(want)
        assert (np.isnan(got) == nan).all()
        assert (m.f2u(got)[~nan] == m.f2u(want)[~nan]).all()
    assert float(m.BIN_SIZE16) == float(F32(2 * np.pi / 16)) and m.f2u(m.TWO_PI_F)[0] == 0x40C90FDB


def test_error_measures_count_every_element():
    """a NaN on one side only, a wrong infinity or a wrong sign of infinity is an infinite error, never a skipped element"""
    nan, inf = np.nan, np.inf
    e = m.abs_err(F32([1.0, nan, nan, 1.0, inf, inf, -inf]), [1.5, nan, 1.0, nan, inf, -inf, 1.0])
    assert list(e) == [0.5, 0.0, inf, inf, 0.0, inf, inf]
    r = m.rel_err(F32([2.0, 0.0, 1e-30, inf, 3.0]), [1.0, 0.0, 0.0, inf, inf])
    assert list(r) == [1.0, 0.0, inf, 0.0, inf]
    assert list(m.ulp_err(F32([1.0 + 2.0 ** -22, 0.0]), [1.0, 0.0])) == [2.0, 0.0]
    assert list(m.sincos_band(F32([0.0, 3.0, 4.0, 1e4, 10001.0, 1e5, 2.0 ** 24, 2.0 ** 25, nan]))) == [0, 0, 1, 1, 2, 2, 3, -1, -1]


# ---------------------------------------------------------------------------------------------------------------------
# tanh_act, the Fisher product's activation (gx_fisher.hip): its numpy restatement over the set the device's goes through
# ---------------------------------------------------------------------------------------------------------------------
def test_the_tanh_act_set_has_the_points_it_promises():
    x = m.tanh_act_set()
    stride = (int(m.f2u(m.TANH_ACT_TOP)[0]) - int(m.f2u(m.FLT_MIN)[0])) // m.TANH_ACT_STRIDE
    assert x.size == 2 * (stride + 2 * (2 * m.TANH_ACT_NEAR + 1)) + len(m.SPECIALS) and 2000000 < x.size < 10000000
    assert _has(x, m.SPECIALS) and _has(x, [0.625, -0.625, 9.0, -9.0, m.FLT_MIN, 1.0, -1.0, 8.0])
    for p in (m.TANH_ACT_SPLIT, m.TANH_ACT_SAT):
        b = int(m.f2u(p)[0])
        assert _has(x, m.u2f([b - 4096, b - 1, b + 1, b + 4096, (b - 4096) | 0x80000000, (b + 4096) | 0x80000000]))
    fin = x[np.isfinite(x)]
    assert np.abs(fin[np.abs(fin) < m.FLT_MAX]).max() < 16.0 and (np.abs(fin) > 9).sum() > 50000
    assert (np.abs(fin) < 0.625).sum() > 1000000 and (np.abs(fin) < 2.0 ** -100).sum() > 100000


def test_tanh_act_restated_in_numpy_is_within_the_bound_its_source_states(oracle):
    """The polynomial below 0.625 with each fmaf through float64 and the checker's tanh_f above, over tanh_act_set(), held
    to the 2.3 ulp that gx_fisher.hip states: so the figure is reachable by the algorithm, and a miss on the device
    (tests/test_gpu_fisher.py, the same set and the same checks) is the kernel's.  Measured: 0.664 ulp at x = 0.4553 below 0.625
    and 1.286 ulp at x = 0.62522 above (the device's figures are the same).  Without the copysignf of the last line, x = -0 gives +0: (+0) + (-0)."""
    x = m.tanh_act_set()
    y = m.tanh_act32(x, lambda v: oracle.math_probe2(np.ascontiguousarray(v))[1])
    worst = m.check_tanh_act(x, y, "numpy")
    assert worst["below 0.625"] < worst["0.625 and above"] < m.TANH_ACT_BOUND_ULP
