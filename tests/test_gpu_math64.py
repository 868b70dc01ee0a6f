"""The device's fp32 math primitives, each evaluated by itself through libguardx_mathprobe.so (gxm_eval, gxm_normal_pair,
gxm_sweep; include/guardx_mathprobe.h), on the arrays of tests/math64.py -- the ones tests/test_math64.py puts through
the C checker.  Every element is compared; NaN positions must coincide.

  (a) against float64 within math64.BOUNDS: sincos_f<false>, sincos_f<true> (|x| <= 2^24), atan2_f, exp_f, log_f (normal
      inputs), tanh_f, normal_pair.  This verdict does not depend on the checker.
  (b) bit for bit against the checker's twin over the same sets, so that a failure says whether the kernel moved or both.
  (c) bit for bit against numpy's float32 (correctly rounded): x / y, 1.0f / x, sqrtf over binades, specials and
      denormals (operands and results) -- the build's "correctly rounded lowering" and its denormal mode; rcp_unscaled and
      div_bin16 on their stated domains.
  (d) all 2^32 bit patterns through gxm_sweep: rcp_unscaled against 1.0f / d, tanh_f against the checker's plain
      statement, sincos_f<true> against sincos_f<false>, div_bin16 against x / kBinSize16.  In-domain mismatches must be
      0; out of domain they are printed, and two are asserted > 0 because gx_device.h says those guards are needed.
So: by (c) the device's `/` is IEEE on the sets; by (d) the fast forms equal their plain forms everywhere they are used; by
(b) the plain forms equal the checker; by (a) both equal the true functions within written-down bounds.

The figures as these tests print them on an MI355X (HIP; they equal the C checker's of tests/test_math64.py digit for
digit, as (b) implies):
    function, measure                 band / range            worst       bound     of bound
    sin, absolute                     |x| <= pi               8.367e-08   1.1e-07   0.76
    cos                                                       9.016e-08   1.2e-07   0.75
    sin                               pi < |x| <= 1e4         9.127e-08   1.2e-07   0.76
    cos                                                       9.121e-08   1.2e-07   0.76
    sin                               1e4 < |x| <= 1e5        9.294e-08   1.2e-07   0.77
    cos                                                       9.140e-08   1.2e-07   0.76
    sin                               1e5 < |x| <= 2^24       2.000e-04   2.6e-04   0.77
    cos                                                       4.045e-05   5.1e-05   0.79
    sin / cos                         NaN, inf, beyond 2^24   0           0         (exact)
    (sincos_f<true> on |x| <= 2^24: the same eight figures)
    atan2, absolute                   exponents +-120         2.577e-07   3.3e-07   0.78
    exp, relative                     [-87, 88]               8.231e-08   1.1e-07   0.75
    log, rel. to max(|t|, 1e-3)       normal floats           1.514e-07   1.9e-07   0.80
    log, ulp of the result                                    1.824       2.3       0.79
    tanh, absolute                    all floats              1.179e-07   1.5e-07   0.79
    normal_pair, |z - z64|            524351 counters         1.56e-06    policy64  0.341
a / b: 1835177 pairs (38059 denormal quotients, 264262 with a denormal operand), 1.0f / x and sqrtf: 2179083 inputs (98306
denormal, 16384 with a denormal 1 / x), rcp_unscaled: 2064399, div_bin16: 840242 -- every one bit for bit.

The sweeps, patterns that differ of patterns tried (2^32 per pair; 1 to 5 ms each):
    rcp_unscaled     in domain             0 of 4244635652
                     denormal d     12582910 of   16777214   (all above 2^-128; below it both give inf)     asserted > 0
                     |d| > 2^126    33554430 of   33554430
    tanh_f           everywhere            0 of 4294967296
    sincos_f<true>   |x| <= 2^24           0 of 2533359618
                     beyond, NaN  1744830462 of 1761607678
    div_bin16        in domain             0 of 1737629623
                     below 2^-100    8627056 of  452984830   (1.9 %; from 0x000026ff = 1.4e-41 up)          asserted > 0
                     -0                    1 of          1
                     beyond 2 pi    23978060 of 2104352842   (from 0x7ec90fdb = 1.3e38 up: the residual overflows; and inf)
"""
import ctypes as C
import time

import numpy as np
import pytest

import math64 as m

pytestmark = pytest.mark.gpu

F32, U32 = np.float32, np.uint32


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch


@pytest.fixture(scope="module")
def sets():
    return m.all_sets()


class Probe:
    """the library and the device's result of every primitive over its set, evaluated once and shared"""

    def __init__(self, torch):
        from guardx_amd import _mathprobe_native as n
        self.torch, self.n, self.lib, self._cache = torch, n, n.load(), {}

    def _dev(self, a):
        return self.torch.from_numpy(np.array(a).view(np.int32)).cuda()        # (a copy: the shared sets are read-only)

    def eval(self, fn, x, y=None):
        """gxm_eval over numpy float32 arrays -> (out0, out1) numpy float32"""
        torch, n = self.torch, self.n
        xd = self._dev(x)
        yd = self._dev(y) if y is not None else None
        o0, o1 = torch.full_like(xd, 0x7FC00000), torch.full_like(xd, 0x7FC00000)
        n.check(self.lib.gxm_eval(fn, x.size, xd.data_ptr(), yd.data_ptr() if yd is not None else None, o0.data_ptr(),
                                  o1.data_ptr(), None))
        torch.cuda.synchronize()
        return o0.cpu().numpy().view(F32), o1.cpu().numpy().view(F32)

    def cached(self, key, fn, x, y=None):
        if key not in self._cache:
            self._cache[key] = self.eval(fn, x, y)
        return self._cache[key]

    def normal_pair(self, env, ctr):
        torch, n = self.torch, self.n
        ed, cd = self._dev(env), self._dev(ctr)
        z0, z1 = torch.full_like(ed, 0x7FC00000), torch.full_like(ed, 0x7FC00000)
        n.check(self.lib.gxm_normal_pair(m.NOISE_SEED[0], m.NOISE_SEED[1], env.size, ed.data_ptr(), cd.data_ptr(),
                                         z0.data_ptr(), z1.data_ptr(), None))
        torch.cuda.synchronize()
        return z0.cpu().numpy().view(F32), z1.cpu().numpy().view(F32)

    def sweep(self, pair, ranges):
        """gxm_sweep over the inclusive ranges of bit patterns, one report -> (mismatches, lowest patterns, seconds)"""
        torch, n = self.torch, self.n
        rep = np.zeros(C.sizeof(n.GxmSweepReport) // 4, U32)
        rep[2:2 + n.GXM_REPORT_LOWEST] = 0xFFFFFFFF
        rd = self._dev(rep)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for lo, hi in ranges:
            n.check(self.lib.gxm_sweep(pair, lo, hi - lo + 1, rd.data_ptr(), None))
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        out = n.GxmSweepReport.from_buffer_copy(rd.cpu().numpy().tobytes())
        count = int(out.mismatches)
        return count, [int(v) for v in out.lowest][:min(count, n.GXM_REPORT_LOWEST)], dt


@pytest.fixture(scope="module")
def probe(torch_cuda):
    return Probe(torch_cuda)


def device_fns(probe, sets, sincos_fn=None):
    n = probe.n
    return dict(sincos=lambda v: probe.cached(("sincos", sincos_fn, v.size), n.GXM_FN_SINCOS if sincos_fn is None else sincos_fn, v),
                atan2=lambda a, b: probe.cached("atan2", n.GXM_FN_ATAN2, b, a)[0],
                exp=lambda v: probe.cached("exp", n.GXM_FN_EXP, v)[0], log=lambda v: probe.cached("log", n.GXM_FN_LOG, v)[0],
                tanh=lambda v: probe.cached("tanh", n.GXM_FN_TANH, v)[0])


def _finite_angles(sets):
    x = sets["sincos"]
    return x[np.abs(x) <= F32(2.0 ** 24)]            # (drops NaN, +-inf and +-FLT_MAX: kFinite's caller guarantees it)


def assert_same_bits(got, want, what, *inputs):
    """NaN exactly where `want` has NaN, the same bits everywhere else; the message lists the first inputs that differ"""
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert got.shape == want.shape
    bad = np.where(np.isnan(want), ~np.isnan(got), m.f2u(got) != m.f2u(want))
    if bad.any():
        idx = np.flatnonzero(bad)[:8]
        rows = ["  in " + " ".join("%08x (%r)" % (m.f2u(a[i:i + 1])[0], float(a[i])) for a in inputs) +
                " -> %08x (%r), want %08x (%r)" % (m.f2u(got[i:i + 1])[0], float(got[i]), m.f2u(want[i:i + 1])[0], float(want[i]))
                for i in idx]
        pytest.fail("%s: %d of %d differ\n%s" % (what, int(bad.sum()), got.size, "\n".join(rows)))


# ---------------------------------------------------------------------------------------------------------------------
# (a) against float64
# ---------------------------------------------------------------------------------------------------------------------
def _report(tag, measured):
    for k, v in measured.items():
        b = m.BOUNDS[k]
        print("%-22s %-14s %.4g  bound %.2g  of bound %.2f" % (tag, k, v, b, v / b if b else 0.0))


def test_a_device_primitives_within_the_bounds_of_float64(probe, sets):
    measured = m.measures(sets, device_fns(probe, sets))
    _report("HIP", measured)
    assert sorted(measured) == sorted(m.BOUNDS)
    for k, v in measured.items():
        assert v <= m.BOUNDS[k], (k, v, m.BOUNDS[k])


def test_a_sincos_finite_form_within_the_bounds_of_float64(probe, sets):
    sub = dict(sincos=_finite_angles(sets))
    assert sub["sincos"].size == sets["sincos"].size - 5
    fns = device_fns(probe, sets, probe.n.GXM_FN_SINCOS_FINITE)
    measured = m.measures(sub, dict(sincos=fns["sincos"]))
    _report("HIP sincos_f<true>", measured)
    assert sorted(measured) == sorted(k for k in m.BOUNDS if k[:4] in ("sin<", "cos<"))
    for k, v in measured.items():
        assert v <= m.BOUNDS[k], (k, v, m.BOUNDS[k])


def test_a_normal_pair_within_policy64s_bound(probe, sets):
    env, ctr = sets["normal_pair"]
    z0, z1 = probe.normal_pair(env, ctr)
    r0, r1, bound = m.ref_normal_pair(env, ctr)
    e = np.maximum(m.abs_err(z0, r0), m.abs_err(z1, r1))
    pos = bound > 0
    print("HIP normal_pair: worst |z - z64| %.4g, worst of bound %.3f, %d counters (%d with radius 0), largest |z| %.4f"
          % (e.max(), (e[pos] / bound[pos]).max(), e.size, int((~pos).sum()), max(np.abs(z0).max(), np.abs(z1).max())))
    assert (e <= bound).all(), (int((e > bound).sum()), env[e > bound][:4], ctr[e > bound][:4])
    k1, km = len(m.U1_ONE_COUNTERS), len(m.U1_MIN_COUNTERS)
    tail0, tail1 = z0[-(k1 + km):], z1[-(k1 + km):]
    assert (tail0[:k1] == 0).all() and (tail1[:k1] == 0).all()                          # u1 = 1: radius 0, no NaN
    # u1 = 2^-24: the radius sqrt(48 ln 2) = 5.768, to log_f's 1.9e-7 / 2 and sin / cos' 1.2e-7 sqrt(2) and three roundings
    np.testing.assert_allclose(np.hypot(tail0[k1:].astype(np.float64), tail1[k1:]), np.sqrt(48 * np.log(2.0)), rtol=5e-7)


# ---------------------------------------------------------------------------------------------------------------------
# (b) bit for bit against the checker
# ---------------------------------------------------------------------------------------------------------------------
def test_b_device_primitives_equal_the_checker_bit_for_bit(probe, sets, oracle):
    dev, chk = device_fns(probe, sets), m.checker_fns(oracle)
    x = sets["sincos"]
    (s, c), (so, co) = dev["sincos"](x), chk["sincos"](x)
    assert_same_bits(s, so, "sin", x)
    assert_same_bits(c, co, "cos", x)
    y, x = sets["pair"]
    assert_same_bits(dev["atan2"](y, x), chk["atan2"](y, x), "atan2(y, x)", y, x)
    for name in ("exp", "log", "tanh"):
        assert_same_bits(dev[name](sets[name]), chk[name](sets[name]), name, sets[name])


def test_b_sincos_finite_form_equals_the_checker_bit_for_bit(probe, sets, oracle):
    x = _finite_angles(sets)
    s, c = device_fns(probe, sets, probe.n.GXM_FN_SINCOS_FINITE)["sincos"](x)
    so, co = m.checker_fns(oracle)["sincos"](x)
    assert_same_bits(s, so, "sin, kFinite", x)
    assert_same_bits(c, co, "cos, kFinite", x)


# ---------------------------------------------------------------------------------------------------------------------
# (c) bit for bit against the correctly rounded operation
# ---------------------------------------------------------------------------------------------------------------------
def test_c_division_reciprocal_and_sqrt_are_correctly_rounded(probe, sets):
    n = probe.n
    a, b = sets["pair"]
    q = m.exact_div(a, b)
    assert_same_bits(probe.eval(n.GXM_FN_DIV, a, b)[0], q, "a / b", a, b)
    x = sets["rcp"]
    assert_same_bits(probe.eval(n.GXM_FN_RCP, x)[0], m.exact_rcp(x), "1.0f / x", x)
    assert_same_bits(probe.eval(n.GXM_FN_SQRT, x)[0], m.exact_sqrt(x), "sqrtf(x)", x)
    den = lambda v: (v != 0) & (np.abs(v) < m.FLT_MIN)      # noqa: E731
    print("a / b: %d pairs, %d denormal quotients, %d denormal operands; 1 / x and sqrt: %d inputs, %d denormal, %d denormal 1 / x"
          % (a.size, int(den(q).sum()), int((den(a) | den(b)).sum()), x.size, int(den(x).sum()), int(den(m.exact_rcp(x)).sum())))


def test_c_rcp_unscaled_and_div_bin16_on_their_domains(probe, sets):
    n = probe.n
    x = sets["rcp_unscaled"]
    assert_same_bits(probe.eval(n.GXM_FN_RCP_UNSCALED, x)[0], m.exact_rcp(x), "rcp_unscaled(d)", x)
    x = sets["div_bin16"]
    assert_same_bits(probe.eval(n.GXM_FN_DIV_BIN16, x)[0], m.exact_div_bin16(x), "div_bin16(x)", x)


# ---------------------------------------------------------------------------------------------------------------------
# (d) all 2^32 patterns
# ---------------------------------------------------------------------------------------------------------------------
SIGN = 0x80000000


def _both(lo, hi):
    return [(lo, hi), (lo | SIGN, hi | SIGN)]


# pair -> {part: inclusive ranges of bit patterns}; "in": the domain gx_device.h states for the fast form
SWEEPS = {
    # rcp_unscaled: +-0, +-inf, NaN and 2^-126 <= |d| <= 2^126
    "RCP": {"in": _both(0, 0) + _both(0x00800000, 0x7E800000) + _both(0x7F800000, 0x7FFFFFFF),
            "denormal": _both(0x00000001, 0x007FFFFF), "beyond 2^126": _both(0x7E800001, 0x7F7FFFFF)},
    # tanh_f: the same values as the plain form, everywhere
    "TANH": {"in": [(0, 0xFFFFFFFF)]},
    # sincos_f<true>: the caller guarantees |x| <= 2^24
    "SINCOS": {"in": _both(0, 0x4B800000), "beyond 2^24": _both(0x4B800001, 0x7FFFFFFF)},
    # div_bin16: 2^-100 <= |x| <= 2 pi, +0 and NaN
    "DIV_BIN16": {"in": [(0, 0)] + _both(0x0D800000, 0x40C90FDB) + _both(0x7F800001, 0x7FFFFFFF),
                  "below 2^-100": _both(0x00000001, 0x0D7FFFFF), "-0": [(SIGN, SIGN)],
                  "beyond 2 pi": _both(0x40C90FDC, 0x7F800000)},
}
MUST_DIFFER = {("RCP", "denormal"), ("DIV_BIN16", "below 2^-100")}      # gx_device.h: these guards are needed


def test_d_sweep_ranges_are_what_the_header_states():
    assert m.u2f([0x7E800000, 0x4B800000, 0x0D800000, 0x40C90FDB, 0x00800000]).tolist() == \
        [2.0 ** 126, 2.0 ** 24, 2.0 ** -100, float(m.TWO_PI_F), float(m.FLT_MIN)]
    for pair, parts in SWEEPS.items():
        flat = sorted(r for rs in parts.values() for r in rs)
        assert flat[0][0] == 0 and flat[-1][1] == 0xFFFFFFFF, pair
        assert all(lo <= hi for lo, hi in flat) and all(a[1] + 1 == b[0] for a, b in zip(flat, flat[1:])), pair
        assert sum(hi - lo + 1 for lo, hi in flat) == 1 << 32, pair


@pytest.mark.parametrize("pair", list(SWEEPS))
def test_d_fast_forms_equal_their_plain_forms_on_every_pattern(probe, pair):
    pid = getattr(probe.n, "GXM_PAIR_" + pair)
    total = 0
    for part, ranges in SWEEPS[pair].items():
        span = sum(hi - lo + 1 for lo, hi in ranges)
        total += span
        count, lowest, dt = probe.sweep(pid, ranges)
        shown = ", ".join("%08x (%r)" % (b, float(m.u2f([b])[0])) for b in lowest)
        print("sweep %-9s %-12s %10d of %10d patterns differ  (%.1f ms)%s"
              % (pair, part, count, span, 1e3 * dt, "  lowest: " + shown if count else ""))
        assert 0 <= count <= span and len(lowest) == min(count, 16) and lowest == sorted(set(lowest))
        assert all(any(lo <= b <= hi for lo, hi in ranges) for b in lowest)
        if part == "in":
            assert count == 0, "%s: %d in-domain patterns differ from the plain form; the lowest: %s" % (pair, count, shown)
        elif (pair, part) in MUST_DIFFER:
            assert count > 0, "%s, %s: gx_device.h says the fast form fails here, the sweep found no such pattern" % (pair, part)
    assert total == 1 << 32


def test_bad_arguments_are_status_codes(probe, torch_cuda):
    n, lib = probe.n, probe.lib
    buf = torch_cuda.zeros(64, dtype=torch_cuda.int32, device="cuda")
    p, q = buf.data_ptr(), buf.data_ptr() + 4 * 32
    assert lib.gxm_eval(n.GXM_FN_COUNT, 4, p, p, q, q, None) == n.GXM_ERR_ARG and b"unknown fn" in lib.gxm_last_error()
    assert lib.gxm_eval(-1, 4, p, p, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_EXP, -1, p, p, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_EXP, 4, None, p, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_EXP, 4, p, p, None, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_DIV, 4, p, None, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_SINCOS, 4, p, p, q, None, None) == n.GXM_ERR_ARG
    assert lib.gxm_eval(n.GXM_FN_EXP, 0, p, None, q, None, None) == n.GXM_OK
    assert lib.gxm_eval(n.GXM_FN_EXP, 4, p, None, q, None, None) == n.GXM_OK            # d_y, d_out1 unused: may be NULL
    assert lib.gxm_normal_pair(1, 2, -1, p, p, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_normal_pair(1, 2, 4, p, None, q, q, None) == n.GXM_ERR_ARG
    assert lib.gxm_normal_pair(1, 2, 0, p, p, q, q, None) == n.GXM_OK
    assert lib.gxm_sweep(n.GXM_PAIR_COUNT, 0, 4, p, None) == n.GXM_ERR_ARG
    assert lib.gxm_sweep(-1, 0, 4, p, None) == n.GXM_ERR_ARG
    assert lib.gxm_sweep(n.GXM_PAIR_RCP, 0, 4, None, None) == n.GXM_ERR_ARG
    assert lib.gxm_sweep(n.GXM_PAIR_RCP, 1, 1 << 32, p, None) == n.GXM_ERR_ARG and b"2^32" in lib.gxm_last_error()
    assert lib.gxm_sweep(n.GXM_PAIR_RCP, 0, 0, p, None) == n.GXM_OK
    torch_cuda.cuda.synchronize()
    out = buf.cpu().numpy()
    assert out[32:36].view(F32).tolist() == [1.0] * 4                                   # the one call that ran: exp_f(0) = 1
    assert (out[:32] == 0).all() and (out[36:] == 0).all()                              # and nothing else was written
