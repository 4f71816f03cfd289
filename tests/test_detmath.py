"""Accuracy of include/aivc_detmath.h on the host (through oracle.detmath_eval), independently of every HIP == oracle test: those
include the same header on both sides, so a wrong coefficient, switch point or saturation constant changes both alike.

Reference: numpy longdouble = x87 80-bit (64-bit significand), whose exp / expm1 / log / log1p / tanh / power are glibc's 80-bit
libm, 2^11 times finer than an fp64 ulp.  test_reference_libm_against_mpmath validates that reference itself against mpmath at 60
digits; every other test here trusts it.

  fp64 cores     error in fp64 ulps of the true value over the sets of tests/detmath_cases.py: exp <= 2 (the header's claim),
                 expm1 / log / log1p <= 4.
  fp32 wrappers  bit equality with the correctly rounded value in the header's stated op order.  The cores are a few fp64 ulps
                 off, so (float)core(x) differs from the correctly rounded fp32 only where the true value lies within those few
                 ulps of a rounding midpoint: probability ~ 8 ulp64 * 2 / 2^29 ulp64 per point, ~0.25 expected in the 17.1 M sweep.
                 A mismatch is tolerated only if the header's value is the float on the OTHER side of a midpoint that the 80-bit value
                 is within 8 ulp64 of, and at most 4 times per function.
  torch          |det - torch| <= 1 ulp32 for exp / expm1 / tanh / softplus (det is correctly rounded, torch / SLEEF within 1 ulp).
  Laplace rows   every symbol of every row codable, no row longer than one turn of the 16-bit range."""
import numpy as np
import pytest

from aivc_amd import abi
import detmath_cases as dc

LD = np.longdouble
pytestmark = pytest.mark.skipif(np.finfo(LD).nmant != 63, reason='the reference needs an 80-bit long double (x87); numpy longdouble '
                                                                 'has %d mantissa bits here' % np.finfo(LD).nmant)
CHUNK = 1 << 21
NEAR_TIE_ULP64 = 8
MAX_NEAR_TIES = 4


def test_longdouble_is_80_bit():
    assert np.finfo(LD).nmant == 63


# ---- the reference itself ------------------------------------------------------------------------------------------------------
def test_reference_libm_against_mpmath():
    """~2000 points per function: glibc's 80-bit functions within 4 ulp80 = 2^-9 ulp64 of mpmath's 60-digit values (what the
    ulp64 bounds and the 8 ulp64 near-tie window below need of the reference: an error far below one fp64 ulp)"""
    mpmath = pytest.importorskip('mpmath')
    mpmath.mp.dps = 60

    def mp(v):  # an 80-bit value as an exact mpf: its 64-bit significand as two doubles, then the exponent (beyond fp64's range too)
        m, e = np.frexp(v)
        hi = np.float64(m)
        return mpmath.ldexp(mpmath.mpf(float(hi)) + mpmath.mpf(float(np.float64(m - LD(hi)))), int(e))
    rng = np.random.default_rng(dc.SEED)
    n = 2000
    cases = [('exp', np.exp, mpmath.exp, rng.uniform(-745, 709, n)), ('expm1', np.expm1, mpmath.expm1, np.concatenate([rng.uniform(-60, 40, n // 2), rng.normal(0, 0.2, n // 2)])),
             ('log', np.log, mpmath.log, np.exp(rng.uniform(-740, 709, n))), ('log1p', np.log1p, mpmath.log1p, np.exp(rng.uniform(-40, 40, n))),
             ('tanh', np.tanh, mpmath.tanh, rng.uniform(-20, 20, n))]
    for name, f_ld, f_mp, xs in cases:
        got = f_ld(xs.astype(LD))
        worst = max(abs((mp(g) - f_mp(mpmath.mpf(float(x)))) / f_mp(mpmath.mpf(float(x)))) for g, x in zip(got, xs))
        print('%s: 80-bit libm within %.3g ulp80 of mpmath over %d points' % (name, float(worst * 2 ** 63), n))
        assert worst <= mpmath.mpf(2) ** -61, name
    a, e = np.exp(rng.uniform(-10, 10, n)).astype(np.float32), rng.uniform(-2, 3, n).astype(np.float32)
    got = np.power(a.astype(LD), e.astype(LD))
    worst = max(abs((mp(g) - mpmath.power(float(x), float(y))) / mpmath.power(float(x), float(y))) for g, x, y in zip(got, a, e))
    print('power: within %.3g ulp80' % float(worst * 2 ** 63))
    assert worst <= mpmath.mpf(2) ** -61


# ---- fp64 cores ----------------------------------------------------------------------------------------------------------------
def ulp64_of(v):
    """the fp64 ulp at the magnitude of the 80-bit values v (2^-1074 in the subnormal range)"""
    _, e = np.frexp(v)
    return np.ldexp(LD(1), np.maximum(e.astype(np.int64) - 53, -1074).astype(np.int32))


def ulp64_error(got, ref):
    return np.abs(got.astype(LD) - ref) / ulp64_of(ref)


REF64 = {abi.DETMATH_EXP: np.exp, abi.DETMATH_EXPM1: np.expm1, abi.DETMATH_LOG: np.log, abi.DETMATH_LOG1P: np.log1p}
BOUND64 = {abi.DETMATH_EXP: 2.0, abi.DETMATH_EXPM1: 4.0, abi.DETMATH_LOG: 4.0, abi.DETMATH_LOG1P: 4.0}


@pytest.mark.parametrize('fn', sorted(REF64), ids=lambda fn: dc.FP64_NAMES[fn])
def test_fp64_core_ulps(fn, oracle):
    """Measured over these sets (gcc -O2 -ffp-contract=off): exp 0.86, expm1 3.1, log 2.8, log1p 3.2 ulp64, as the header states.
    exp saturates by its documented range tests, not by the value: +inf for every x > 709 (the true value overflows only above
    709.78) and 0 for x < -745 (the true value rounds to 2^-1074 down to -745.13, an error of 0.57 ulp at most).  The window around
    709 pins the first literally and measures the rest."""
    worst = {}
    for name, x in dc.fp64_sets(fn):
        got = oracle.detmath_eval(fn, x)
        if fn == abi.DETMATH_EXP:
            sat = x > 709.0
            assert np.all(np.isposinf(got[sat])), name
            assert np.all(got[x < -745.0] == 0.0), name
            x, got = x[~sat], got[~sat]
        assert np.all(np.isfinite(got)), name
        err = np.concatenate([ulp64_error(got[i:i + CHUNK], REF64[fn](x[i:i + CHUNK].astype(LD))) for i in range(0, x.size, CHUNK)])
        i = int(np.argmax(err))
        worst[name] = float(err[i])
        print('%s %s: %d points, max %.3f ulp64 at x = %r' % (dc.FP64_NAMES[fn], name, x.size, err[i], float(x[i])))
    assert max(worst.values()) <= BOUND64[fn], worst


def test_fp64_core_special_values(oracle):
    inf, nan = np.inf, np.nan
    ev = lambda fn, *xs: oracle.detmath_eval(fn, np.array(xs, np.float64))
    got = ev(abi.DETMATH_EXP, 0.0, -0.0, inf, -inf, 709.5, -745.5)
    assert got.tolist() == [1.0, 1.0, inf, 0.0, inf, 0.0] and not np.signbit(got[3])
    got = ev(abi.DETMATH_EXPM1, 0.0, -0.0, inf, -inf, -60.5)
    assert got.tolist() == [0.0, 0.0, inf, -1.0, -1.0] and np.signbit(got).tolist() == [False, True, False, True, True]
    assert ev(abi.DETMATH_LOG, 1.0).tolist() == [0.0] and ev(abi.DETMATH_LOG1P, 0.0).tolist() == [0.0]
    assert np.isnan(ev(abi.DETMATH_EXP, nan)).all() and np.isnan(ev(abi.DETMATH_EXPM1, nan)).all()
    # +- the largest finite argument of each core (log: both ends of the finite positive doubles)
    dmax, dtrue_min = np.finfo(np.float64).max, 5e-324
    for fn, xs in ((abi.DETMATH_EXP, [709.0, -745.0]), (abi.DETMATH_EXPM1, [709.0, -60.0]), (abi.DETMATH_LOG, [dmax, dtrue_min]),
                   (abi.DETMATH_LOG1P, [dmax])):
        x = np.array(xs, np.float64)
        err = ulp64_error(oracle.detmath_eval(fn, x), REF64[fn](x.astype(LD)))
        assert np.all(err <= BOUND64[fn]), (dc.FP64_NAMES[fn], xs, err)


# ---- fp32 wrappers -------------------------------------------------------------------------------------------------------------
def _ld(x):
    return x.astype(LD)


def _softplus_value(x):
    return np.log1p(np.exp(_ld(x)))


# fn -> (the 80-bit value that the header rounds once to fp32, what follows that rounding in fp32)
_ONE = np.float32(1)
WRAPPERS = {
    abi.DETMATH_EXPF: (lambda x: np.exp(_ld(x)), lambda x, r: r),
    abi.DETMATH_EXPM1F: (lambda x: np.expm1(_ld(x)), lambda x, r: r),
    abi.DETMATH_TANHF: (lambda x: np.tanh(_ld(x)), lambda x, r: r),
    abi.DETMATH_SOFTPLUSF: (_softplus_value, lambda x, r: np.where(x > np.float32(20), x, r)),
    abi.DETMATH_SIGMOIDF: (lambda x: np.exp(_ld(-x)), lambda x, r: _ONE / (_ONE + r)),
}


def _other_side_of_a_near_tie(v):
    """80-bit values v -> (the float on the other side of the fp32 rounding midpoint nearest to v, whether v lies within
    NEAR_TIE_ULP64 fp64 ulps of that midpoint)"""
    with np.errstate(over='ignore'):
        r = v.astype(np.float32)
    other = np.nextafter(r, np.where(_ld(r) < v, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32))
    mid = (_ld(r) + _ld(other)) / 2
    with np.errstate(invalid='ignore'):
        near = np.isfinite(other) & (_ld(r) != v) & (np.abs(v - mid) <= NEAR_TIE_ULP64 * ulp64_of(v))
    return other, near


def check_wrapper(oracle, fn, x, what):
    """oracle.detmath_eval(fn, x) against the op-order expected value, chunk by chunk -> number of tolerated near-ties"""
    value, finish = WRAPPERS[fn]
    got = oracle.detmath_eval(fn, x)
    ties = 0
    for i in range(0, x.size, CHUNK):
        xc, gc = x[i:i + CHUNK], got[i:i + CHUNK]
        with np.errstate(all='ignore'):
            v = value(xc)
            want = finish(xc, v.astype(np.float32)).astype(np.float32)
        bad = np.flatnonzero(~dc.same_bits(gc, want))
        if bad.size:
            with np.errstate(all='ignore'):
                other, near = _other_side_of_a_near_tie(v[bad])
                alt = finish(xc[bad], other).astype(np.float32)
            ok = near & dc.same_bits(gc[bad], alt)
            j = bad[~ok]
            assert j.size == 0, ('%s %s: %d values differ from the correctly rounded one and are no near-tie; first x = %r (bits 0x%08X): '
                                 'got %r, want %r' % (dc.FP32_NAMES[fn], what, j.size, float(xc[j[0]]), int(xc[j[:1]].view(np.uint32)[0]),
                                                      float(gc[j[0]]), float(want[j[0]])))
            ties += int(ok.sum())
    print('%s %s: %d points, %d near-tie(s) rounded to the other side' % (dc.FP32_NAMES[fn], what, x.size, ties))
    assert ties <= MAX_NEAR_TIES
    return ties


@pytest.mark.parametrize('fn', sorted(WRAPPERS), ids=lambda fn: dc.FP32_NAMES[fn])
def test_fp32_wrapper_sweep(fn, oracle):
    """every 251st bit pattern: rn32(exp x), rn32(expm1 x), rn32(tanh x), x > 20 ? x : rn32(log1p(exp x)), and for the sigmoid
    1 / (1 + rn32(exp(-x))) evaluated in fp32.  Measured: 0 mismatches in 17 111 424 points for each of the five."""
    check_wrapper(oracle, fn, dc.sweep32(), 'sweep')


@pytest.mark.parametrize('fn', sorted(WRAPPERS), ids=lambda fn: dc.FP32_NAMES[fn])
def test_fp32_wrapper_switch_points(fn, oracle):
    """4096 consecutive floats on each side of every point at which the wrapper or the core under it changes path, or at which
    the correctly rounded value does (detmath_cases.SWITCH_POINTS).  A window sees a constant of the header only where the value
    changes nearby: aivc_expm1f_det's -17.5f sits where rn32(expm1 x) is -1 on both sides, so the window around it pins the
    saturation but would not notice the constant moved; the window at ln 2^-25 = -17.3287, where the value leaves -1, does."""
    check_wrapper(oracle, fn, dc.switch_windows(fn), 'windows at %s' % dc.SWITCH_POINTS[fn])


def test_powf(oracle):
    """rn32(a^e) from the 80-bit powl; e == 0 -> 1, e == 1 -> a, a == 0 -> 0 (e >= 0 here: the header is stated for a > 0 and
    returns 0 for the base 0 whatever the exponent)"""
    a, e = dc.pow_pairs()
    got = oracle.detmath_eval(abi.DETMATH_POWF, a, e)
    v = np.power(_ld(a), _ld(e))
    want = v.astype(np.float32)
    bad = np.flatnonzero(~dc.same_bits(got, want))
    other, near = _other_side_of_a_near_tie(v[bad])
    ok = near & dc.same_bits(got[bad], other)
    print('powf: %d pairs, %d near-tie(s) rounded to the other side' % (a.size, int(ok.sum())))
    assert ok.all(), (a[bad[~ok]][:4], e[bad[~ok]][:4], got[bad[~ok]][:4], want[bad[~ok]][:4])
    assert ok.sum() <= MAX_NEAR_TIES
    k = 1000
    assert np.all(got[-3 * k:-2 * k] == 1) and np.array_equal(got[-2 * k:-k], a[:k]) and got[-k] == 1 and np.all(got[-k + 1:] == 0)


def test_fp32_special_values(oracle):
    """+-0, +-inf, NaN, +-FLT_MAX, +- the smallest subnormal against a literal table.
    aivc_tanhf_det(-0.0f) is +0.0f (its sign test `x < 0` is false for -0), where torch.tanh gives -0.0: pinned as it is."""
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    mx, tiny = dc.FLT_MAX, dc.FLT_TRUE_MIN
    ln2 = np.float32(0.6931472)
    assert dc.SPECIALS32.view(np.uint32).tolist() == [0, 0x80000000, 0x7F800000, 0xFF800000, 0x7FC00000, 0x7F7FFFFF, 0xFF7FFFFF, 1, 0x80000001]
    #          +0    -0     +inf  -inf   NaN   FLT_MAX  -FLT_MAX  tiny   -tiny
    table = {
        abi.DETMATH_EXPF: [1, 1, inf, 0, nan, inf, 0, 1, 1],
        abi.DETMATH_EXPM1F: [0, -0.0, inf, -1, nan, inf, -1, tiny, -tiny],
        abi.DETMATH_TANHF: [0, 0, 1, -1, nan, 1, -1, tiny, -tiny],
        abi.DETMATH_SOFTPLUSF: [ln2, ln2, inf, 0, nan, mx, 0, ln2, ln2],
        abi.DETMATH_SIGMOIDF: [0.5, 0.5, 1, 0, nan, 1, 0, 0.5, 0.5],
    }
    for fn, want in table.items():
        got = oracle.detmath_eval(fn, dc.SPECIALS32)
        want = np.array(want, np.float32)
        assert dc.same_bits(got, want).all(), (dc.FP32_NAMES[fn], got, want)
    assert not np.signbit(oracle.detmath_eval(abi.DETMATH_TANHF, np.array([-0.0], np.float32)))[0]


def test_rate_of_prob_passes_nan_through(oracle):
    """aivc_det_log is stated for finite x > 0 only; aivc_rate_of_prob keeps a NaN probability away from it (torch.clamp and
    -log2 pass a NaN through as well)"""
    p = np.array([0.25, np.nan, 1.0, 0.0], np.float32)
    rate, _ = oracle.rate_bits(p, 2.0 ** -16, 1.0)
    assert np.isnan(rate[1]) and rate[[0, 2, 3]].tolist() == [2.0, 0.0, 16.0]


# ---- torch ---------------------------------------------------------------------------------------------------------------------
def _ordered(f):
    """float32 -> int64 that counts representable values (-0 and +0 both 0)"""
    b = f.view(np.int32).astype(np.int64)
    return np.where(b < 0, -(b & 0x7FFFFFFF), b)


@pytest.mark.parametrize('fn', [abi.DETMATH_EXPF, abi.DETMATH_EXPM1F, abi.DETMATH_TANHF, abi.DETMATH_SOFTPLUSF], ids=lambda fn: dc.FP32_NAMES[fn])
def test_within_one_ulp_of_torch(fn, oracle):
    """The same sweep through CPU torch.exp / expm1 / tanh / F.softplus: det is the correctly rounded value and torch (SLEEF) is
    within 1 ulp of the truth, so they are at most 1 ulp32 apart (measured maximum: 1 for all four).
    torch.sigmoid is NOT asserted: it evaluates another formula and was measured up to 4 ulp32 away from
    1 / (1 + rn32(exp(-x))), worst near x = -16.7; the op-order value of test_fp32_wrapper_sweep is the statement for sigmoid."""
    import torch
    x = dc.sweep32()
    f = {abi.DETMATH_EXPF: torch.exp, abi.DETMATH_EXPM1F: torch.expm1, abi.DETMATH_TANHF: torch.tanh,
         abi.DETMATH_SOFTPLUSF: torch.nn.functional.softplus}[fn]
    want = f(torch.from_numpy(x)).numpy()
    got = oracle.detmath_eval(fn, x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan)
    d = np.abs(_ordered(got[~nan]) - _ordered(want[~nan]))
    print('%s against torch: %d points, max %d ulp32, %d differ' % (dc.FP32_NAMES[fn], x.size, d.max(), np.count_nonzero(d)))
    assert d.max() <= 1


# ---- Laplace rows --------------------------------------------------------------------------------------------------------------
def test_laplace_rows_are_codable_over_the_sigma_range(oracle):
    """every 4099th float of [1e-4, 148.41316]: each of the 513 symbols of a row has a step of at least 1 (mod 2^16: the rows wrap
    by design), and row[0] plus the steps stays within one turn, which rint(cdf * 65023) + k <= 65023 + 513 = 65536 guarantees"""
    sig = dc.sigma_sweep()
    assert sig.size == 41997 and sig[0] == np.float32(1e-4) and sig[-1] <= np.float32(148.41316)
    rows = oracle.laplace_cdf_rows(sig.reshape(1, 1, -1, 1), [0])[:, :abi.LP].astype(np.int64)
    steps = (rows[:, 1:] - rows[:, :-1]) % 65536
    assert steps.shape == (sig.size, 513)
    assert steps.min() >= 1
    assert (rows[:, 0] + steps.sum(axis=1)).max() <= 65536


# ---- the bits themselves -------------------------------------------------------------------------------------------------------
def _u01(n, salt):
    """n doubles in [0, 1) from splitmix64 of a counter: integer arithmetic only, the same on every machine and numpy release"""
    z = (np.arange(1, n + 1, dtype=np.uint64) + np.uint64(salt)) * np.uint64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    z = z ^ (z >> np.uint64(31))
    return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53, z


def _pinned_inputs(fn):
    n = 1 << 20
    u, z = _u01(n, fn)
    f32 = lambda a: a.astype(np.float32)
    if fn == abi.DETMATH_EXP:
        return (np.concatenate([u * 1454.0 - 745.0, dc.window64(709.0), dc.window64(-745.0)]),)
    if fn == abi.DETMATH_EXPM1:
        return (np.concatenate([u * 2.0 - 1.0, u * 100.0 - 60.0, dc.window64(0.34), dc.window64(-0.34), dc.window64(-60.0)]),)
    if fn == abi.DETMATH_LOG:  # every exponent of the positive doubles, subnormals included
        return (np.concatenate([(z % np.uint64(0x7FF0000000000000 - 1) + np.uint64(1)).view(np.float64), u * 1.5 + 0.5,
                                dc.window64(dc.SQRT2_SWITCH), dc.window64(dc.DBL_MIN)]),)
    if fn == abi.DETMATH_LOG1P:
        return (np.concatenate([u * 1e-4, u * 100.0, dc.window64(1e-5)]),)
    if fn == abi.DETMATH_POWF:
        return f32(u * 1000.0 + 1e-3), f32(_u01(n, 77)[0] * 5.0 - 2.0)
    if fn == abi.DETMATH_LAPLACE_CDF:
        sig = dc.sigma_sweep()[::64]
        return np.tile(np.arange(abi.LP, dtype=np.float32) - np.float32(256.5), sig.size), np.repeat(sig, abi.LP)
    return (np.concatenate([dc.switch_windows(fn), dc.SPECIALS32, f32(u * 240.0 - 120.0), dc.sweep32()[::257]]),)


PINNED = {
    abi.DETMATH_EXP: 'bdc09b6292603dcc0cbe623354d7e9c3', abi.DETMATH_EXPM1: '85b57f4171ea2b5ed771b5dd515ea7b9',
    abi.DETMATH_LOG: '28df1149a97d18af865d46c34cd06e39', abi.DETMATH_LOG1P: 'adce9f5a401ce28725f515eb030cea3c',
    abi.DETMATH_EXPF: '531a66edafadd93623be64eabe9e1dcb', abi.DETMATH_EXPM1F: '4b19bfb10542f955731e9bfeb048666c',
    abi.DETMATH_SIGMOIDF: '956b0e1e36827943e4bff8bd716fb917', abi.DETMATH_TANHF: '3013f5dcd3f7326a4328e0856d08a023',
    abi.DETMATH_SOFTPLUSF: '4608dd8b351c34f7de345018f1d0638d', abi.DETMATH_POWF: '22e67f751cf3faa8088e645d4b7dadcc',
    abi.DETMATH_LAPLACE_CDF: 'c60a8a9385b67c5f974a595ed1d5fe2f',
}


@pytest.mark.parametrize('fn', range(abi.DETMATH_COUNT))
def test_contract_bits_are_pinned(fn, oracle):
    """The header is a bit contract between an encoder and a decoder, not only an approximation: the series switch of
    aivc_det_expm1 moved from 0.34 to 0.5 keeps every accuracy bound above (the series is as accurate there) and still makes one
    build's streams unreadable by another.  SHA-256 of each function's results over machine-independent arguments (a counter hash, the switch windows, the
    special values), recorded from the header as it stands at ABI 22.  A digest changes only with a deliberate change of the
    contract, which also has to bump the stream's version; record the new value then.  (NaN results are canonicalised.)"""
    import hashlib
    got = oracle.detmath_eval(fn, *_pinned_inputs(fn)).copy()
    got[np.isnan(got)] = np.nan
    digest = hashlib.sha256(got.tobytes()).hexdigest()[:32]
    print('fn %d: %d results, sha256[:32] %s' % (fn, got.size, digest))
    assert digest == PINNED[fn]
