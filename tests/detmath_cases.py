"""The arguments at which include/aivc_detmath.h is pinned, each set stated once: tests/test_detmath.py evaluates the header on the
host (oracle.detmath_eval) against 80-bit libm there, tests/test_gpu_detmath.py evaluates it on the device (ops.detmath_eval)
against the host at the same arguments.  Not a test module.

  fp64 cores     seeded random sets over each function's domain and windows of 4096 consecutive doubles around every constant at
                 which the arithmetic changes path (range tests, the series switches, the mantissa switch of the logarithm)
  fp32 wrappers  the strided sweep of ALL bit patterns (every 251st: 17.1 M floats of every binade and both signs, NaNs and
                 infinities included), windows of 4096 consecutive floats on each side of every switch point, and literal
                 special values
  pow            seeded (a, e) pairs, the literal exponents 0 and 1, the base 0
  laplace_cdf    (device == host only) t = k - 256.5 over a strided sweep of the codec's sigma range, and seeded (t, sigma) pairs"""
import numpy as np

from aivc_amd import abi

SEED = 1
N_RANDOM = 2_000_000
SWEEP_STRIDE = 251

FP64_NAMES = {abi.DETMATH_EXP: 'exp', abi.DETMATH_EXPM1: 'expm1', abi.DETMATH_LOG: 'log', abi.DETMATH_LOG1P: 'log1p'}
FP32_NAMES = {abi.DETMATH_EXPF: 'expf', abi.DETMATH_EXPM1F: 'expm1f', abi.DETMATH_SIGMOIDF: 'sigmoidf', abi.DETMATH_TANHF: 'tanhf',
              abi.DETMATH_SOFTPLUSF: 'softplusf'}

DBL_MIN = 2.2250738585072014e-308  # the smallest normal double
SQRT2_SWITCH = 1.4142135623730951  # aivc_det_log halves mantissas above this


def window64(centre, half=2048):
    """2 * half consecutive doubles around centre (by bit pattern: the neighbours on both sides)"""
    b = np.array([centre], np.float64).view(np.int64)[0]
    return (b + np.arange(-half, half, dtype=np.int64)).view(np.float64)


def window32(centre, half=4096):
    """half consecutive floats on each side of fp32(centre), centre included"""
    b = np.array([centre], np.float32).view(np.int32)[0]
    return (b + np.arange(-half, half + 1, dtype=np.int32)).view(np.float32)


def fp64_sets(fn):
    """-> [(name, float64 array)]: the random sets and the dense windows of one fp64 core"""
    rng = np.random.default_rng(SEED + fn)
    n = N_RANDOM
    if fn == abi.DETMATH_EXP:
        return [('uniform[-745,709]', rng.uniform(-745.0, 709.0, n)), ('uniform[-40,40]', rng.uniform(-40.0, 40.0, n)),
                ('window 709', window64(709.0)), ('window -745', window64(-745.0))]
    if fn == abi.DETMATH_EXPM1:
        return [('uniform[-0.34,0.34]', rng.uniform(-0.34, 0.34, n)), ('uniform[-60,40]', rng.uniform(-60.0, 40.0, n)),
                ('normal(0,1e-6)', rng.normal(0.0, 1e-6, n)),
                ('window 0.34', window64(0.34)), ('window -0.34', window64(-0.34)), ('window -60', window64(-60.0))]
    if fn == abi.DETMATH_LOG:
        return [('log-uniform[e^-740,e^709]', np.exp(rng.uniform(-740.0, 709.0, n))), ('uniform[0.5,2]', rng.uniform(0.5, 2.0, n)),
                ('window sqrt2', window64(SQRT2_SWITCH)), ('window DBL_MIN', window64(DBL_MIN))]
    assert fn == abi.DETMATH_LOG1P
    return [('log-uniform[e^-40,e^40]', np.exp(rng.uniform(-40.0, 40.0, n))), ('window 1e-5', window64(1e-5))]


def sweep32():
    """every SWEEP_STRIDE-th bit pattern of a float: 17 111 424 values"""
    return np.arange(0, 2 ** 32, SWEEP_STRIDE, dtype=np.uint64).astype(np.uint32).view(np.float32)


LN_1E5 = -11.512925464970229  # ln(1e-5): below it softplus's exp(x) takes the series branch of aivc_det_log1p
EXPF_OVERFLOW, EXPF_SUBNORMAL, EXPF_UNDERFLOW = 88.72284, -87.33655, -103.97208  # fp32 exp: inf above / subnormal below / 0 below

EXPM1F_LEAVES_MINUS_1 = -17.328679513998633  # ln 2^-25: above it rn32(expm1 x) is no longer -1 (the header saturates below -17.5)

# the points at which a wrapper (or the core under it, seen through the wrapper) changes path
SWITCH_POINTS = {
    abi.DETMATH_EXPM1F: [0.34, -0.34, -17.5, EXPM1F_LEAVES_MINUS_1],
    abi.DETMATH_TANHF: [0.17, -0.17, 20.0, -20.0],
    abi.DETMATH_SOFTPLUSF: [20.0, LN_1E5],
    abi.DETMATH_EXPF: [EXPF_OVERFLOW, EXPF_SUBNORMAL, EXPF_UNDERFLOW],
    abi.DETMATH_SIGMOIDF: [-EXPF_OVERFLOW, -EXPF_SUBNORMAL, -EXPF_UNDERFLOW],
}


def switch_windows(fn):
    return np.concatenate([window32(c) for c in SWITCH_POINTS[fn]])


FLT_MAX = np.float32(3.4028235e38)
FLT_TRUE_MIN = np.float32(1e-45)
SPECIALS32 = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, FLT_MAX, -FLT_MAX, FLT_TRUE_MIN, -FLT_TRUE_MIN], np.float32)


def pow_pairs():
    """-> (a, e) float32: N_RANDOM pairs with a log-uniform over [e^-10, e^10] and e uniform over [-2, 3], the same bases with the
    exponents 0 and 1 (the first 1000 of them), and the base 0 with exponents in [0, 3] (0 itself included)"""
    rng = np.random.default_rng(SEED + abi.DETMATH_POWF)
    a = np.exp(rng.uniform(-10.0, 10.0, N_RANDOM)).astype(np.float32)
    e = rng.uniform(-2.0, 3.0, N_RANDOM).astype(np.float32)
    k = 1000
    e0 = np.concatenate([[0.0], rng.uniform(0.0, 3.0, k - 1)]).astype(np.float32)
    return (np.concatenate([a, a[:k], a[:k], np.zeros(k, np.float32)]),
            np.concatenate([e, np.zeros(k, np.float32), np.ones(k, np.float32), e0]))


SIGMA_LO, SIGMA_HI, SIGMA_STRIDE = 1e-4, 148.41316, 4099  # the codec's sigma range (exp(lv / 2) clamped)


def sigma_sweep(stride=SIGMA_STRIDE):
    """every stride-th float of the codec's sigma range: 41 997 of them at the default stride"""
    lo, hi = (np.array([v], np.float32).view(np.int32)[0] for v in (SIGMA_LO, SIGMA_HI))
    return np.arange(lo, hi + 1, stride, dtype=np.int32).view(np.float32)


def laplace_cdf_pairs():
    """-> (t, sigma): t = k - 256.5 for k = 0..513 at every 64th sigma of the sweep (657 sigmas, the low end of the range included)
    and at its last sigma, then N_RANDOM pairs with t uniform over [-300, 300] and sigma log-uniform over the range, then t = 0"""
    rng = np.random.default_rng(SEED + abi.DETMATH_LAPLACE_CDF)
    sig = np.concatenate([sigma_sweep()[::64], sigma_sweep()[-1:]])
    t = (np.arange(abi.LP, dtype=np.float32) - np.float32(256.5))
    tr = rng.uniform(-300.0, 300.0, N_RANDOM).astype(np.float32)
    sr = np.exp(rng.uniform(np.log(SIGMA_LO), np.log(SIGMA_HI), N_RANDOM)).astype(np.float32)
    return (np.concatenate([np.tile(t, sig.size), tr, np.zeros(8, np.float32)]), np.concatenate([np.repeat(sig, abi.LP), sr, sr[:8]]))


def sample(fn, n, seed):
    """n arguments of function fn inside its domain (a, b or None): what the guarded runs of tests/test_gpu_memory_discipline.py use"""
    rng = np.random.default_rng(seed)
    if fn == abi.DETMATH_EXP:
        return rng.uniform(-745.0, 709.0, n), None
    if fn == abi.DETMATH_EXPM1:
        return rng.uniform(-60.0, 40.0, n), None
    if fn == abi.DETMATH_LOG:
        return np.exp(rng.uniform(-740.0, 709.0, n)), None
    if fn == abi.DETMATH_LOG1P:
        return np.exp(rng.uniform(-40.0, 40.0, n)), None
    if fn == abi.DETMATH_POWF:
        return np.exp(rng.uniform(-10.0, 10.0, n)).astype(np.float32), rng.uniform(-2.0, 3.0, n).astype(np.float32)
    if fn == abi.DETMATH_LAPLACE_CDF:
        return (rng.uniform(-300.0, 300.0, n).astype(np.float32),
                np.exp(rng.uniform(np.log(SIGMA_LO), np.log(SIGMA_HI), n)).astype(np.float32))
    return rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32), None  # any bit pattern


def same_bits(got, want):
    """elementwise: the same bit pattern, or both NaN (payload and sign of a NaN are not part of the contract)"""
    assert got.dtype == want.dtype and got.shape == want.shape
    u = np.uint64 if got.dtype == np.float64 else np.uint32
    return (got.view(u) == want.view(u)) | (np.isnan(got) & np.isnan(want))
