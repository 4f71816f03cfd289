"""include/aivc_detmath.h on the device == on the host, function by function and bit for bit (aivc_detmath_eval against its oracle twin).

The header claims that IEEE binary64 add / mul / fma / div and the conversions around them round alike on x86-64 and on gfx950, so
that the codec's sigma, CDF rows and gates are the same bits on both.  Every other HIP == oracle test sees that claim only through
whole kernels on standard-normal inputs: pre-activations within +-5 and log-variances within +-30.  Here each function runs at the
arguments of tests/detmath_cases.py -- the same ones at which tests/test_detmath.py pins the host's accuracy -- which include what
those inputs never reach: fp32 results of exp that are subnormal (x in [-103.97, -87.34]) or overflow, quotients 1.0f / d that are
subnormal (sigmoid below -87.3), the fp64 division of the logarithm at mantissas around sqrt 2 and in the subnormal doubles, every
switch point of the header, NaNs and infinities.  A NaN result is compared as "both NaN".

Then the one device-only shortcut of the entropy model, the windows kernel's wave-uniform saturation test, at its threshold; the sigmoid
epilogues of the conv family beyond +-5 are rows of tests/conv_cases.py (CONV_CASES' last row, ATTENTION_GATE_CASES' last row).

Each test prints how many values it compared."""
import numpy as np
import pytest
import torch

from aivc_amd import abi
import detmath_cases as dc
from op_cases import WINDOW_CHUNK_TMIN, detmath_case, on, saturation_threshold_case

pytestmark = pytest.mark.gpu

SPECIALS64 = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 709.0, -745.0, 709.5, -745.5, -60.0, -60.5, np.finfo(np.float64).max, 5e-324,
                       dc.DBL_MIN, 1.0, 1e-5, 0.34, -0.34], np.float64)
LOG_DOMAIN = np.array([np.finfo(np.float64).max, 5e-324, dc.DBL_MIN, 1.0, 1e-5, 0.34, dc.SQRT2_SWITCH, 0.5, 2.0], np.float64)  # finite x > 0
LOG1P_DOMAIN = np.concatenate([LOG_DOMAIN, [0.0]])


def _run(oracle, cuda, fn, a, b=None):
    from aivc_amd import ops
    case = detmath_case(oracle, fn, a, b)
    case.check(case.run(ops, on(cuda)))
    print('detmath fn %d: %d values compared on the device and on the host, all bit-equal' % (fn, case.n))


@pytest.mark.parametrize('fn', sorted(dc.FP64_NAMES), ids=lambda fn: dc.FP64_NAMES[fn])
def test_fp64_core_device_equals_host(fn, oracle, cuda):
    """the random sets and the dense windows of tests/test_detmath.py, and special values inside each core's domain"""
    special = {abi.DETMATH_EXP: SPECIALS64, abi.DETMATH_EXPM1: SPECIALS64, abi.DETMATH_LOG: LOG_DOMAIN, abi.DETMATH_LOG1P: LOG1P_DOMAIN}[fn]
    _run(oracle, cuda, fn, np.concatenate([x for _, x in dc.fp64_sets(fn)] + [special]))


@pytest.mark.parametrize('fn', sorted(dc.FP32_NAMES), ids=lambda fn: dc.FP32_NAMES[fn])
def test_fp32_wrapper_device_equals_host(fn, oracle, cuda):
    """every 251st bit pattern, 4096 floats on each side of every switch point, the special values"""
    _run(oracle, cuda, fn, np.concatenate([dc.sweep32(), dc.switch_windows(fn), dc.SPECIALS32]))


def test_powf_device_equals_host(oracle, cuda):
    _run(oracle, cuda, abi.DETMATH_POWF, *dc.pow_pairs())


def test_laplace_cdf_device_equals_host(oracle, cuda):
    """the fp32 divisions sigma / sqrt 2 and |t| / b, the saturation at -17.5 and the fp64 expm1 between them"""
    _run(oracle, cuda, abi.DETMATH_LAPLACE_CDF, *dc.laplace_cdf_pairs())


def test_nothing_to_evaluate(cuda):
    """n == 0: no launch, an empty result; two-operand functions ask for b"""
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    for fn in range(abi.DETMATH_COUNT):
        dt = torch.float64 if abi.detmath_is_fp64(fn) else torch.float32
        e = torch.empty(0, dtype=dt, device=cuda)
        assert ops.detmath_eval(fn, e, e if abi.detmath_operands(fn) == 2 else None).numel() == 0
    with pytest.raises(AivcNativeError):
        ops.detmath_eval(abi.DETMATH_POWF, torch.ones(4, device=cuda))
    with pytest.raises(AivcNativeError):
        ops.detmath_eval(abi.DETMATH_COUNT, torch.ones(4, device=cuda))
    torch.cuda.synchronize()


@pytest.mark.parametrize('chunk', sorted(WINDOW_CHUNK_TMIN))
def test_windows_saturation_shortcut_at_its_threshold(chunk, oracle, cuda):
    """laplace_cdf_windows_batch_kernel skips the fp64 work of a wavefront whose lanes all satisfy tmin / b > 17.5f; the oracle
    has no such path.  Sigmas within 4 floats of that threshold for this chunk, laid out so that one wavefront is saturated in every
    lane, one in all but one, one in none, two are mixed and the partial last one is saturated in its 31 valid lanes
    (op_cases.saturation_threshold_case): windows and sigma per position == the oracle's == the slice of its full rows, and a
    stream decoded through those windows (whose slow path rebuilds rows from the same sigmas) gives the coded symbols.
    (Both paths agree at the threshold by construction: this shows the shortcut harmless there, not that its predicate is exact.)"""
    from aivc_amd import ops
    case = saturation_threshold_case(oracle, chunk)
    case.check(case.run(ops, on(cuda)))
