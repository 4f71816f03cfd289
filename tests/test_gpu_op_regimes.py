"""The pixel, latent, entropy and rate kernels (csrc/pixel_ops.hip, latent.hip, entropy.hip, rate.hip) against the CPU oracle by
bits on the regimes of tests/op_regimes.py: NaN, infinite and overflowing flows, axes of size 1, non-finite and subnormal pixels
and latents, rounding ties, the clamp constants' neighbours, and every kind of sigma -- the edge of hyper_params' range, what the
API accepts beyond it, and what lies outside the domain of a cdf.  One test id is one builder under one regime.  The oracle itself
is pinned on the same cases by tests/test_op_regimes.py (CPU); tests/test_gpu_memory_discipline.py runs them once more with every
buffer an arena.

aivc_warp_modes in all 18 modes is held to tests/golden/warp_nonfinite.npz, the reference's own answer to the same flow sets,
with the tolerances and the mask rule of tests/test_gpu_warp_modes.py."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import op_regimes as R  # noqa: E402
from op_cases import on, warp_modes_case  # noqa: E402
from warp_modes_cases import CASES, case_key  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case_id', sorted(R.REGIME_CASES))
def test_device_equals_the_oracle_by_bits(case_id, oracle, cuda):
    from aivc_amd import ops
    case = R.REGIME_CASES[case_id](oracle)
    case.check(case.run(ops, on(cuda)))


NONFINITE_CASES = [c for c in CASES if c[0] == 0]


@pytest.mark.parametrize('s,mode,pad,ac', NONFINITE_CASES, ids=[case_key(*c) for c in NONFINITE_CASES])
def test_warp_modes_match_the_reference_on_nonfinite_flows(s, mode, pad, ac, cuda, golden):
    from aivc_amd import ops
    with np.errstate(over='ignore', invalid='ignore'):  # (the position of a non-finite flow, where left_out looks for ties)
        case = warp_modes_case(golden('warp_nonfinite'), s, mode, pad, ac)
    case.check(case.run(ops, on(cuda)))
