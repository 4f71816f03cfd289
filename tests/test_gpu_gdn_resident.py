"""csrc/gdn.hip -- the stand-alone (I)GDN kernel with gamma resident in registers: the bits of the CPU oracle and of the
generic kernel's GDN-mode launch (aivc_conv2d with algo = AIVC_ALGO_MFMA) on 64 / 128 channels, partial tiles,
more tiles than workgroups, residual, inverse, operands outside the lean sqrt / division range."""
import ctypes as C

import numpy as np
import pytest
import torch

from aivc_amd import abi
from conv_cases import GDN_RESIDENT_CASES, gdn_resident_case
from numeric_regimes import assert_bits
from op_cases import T, on

pytestmark = pytest.mark.gpu


def _variant(c, n, h, w, inverse, dev):
    from aivc_amd import _lib
    x = torch.zeros((n, h, w, c), device=dev)
    g = torch.zeros((c, c), device=dev)
    b = torch.ones(c, device=dev)
    p = abi.ConvParams(abi.MODE_IGDN if inverse else abi.MODE_GDN, 1, 1, 0, n, h, w, c, h, w, c, 0, 0, abi.ALGO_AUTO, 0, 0,
                       x.data_ptr(), g.data_ptr(), b.data_ptr(), None, None, x.data_ptr(), None, None)
    return _lib.load()['aivc_conv2d_variant'](C.byref(p))


@pytest.mark.parametrize('case', GDN_RESIDENT_CASES)
def test_resident_gdn_bit_exact(case, oracle, cuda):
    from aivc_amd import ops
    c, n, h, w, inv, _ = case
    assert _variant(c, n, h, w, inv, cuda) == 400  # the kernel under test takes the launch
    # (the CPU oracle at the large sizes: the generic kernel stands in, itself pinned here and in test_gpu_ops)
    gc = gdn_resident_case(oracle, case, with_oracle=n * h * w <= 4096)
    d = gc.place(on(cuda))
    got = gc.call(ops, d)
    assert torch.equal(got, gc.call(ops, d, algo=abi.ALGO_MFMA))
    if gc.want is not None:
        gc.check(got)


@pytest.mark.parametrize('inv', [False, True])
@pytest.mark.parametrize('kind', ['zeros', 'tiny', 'huge', 'mixed'])
def test_resident_gdn_outside_the_lean_range(kind, inv, oracle, cuda):
    """operands outside [2^-60, 2^60] (and exact zeros): the wavefront takes the compiler's full IEEE sequences"""
    from aivc_amd import ops
    c, n, h, w = 128, 1, 9, 15
    rng = np.random.default_rng(11)
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    beta = (np.abs(rng.standard_normal(c)) + 0.2).astype(np.float32)
    gamma = (np.abs(rng.standard_normal((c, c))) * 0.05).astype(np.float32)
    if kind == 'zeros':
        x[:, ::2] = 0.0
    elif kind == 'tiny':
        x *= np.float32(2.0 ** -70)
        beta *= np.float32(2.0 ** -100)
    elif kind == 'huge':
        x *= np.float32(2.0 ** 40)
    else:
        x[0, 3, 4, 5] = 0.0
        x[0, 7, 1, 99] = np.float32(2.0 ** 50)
    want = oracle.gdn(x, beta, gamma, inverse=inv)
    got = ops.gdn(T(x, cuda), T(beta, cuda), T(gamma, cuda), inverse=inv)
    assert_bits(got.cpu().numpy(), want)


def test_unsupported_shapes_fall_back(cuda):
    """96 / 192 channels: the generic kernel keeps the launch"""
    assert _variant(96, 1, 9, 9, False, cuda) != 400
    assert _variant(192, 1, 9, 9, False, cuda) != 400
    assert _variant(8, 1, 9, 9, False, cuda) != 400
