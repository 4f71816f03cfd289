"""warp() in every sampling mode of the reference's signature on the device (aivc_warp_modes, include/aivc_hip_warp.h;
warp_modes_kernel in csrc/pixel_ops.hip) against what the reference itself computed (tests/golden/warp_modes.npz,
tools/gen_golden_warp.py).  The semantics are pinned on the CPU by tests/test_warp_modes.py; both use tests/warp_modes_cases.py.

Tolerances of the comparison with the reference's y:
  bilinear, nearest   rtol = 1e-5, atol = 2e-6: the bound of test_warp in tests/test_gpu_reference_layers.py.
  bicubic             16 taps with weights of both signs.  The reference's own fp32 result deviates from the fp64 restatement
                      of tests/test_warp_modes.py by at most BICUBIC_REFERENCE_DEVIATION (tests/warp_modes_cases.py; measured on the CPU over the 12
                      bicubic cases of the fixture; test_warp_modes.py re-measures it and fails if the constant is stale).
                      Two fp32 evaluations in different orders may each be that far from the truth, times 2 for margin:
                      atol = 4 x that, rtol = 0.
Pixels at the mask's threshold and `nearest` samples next to a tie are left out as tests/test_warp_modes.py's docstring says (<= 0.5 %)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from op_cases import BICUBIC_ATOL, warp_modes_case  # noqa: E402
from warp_modes_cases import CASES, INTERP, PAD, case_key  # noqa: E402

pytestmark = pytest.mark.gpu

assert BICUBIC_ATOL == 4 * 3.216e-6  # (measured: 3.2160e-06, case 0_bicubic_border_0) = 1.2864e-5


@pytest.mark.parametrize('s,mode,pad,ac', CASES, ids=[case_key(*c) for c in CASES])
def test_warp_matches_the_reference_in_every_mode(s, mode, pad, ac, cuda, golden):
    from aivc_amd.func_util.optical_flow import warp
    g = golden('warp_modes')
    c = warp_modes_case(g, s, mode, pad, ac)
    with torch.no_grad():
        y = warp(torch.from_numpy(g['x_%d' % s]).to(cuda), torch.from_numpy(g['flow_%d' % s]).to(cuda), mode, pad, ac)
    assert y.is_cuda and tuple(y.shape) == c.want.shape
    print('%-30s max |y - reference| = %.3e over %d values (%d left out)'
          % (case_key(s, mode, pad, ac), np.abs(y.cpu().numpy() - c.want)[c.keep].max(), c.keep.sum(), (~c.keep).sum()))
    c.check(y)


def test_three_channel_frames_go_through_every_mode(cuda, golden):
    """the module API hands 3-channel frames (MotionCompensation): channels are independent, so the first three channels of
    a 4-channel call and the 3-channel call agree bit for bit"""
    from aivc_amd.func_util.optical_flow import warp
    from aivc_amd.models.motion_compensation import MotionCompensation
    g = golden('warp_modes')
    x, flo = torch.from_numpy(g['x_0']).to(cuda), torch.from_numpy(g['flow_0']).to(cuda)
    for mode, pad, ac in (('nearest', 'zeros', False), ('bicubic', 'reflection', True), ('bilinear', 'zeros', True)):
        assert torch.equal(warp(x[:, :3], flo, mode, pad, ac), warp(x, flo, mode, pad, ac)[:, :3])
    beta = torch.rand(1, 1, 29, 53, device=cuda)
    for mode in INTERP:
        out = MotionCompensation()({'prev': x[:, :3], 'next': x[:, 1:], 'v_prev': flo, 'v_next': -flo, 'beta': beta, 'interpol_mode': mode})
        want = beta * warp(x[:, :3], flo, mode) + (1 - beta) * warp(x[:, 1:], -flo, mode)
        assert torch.equal(out['x_warp'], want)
    # 'bilinear' alone is the fixture's bilinear / border / 1 case
    np.testing.assert_allclose(warp(x, flo, 'bilinear').cpu().numpy(), g['y_0_bilinear_border_1'], rtol=1e-5, atol=2e-6)


def _codec_mode_inputs(i, golden, oracle):
    """the reference-run fixtures warp_0 .. warp_2 (finite flows), or a flow set of tests/op_regimes.py FLOWS on one of its shapes"""
    if isinstance(i, int):
        g = golden('warp_%d' % i)
        return g['x'], g['flow']
    import op_regimes
    d = op_regimes.REGIME_CASES[i](oracle).inputs
    return (np.ascontiguousarray(np.transpose(d[k], (0, 3, 1, 2))) for k in ('x', 'flow'))


@pytest.mark.parametrize('i', list(range(3)) + ['warp-%s-%dx%dx%d' % ((nm,) + sh) for nm in ('nan_x', 'nan_y', 'nan_xy', 'inf', 'big', 'integer')
                                                for sh in ((2, 5, 7), (2, 5, 1), (1, 1, 1))])
def test_codec_mode_is_aivc_warp_bit_for_bit(i, cuda, golden, oracle):
    from aivc_amd import abi, ops
    from aivc_amd._lib import call
    x, flo = _codec_mode_inputs(i, golden, oracle)
    x = ops.to_nhwc(torch.from_numpy(x).to(cuda))
    flo = ops.to_nhwc(torch.from_numpy(flo).to(cuda))
    n, h, w, c = x.shape
    a, b = torch.full_like(x, 7.0), torch.full_like(x, -7.0)
    call('aivc_warp', x.data_ptr(), flo.data_ptr(), n, h, w, c, a.data_ptr(), ops._stream())
    call('aivc_warp_modes', x.data_ptr(), flo.data_ptr(), n, h, w, c, abi.WARP_BILINEAR, abi.WARP_BORDER, 1, b.data_ptr(), ops._stream())
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    assert torch.equal(ops.warp(x, flo), a) and torch.equal(ops.warp(x, flo, 'bilinear', 'border', True), a)


def test_unknown_modes_are_refused(cuda, golden):
    from aivc_amd import _lib, abi, ops
    from aivc_amd.func_util.optical_flow import warp
    g = golden('warp_modes')
    x, flo = torch.from_numpy(g['x_0']).to(cuda), torch.from_numpy(g['flow_0']).to(cuda)
    for kw in (dict(interpol_mode='trilinear'), dict(interpol_mode='Bilinear'), dict(padding_mode='replicate'),
               dict(padding_mode='border '), dict(interpol_mode=None)):
        with pytest.raises(ValueError):
            warp(x, flo, **kw)
    with pytest.raises(ValueError):
        ops.warp(ops.to_nhwc(x), ops.to_nhwc(flo), 'area')
    fn = _lib.load()['aivc_warp_modes']
    xn, fl = ops.to_nhwc(x), ops.to_nhwc(flo)
    out = torch.empty_like(xn)
    n, h, w, c = xn.shape
    args = lambda interp, pad, cc=c: (xn.data_ptr(), fl.data_ptr(), n, h, w, cc, interp, pad, 0, out.data_ptr(), None)
    for interp, pad in ((3, 0), (-1, 0), (0, 3), (0, -1), (2, 7), (99, 99)):
        assert fn(*args(interp, pad)) == -1, (interp, pad)  # AIVC_ERR_ARG
    assert abi.ERRORS[-1] == 'AIVC_ERR_ARG'
    assert fn(*args(abi.WARP_NEAREST, abi.WARP_ZEROS, 3)) == -1  # groups of 4 channels outside the codec's mode
    assert fn(xn.data_ptr() + 4, fl.data_ptr(), n, h, w - 1, c, 1, 1, 0, out.data_ptr(), None) == -1  # 16-byte alignment
    assert fn(None, fl.data_ptr(), n, h, w, c, 1, 1, 0, out.data_ptr(), None) == -1
    assert fn(*args(abi.WARP_NEAREST, abi.WARP_ZEROS)) == 0
    torch.cuda.synchronize()


def test_full_hd_frames_in_every_instantiation(cuda):
    """1920 x 1080 x 4: every kernel instantiation (and both values of align_corners) completes; where modes coincide the
    results do: with samples strictly inside the frame, reflection and zeros never act, so bilinear + reflection and
    bilinear + zeros equal the default path (aivc_warp) up to the rounding of two evaluation orders, and the mask keeps
    every pixel."""
    from aivc_amd import ops
    gen = torch.Generator().manual_seed(5)
    h, w = 1080, 1920
    x = torch.randn(1, h, w, 4, generator=gen).to(cuda)
    flo = (torch.rand(1, h, w, 2, generator=gen) * 6.0 - 3.0)
    cols, rows = torch.arange(w).view(1, 1, w), torch.arange(h).view(1, h, 1)
    flo[..., 0] = torch.minimum(torch.maximum(flo[..., 0], 0.5 - cols), (w - 1.5) - cols)  # samples stay in [0.5, size - 1.5]
    flo[..., 1] = torch.minimum(torch.maximum(flo[..., 1], 0.5 - rows), (h - 1.5) - rows)
    flo = flo.to(cuda)
    base = ops.warp(x, flo)
    outs = {}
    for mode in INTERP:
        for pad in PAD:
            for ac in (True, False):
                y = ops.warp(x, flo, mode, pad, ac)
                assert y.shape == x.shape and bool(torch.isfinite(y).all())
                outs[mode, pad, ac] = y
    torch.cuda.synchronize()
    for pad in ('reflection', 'zeros'):
        # 4 products and 3 sums of terms bounded by max|x| in each of the two evaluations
        assert float((outs['bilinear', pad, True] - base).abs().max()) <= 16 * 2.0 ** -24 * float(x.abs().max())
    for mode in INTERP:  # in-frame samples (bicubic: in-frame away from the edges): the padding mode does not matter
        for ac in (True, False):
            a, b, c = (outs[mode, pad, ac] for pad in PAD)
            inner = (slice(None), slice(8, h - 8), slice(8, w - 8))
            if (mode, ac) != ('bilinear', True):  # (there `border` is aivc_warp, compared above: another evaluation order)
                assert torch.equal(a[inner], b[inner]), (mode, ac)
            # (reflection about -0.5 rounds the position once more, p + 0.5 - 0.5, as grid_sample does: not the same bits)
            if ac or mode == 'bicubic':
                assert torch.equal(b[inner], c[inner]), (mode, ac)
    # nearest returns input values: every output pixel is one of the 4 neighbours of its position
    y = outs['nearest', 'border', True]
    assert bool(torch.isin(y[0, 500, 700], x[0, 495:506, 695:706].reshape(-1, 4)).all())


def test_the_codec_launches_none_of_the_new_kernels(cuda):
    """a default-contract I + P + B encode / decode goes through aivc_warp_blend as before: the launch records of ops
    (PROFILE for the convolutions, PROFILE_HBM for the HBM-bound stages, where warp_modes reports) show no warp_modes"""
    from aivc_amd import ops, synth
    from aivc_amd.models import arch
    model = synth.make_model(arch.TINY_WIDTHS, seed=7, device=cuda)
    frames = synth.synthetic_video(64, 48, 3, seed=3)
    fc = model.frame_codec()
    ops.PROFILE, ops.PROFILE_HBM = [], []
    try:
        with torch.no_grad():
            enc = fc.encode_video(synth.to_device_frames(frames, cuda), '1_GOP_2')  # I, P and B frames
            dec, _, _, _ = fc.decode_video(fc.assemble_video(enc), cuda)
        torch.cuda.synchronize()
        names = [str(rec[0]) for rec in ops.PROFILE] + [rec[0] for rec in ops.PROFILE_HBM]
        assert len(dec) == 3 and len(ops.PROFILE) > 0
        assert 'warp_blend' in names
        assert not any('warp_modes' in nm for nm in names)
        ops.warp(torch.zeros(1, 8, 8, 4, device=cuda), torch.zeros(1, 8, 8, 2, device=cuda), 'nearest')  # (the record does see one)
        assert ops.PROFILE_HBM[-1][0] == 'warp_modes'
    finally:
        ops.PROFILE, ops.PROFILE_HBM = None, None
