"""What tests/test_warp_modes.py (CPU) and tests/test_gpu_warp_modes.py (GPU) share about tests/golden/warp_modes.npz
(tools/gen_golden_warp.py): the list of cases, the fp32 sample position, which pixels the comparisons leave out, and the
measured deviation from which the device's bicubic bound follows.  Not a test module."""
import numpy as np

INTERP = ('bilinear', 'nearest', 'bicubic')
PAD = ('border', 'zeros', 'reflection')
CASES = [(s, m, p, a) for s in (0, 1) for m in INTERP for p in PAD for a in (True, False)]
MASK_THRESHOLD, MASK_BAND, TIE_BAND, MAX_LEFT_OUT = 0.9999, 1e-5, 1e-4, 0.005


def case_key(s, mode, pad, ac):
    return '%d_%s_%s_%d' % (s, mode, pad, int(ac))


def sample_position(flow, h, w, ac):
    """fp32, in the reference's order: grid + flow, * 2 / max(size - 1, 1) - 1, then grid_sample's unnormalisation:
    (g + 1) * ((size - 1) / 2) with align_corners, fma(g + 1, size / 2, -0.5) without (torch's CPU kernel contracts it)."""
    f = np.float32
    out = []
    for ch, size in ((0, w), (1, h)):
        base = np.arange(size, dtype=f).reshape((1, size) if ch == 0 else (size, 1))
        g = (f(2.0) * (base + flow[0, ch].astype(f))) / f(max(size - 1, 1)) - f(1.0)
        if ac:
            out.append((g + f(1.0)) * f((size - 1) / 2.0))
        else:  # ONE rounding (a fused multiply-add): the product and the difference are exact in fp64
            out.append(((g + f(1.0)).astype(np.float64) * (size / 2.0) - 0.5).astype(f))
    assert out[0].dtype == f and out[1].dtype == f
    return out


def left_out(g, s, mode, pad, ac):
    """[1, h, w] bool: pixels no comparison looks at (see the docstring of tests/test_warp_modes.py); asserts the 0.5 % cap"""
    m = g['m_' + case_key(s, mode, pad, ac)]
    out = np.abs(m - np.float32(MASK_THRESHOLD)) < MASK_BAND
    if mode == 'nearest':
        _, _, h, w = g['x_%d' % s].shape
        for p in sample_position(g['flow_%d' % s], h, w, ac):
            d = np.abs(p - np.floor(p) - np.float32(0.5))
            out = out | ((d < TIE_BAND) & (d != 0))[None]
    assert out.mean() <= MAX_LEFT_OUT, out.mean()
    return out


# Largest |reference fp32 y - fp64 restatement| over the 12 bicubic cases of the fixture, measured on the CPU by
# tests/test_warp_modes.py (which re-measures it and fails when this constant is stale): 3.2160e-06, case 0_bicubic_border_0.
BICUBIC_REFERENCE_DEVIATION = 3.216e-6
