"""CPU tier: the 18 sampling modes of warp() (interpol_mode x padding_mode x align_corners, src/func_util/optical_flow.py:14-55)
pinned by a numpy restatement against what the reference itself computed (tests/golden/warp_modes.npz, tools/gen_golden_warp.py).

The restatement is this file's own (it is not the CPU oracle).  The sample POSITION is evaluated in fp32 in the reference's
order of operations -- it is part of the semantics: which neighbour `nearest` picks and which pixels the mask zeroes depend
on its bits; for bilinear and nearest that includes the padding of the coordinate -- and everything after it (weights, the 4 / 16-tap sums, the mask's weight sum) in fp64.

What it pins, beyond grid_sample's modes:
  * the mask: the same weights applied to ones, `< 0.9999` -> the WHOLE pixel is zero (only `zeros` padding ever gets there);
  * align_corners=False is normalised with size - 1 all the same: position ((col + v) * W / (W - 1)) - 0.5, a zoom about the centre.

Pixels left out of every comparison (tests/warp_modes_cases.py; at most 0.5 % of a case, asserted): stored fp32 mask within 1e-5 of 0.9999; `nearest`
samples whose fp32 position is within 1e-4 of a half-integer without being exactly on one (exact ties stay in: half to even).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from warp_modes_cases import (BICUBIC_REFERENCE_DEVIATION, CASES, MASK_THRESHOLD, case_key, left_out,  # noqa: E402
                              sample_position)

CUBIC_A = -0.75


def pad_coordinate(p, size, pad, ac):
    """grid_sample's padding of a coordinate, in p's own precision (fp32 for the bilinear / nearest position, whose bits
    matter; the bicubic tap indices are whole numbers, exact either way).  Reflection has the period 2 * span."""
    t = p.dtype.type
    if pad == 'zeros':
        return p
    if pad == 'reflection':
        lo, twice_span = (t(0.0), t(2 * (size - 1))) if ac else (t(-0.5), t(2 * size))
        if twice_span == 0:
            p = np.zeros_like(p)
        else:
            a = np.abs(p - lo)
            extra = a - np.trunc(a / twice_span) * twice_span
            p = np.minimum(extra, twice_span - extra) + lo
    with np.errstate(invalid='ignore'):  # grid_sample's clip, written as its min / max: a NaN coordinate ends at 0
        p = np.where(p > t(0.0), p, t(0.0))
        return np.where(p < t(size - 1), p, t(size - 1))


def gather(x, iy, ix):
    """x [c, h, w], integer-valued float indices [h, w] -> (values [c, h, w] with 0 outside, inside [h, w] as 0. / 1.)"""
    _, h, w = x.shape
    with np.errstate(invalid='ignore'):
        ok = (iy >= 0) & (iy < h) & (ix >= 0) & (ix < w)  # (false for a NaN index: `zeros` padding leaves a NaN position alone)
    v = x[:, np.where(ok, iy, 0).astype(np.int64), np.where(ok, ix, 0).astype(np.int64)]
    return np.where(ok, v, 0.0), ok.astype(np.float64)  # (a tap outside is skipped, not multiplied by 0: the pixel may be inf)


def cubic_weights(t):
    a = CUBIC_A
    inner = lambda u: ((a + 2.0) * u - (a + 3.0)) * u * u + 1.0
    outer = lambda u: ((a * u - 5.0 * a) * u + 8.0 * a) * u - 4.0 * a
    return [outer(t + 1.0), inner(t), inner(1.0 - t), outer(2.0 - t)]


def warp_fp64(x, flow, mode, pad, ac):
    """x [1, c, h, w], flow [1, 2, h, w] -> (y [1, c, h, w] fp64 after the mask, weight sum of the mask [1, h, w] fp64)"""
    _, c, h, w = x.shape
    x64 = x[0].astype(np.float64)
    px, py = sample_position(flow, h, w, ac)
    if mode != 'bicubic':
        px, py = pad_coordinate(px, w, pad, ac), pad_coordinate(py, h, pad, ac)
        assert px.dtype == np.float32
    px, py = px.astype(np.float64), py.astype(np.float64)
    y = np.zeros((c, h, w))
    m = np.zeros((h, w))
    if mode == 'nearest':
        ix, iy = np.rint(px), np.rint(py)  # half to even
        y, m = gather(x64, iy, ix)
    elif mode == 'bilinear':
        x0, y0 = np.floor(px), np.floor(py)
        tx, ty = px - x0, py - y0
        for dy, wy in ((0, 1.0 - ty), (1, ty)):
            for dx, wx in ((0, 1.0 - tx), (1, tx)):
                v, ok = gather(x64, y0 + dy, x0 + dx)
                y = y + v * (wx * wy)
                m = m + ok * (wx * wy)
    else:  # bicubic: the padding applies to each tap's index, not to the position
        x0, y0 = np.floor(px), np.floor(py)
        wxs, wys = cubic_weights(px - x0), cubic_weights(py - y0)
        for i in range(4):
            iy = pad_coordinate(y0 - 1 + i, h, pad, ac)
            for j in range(4):
                ix = pad_coordinate(x0 - 1 + j, w, pad, ac)
                v, ok = gather(x64, iy, ix)
                y = y + v * (wxs[j] * wys[i])
                m = m + ok * (wxs[j] * wys[i])
    y = y * (m >= MASK_THRESHOLD)
    return y[None], m[None]


def deviation(g, s, mode, pad, ac):
    """-> (largest |reference fp32 y - fp64 restatement| over the compared pixels, largest |stored mask - restated weight sum|)"""
    x, flow = g['x_%d' % s], g['flow_%d' % s]
    y64, m64 = warp_fp64(x, flow, mode, pad, ac)
    keep = ~left_out(g, s, mode, pad, ac)
    key = case_key(s, mode, pad, ac)
    dy = np.abs(g['y_' + key].astype(np.float64) - y64) * keep[:, None]
    dm = np.abs(g['m_' + key].astype(np.float64) - m64) * keep
    return dy.max(), dm.max()


# fp32 rounding of what follows the position, as a multiple of 2^-24 * max|x| (the reference evaluates it in fp32, the
# restatement in fp64):
#   nearest   copies a value: exact.
#   bilinear  1 - t rounds once, each weight product once, 4 products and 3 sums: < 8 roundings of terms whose absolute
#             values sum to <= max|x|.
#   bicubic   each weight is a 3-step Horner form with intermediates up to 2.25 (about 6 roundings: <= 14 * 2^-24 absolute);
#             the |weights| of one direction sum to <= 1.375 (at t = 0.5), so the two directions' weight errors contribute
#             2 * 1.375 * 4 * 14 = 154 units, the 16 products and 19 sums of terms with sum |w_x w_y| <= 1.375^2 another
#             35 * 1.89 = 66: 220, rounded up to 256.
ROUNDINGS = {'nearest': 0, 'bilinear': 8, 'bicubic': 256}


@pytest.mark.parametrize('s,mode,pad,ac', CASES, ids=[case_key(*c) for c in CASES])
def test_fp64_restatement_matches_the_reference(s, mode, pad, ac, golden):
    g = golden('warp_modes')
    dy, dm = deviation(g, s, mode, pad, ac)
    bound = ROUNDINGS[mode] * 2.0 ** -24 * float(np.abs(g['x_%d' % s]).max())
    print('%-34s max |y - y64| = %.3e (bound %.3e)   max |m - m64| = %.3e' % (case_key(s, mode, pad, ac), dy, bound, dm))
    assert dy <= bound
    assert dm <= ROUNDINGS[mode] * 2.0 ** -24


def test_bicubic_deviation_of_the_reference_is_what_the_gpu_bound_was_derived_from(golden):
    """tests/test_gpu_warp_modes.py bounds the device's bicubic error by 4 x the reference's own fp32 deviation from this
    file's fp64 restatement (BICUBIC_REFERENCE_DEVIATION in tests/warp_modes_cases.py): the constant must not be smaller than
    what is measured here, nor more than 10 % above it."""
    g = golden('warp_modes')
    worst = max(deviation(g, s, mode, pad, ac)[0] for s, mode, pad, ac in CASES if mode == 'bicubic')
    print('largest bicubic deviation of the reference from fp64: %.4e' % worst)
    assert worst <= BICUBIC_REFERENCE_DEVIATION <= 1.1 * worst


def test_the_fixture_exercises_what_it_claims(golden):
    g = golden('warp_modes')
    for s in (0, 1):
        _, c, h, w = g['x_%d' % s].shape
        assert c % 4 == 0
        flow = g['flow_%d' % s]
        assert (flow[0, :, :3] == 0).all()  # zero flow, corners included
        ix, iy = sample_position(flow, h, w, True)
        for p, size in ((ix, w), (iy, h)):
            assert p.min() <= -8 and p.max() >= size - 1 + 8  # two bicubic footprints outside every edge
        frac = np.abs(flow - np.round(flow))
        assert ((frac > 0.05) & (frac < 0.45)).mean() > 0.5  # sub-pixel motion
    assert g['x_0'].shape[2] % 2 == 1 and g['x_0'].shape[3] % 2 == 1
    # exact `nearest` ties (fp32 position on a half-integer) with a sample inside the frame
    n_ties = 0
    for ac in (True, False):
        ix, iy = sample_position(g['flow_1'], 17, 33, ac)
        n_ties += int(((ix - np.floor(ix) == 0.5) & (ix > 0) & (ix < 32)).sum() + ((iy - np.floor(iy) == 0.5) & (iy > 0) & (iy < 16)).sum())
    assert n_ties >= 50
    # the mask rule bites only under `zeros`, and there it zeroes whole pixels whose footprint is partly inside
    for s, mode, pad, ac in CASES:
        key = case_key(s, mode, pad, ac)
        m, y = g['m_' + key], g['y_' + key]
        if pad != 'zeros':
            assert (m >= 0.9999).all(), key
        else:
            partly = (m > 0.01) & (m < 0.9998)
            assert mode == 'nearest' or partly.sum() >= 8, key
            assert (y[:, :, partly[0]] == 0).all(), key
    # align_corners=False at zero flow is a zoom, not the identity
    y = g['y_0_bilinear_border_0']
    assert np.abs(y[0, :, 1, 5:-5] - g['x_0'][0, :, 1, 5:-5]).max() > 0.05
    assert np.abs(g['y_0_bilinear_border_1'][0, :, :3] - g['x_0'][0, :, :3]).max() < 1e-5  # (col * 2 / 52 - 1 does not round-trip in fp32)


@pytest.mark.skipif(not os.path.isdir('/root/reference/src'), reason='the reference checkout is not on this machine')
def test_fixture_regenerates_bit_for_bit(tmp_path, golden):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE='1')
    subprocess.run([sys.executable, os.path.join(ROOT, 'tools', 'gen_golden_warp.py'), '--out', str(tmp_path)], check=True, env=env)
    new, old = np.load(str(tmp_path / 'warp_modes.npz')), golden('warp_modes')
    assert sorted(new.files) == sorted(old.files) and len(old.files) == 4 + 2 * len(CASES)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].shape == old[k].shape, k
        assert new[k].tobytes() == old[k].tobytes(), k
    new, old = np.load(str(tmp_path / 'warp_nonfinite.npz')), golden('warp_nonfinite')  # (the non-finite flow sets of tests/op_regimes.py)
    assert sorted(new.files) == sorted(old.files)
    for k in old.files:
        assert new[k].dtype == old[k].dtype and new[k].tobytes() == old[k].tobytes(), k
