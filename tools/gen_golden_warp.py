#!/usr/bin/env python3
"""Generate tests/golden/warp_modes.npz by IMPORTING the reference's own warp() (src/func_util/optical_flow.py:14-55).

Runs only where the reference checkout is present; the test-suite uses the committed fixture.  Nothing from the reference is
copied: the fixture holds seeded inputs and what the reference computes for them on CPU (torch fp32) in all 18 combinations of
interpol_mode x padding_mode x align_corners, for two shapes:

    shape 0   x [1, 4, 29, 53]   odd sides, size - 1 not a power of two
    shape 1   x [1, 8, 17, 33]   size - 1 = 16 / 32: (col + v) * 2 / (size - 1) - 1 is exact for half-integer col + v, so the
                                 flows of its tie block land EXACTLY on half-integers in the reference's fp32 (the `nearest` tie)

The flows mix sub-pixel motion, a zero-flow block (rows 0 ... 2, which hold the frame corners), the tie block (shape 1) and,
along every edge, vectors that carry the sample up to 12 pixels (three bicubic footprints) outside the frame.

Per case the file stores y_<shape>_<interp>_<pad>_<ac> (the reference's output) and m_<...> [1, h, w]: the fp32 value of the
reference's mask BEFORE its threshold: the return value of the reference's own second grid_sample call, recorded while its
warp() runs (warp_and_mask).

The tool asserts what tests/test_warp_modes.py and tests/test_gpu_warp_modes.py rely on: at most 0.5 % of the pixels of any
case have a mask within 1e-5 of the threshold 0.9999, and at most 0.5 % of the `nearest` samples lie within 1e-4 of a
half-integer without being exactly on it.

A second, small file, tests/golden/warp_nonfinite.npz, holds one set x [1, 4, 9, 11] in the same layout (shape index 0) whose
N(0, 1) * 2 flow carries the sets of nonfinite_flow_sets() below (those of FLOWS in tests/op_regimes.py) -- NaN in x, in y, in
both, +-inf, +-3e38, whole positions -- at 5 pixels each: what the reference does with a flow that is not finite, in all 18 modes.

    python tools/gen_golden_warp.py [--out DIR]     # rewrites tests/golden/warp_modes.npz and warp_nonfinite.npz
"""
import os
import sys

sys.dont_write_bytecode = True
os.environ['PYTHONDONTWRITEBYTECODE'] = '1'

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import REF, install_stubs  # noqa: E402

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden')

INTERP = ('bilinear', 'nearest', 'bicubic')
PAD = ('border', 'zeros', 'reflection')
SHAPES = ((1, 4, 29, 53), (1, 8, 17, 33))
NONFINITE_SHAPE = (1, 4, 9, 11)
MASK_THRESHOLD = 0.9999
MASK_BAND = 1e-5    # pixels whose stored mask is this close to the threshold are left out of the comparisons
TIE_BAND = 1e-4     # `nearest` samples this close to a half-integer (and not on it) likewise
MAX_LEFT_OUT = 0.005


def make_flow(gen, h, w, ties):
    """[1, 2, h, w] pixel-unit flow, channel 0 horizontal."""
    flo = torch.randn(1, 2, h, w, generator=gen) * 1.5  # sub-pixel and few-pixel motion
    u = lambda *s: torch.rand(*s, generator=gen)
    rows = torch.arange(h, dtype=torch.float32).view(h, 1)
    cols = torch.arange(w, dtype=torch.float32).view(1, w)
    # along every edge: from each pixel of a 3-pixel band to between 0.3 and 12 pixels outside the frame
    flo[0, 0, 6:, 0:3] = -(cols[:, 0:3] + 0.3 + 11.7 * u(h - 6, 3))
    flo[0, 0, 6:, w - 3:] = (w - 1 - cols[:, w - 3:]) + 0.3 + 11.7 * u(h - 6, 3)
    flo[0, 1, 3:6, :] = -(rows[3:6] + 0.3 + 11.7 * u(3, w))
    flo[0, 1, h - 3:, :] = (h - 1 - rows[h - 3:]) + 0.3 + 11.7 * u(3, w)
    # zero flow: the first rows (with two corners of the frame) and the last pixel of the frame
    flo[0, :, 0:3, :] = 0.0
    flo[0, :, h - 1, w - 1] = 0.0
    if ties:
        # half-integer displacements in one or both directions, in frame and across the left edge
        k = torch.randint(-3, 3, (2, 4, 12), generator=gen).float() + 0.5
        flo[0, :, 7:11, 1:13] = k
        flo[0, 1, 7:9, 1:13] = torch.randint(-2, 3, (2, 12), generator=gen).float()  # ... horizontal tie only
        flo[0, 0, 9:10, 1:7] = torch.randint(-2, 3, (1, 6), generator=gen).float()  # ... vertical tie only
    return flo


def nonfinite_flow_sets():
    """The flow sets of the non-finite fixture, in order: [(name, kinds)], a kind (fx, fy) with None = the drawn value stays, or a
    function (row, col, h, w) -> (fx, fy).  Pixel i of a set takes kind i modulo their number.  The same sets, in the same
    order, as FLOWS of tests/op_regimes.py; tests/test_op_regimes.py rebuilds the fixture's flow from that table and compares."""
    nan, inf, big = np.float32(np.nan), np.float32(np.inf), np.float32(3e38)
    return [('nan_x', [(nan, None)]), ('nan_y', [(None, nan)]), ('nan_xy', [(nan, nan)]),
            ('inf', [(inf, None), (-inf, None), (None, inf), (None, -inf), (inf, -inf)]),
            ('big', [(big, None), (-big, None), (None, big), (None, -big), (-big, big)]),
            ('integer', [lambda r, q, h, w: (np.float32((q + 2) % w - q), np.float32((r + 1) % h - r)),   # a whole position inside
                         lambda r, q, h, w: (np.float32(w - 1 - q), np.float32(h - 1 - r)),              # exactly size - 1
                         lambda r, q, h, w: (np.float32(-q), np.float32(-r))])]                          # position 0


def nonfinite_flow(gen, rng, h, w, per_set=5):
    """[1, 2, h, w]: an N(0, 1) * 2 flow with every set of nonfinite_flow_sets() planted at per_set pixels of its own"""
    flow = (torch.randn(1, h, w, 2, generator=gen) * 2.0).numpy()
    sets = nonfinite_flow_sets()
    _, rows, cols = np.unravel_index(rng.permutation(h * w)[:per_set * len(sets)], (1, h, w))
    for i, (_, kinds) in enumerate(sets):
        for j in range(per_set):
            r, q = int(rows[per_set * i + j]), int(cols[per_set * i + j])
            kind = kinds[j % len(kinds)]
            fx, fy = kind(r, q, h, w) if callable(kind) else kind
            if fx is not None:
                flow[0, r, q, 0] = fx
            if fy is not None:
                flow[0, r, q, 1] = fy
    return torch.from_numpy(np.ascontiguousarray(np.transpose(flow, (0, 3, 1, 2))))


def sample_position(flo, h, w, align_corners):
    """the reference's normalisation (its lines 31-35) and grid_sample's unnormalisation, in fp32 like both"""
    f = np.float32
    v = flo.numpy().astype(f)
    out = []
    for ch, size in ((0, w), (1, h)):
        base = np.arange(size, dtype=f).reshape((1, size) if ch == 0 else (size, 1))
        g = (f(2.0) * (base + v[0, ch])) / f(max(size - 1, 1)) - f(1.0)
        if align_corners:
            out.append((g + f(1.0)) * f((size - 1) / 2.0))
        else:
            # torch's CPU kernel contracts this into ONE fused multiply-add; the product and the difference are exact in fp64
            out.append(((g + f(1.0)).astype(np.float64) * (size / 2.0) - 0.5).astype(f))
    return out  # [ix, iy], each [h, w] fp32


def warp_and_mask(warp, x, flo, mode, pad, ac):
    """the reference's warp(x, flo, ...) -> (its result, the mask it sampled before thresholding it: one channel, all are
    alike).  The mask is what the reference's second grid_sample call returned, kept aside (cloned: the reference thresholds
    it in place) by standing in front of torch's grid_sample for the duration of the call."""
    functional = torch.nn.functional
    real, seen = functional.grid_sample, []

    def recording(*args, **kwargs):
        out = real(*args, **kwargs)
        seen.append(out.detach().clone())
        return out
    functional.grid_sample = recording
    try:
        with torch.no_grad():
            y = warp(x, flo, interpol_mode=mode, padding_mode=pad, align_corners=ac)
    finally:
        functional.grid_sample = real
    assert len(seen) == 2 and seen[1].shape == x.shape, len(seen)  # the image, then the ones
    return y, seen[1][:, 0]


def main():
    out_dir = OUT
    if len(sys.argv) > 2 and sys.argv[1] == '--out':
        out_dir = sys.argv[2]
    install_stubs()
    sys.path.insert(0, REF)
    import func_util.console_display as cd
    cd.FLAG_QUIET = True
    from func_util.optical_flow import warp

    torch.set_num_threads(1)
    gen = torch.Generator().manual_seed(1418)
    arrs = {}

    def every_mode(arrs, s, x, flo):
        """the 18 modes of one set into arrs -> the number of exact `nearest` ties"""
        _, _, h, w = x.shape
        arrs['x_%d' % s], arrs['flow_%d' % s] = x.numpy(), flo.numpy()
        n_exact = 0
        for mode in INTERP:
            for pad in PAD:
                for ac in (True, False):
                    y, m = warp_and_mask(warp, x, flo, mode, pad, ac)
                    key = '%d_%s_%s_%d' % (s, mode, pad, int(ac))
                    arrs['y_' + key], arrs['m_' + key] = y.numpy(), m.numpy()
                    with np.errstate(over='ignore', invalid='ignore'):  # (a NaN mask or position is in no band)
                        left_out = np.abs(m.numpy() - np.float32(MASK_THRESHOLD)) < MASK_BAND
                        if mode == 'nearest':
                            for p in sample_position(flo, h, w, ac):
                                d = np.abs(p - np.floor(p) - np.float32(0.5))
                                left_out = left_out | ((d < TIE_BAND) & (d != 0))[None]
                                n_exact += int((d == 0).sum())
                    assert left_out.mean() <= MAX_LEFT_OUT, (key, left_out.mean())
        return n_exact

    for s, shape in enumerate(SHAPES):
        _, c, h, w = shape
        x = torch.randn(*shape, generator=gen)
        flo = make_flow(gen, h, w, ties=(s == 1))
        n_exact = every_mode(arrs, s, x, flo)
        if s == 1:
            assert n_exact >= 100, n_exact  # the tie block does land on half-integers in fp32
        ix, iy = sample_position(flo, h, w, True)
        for p, size in ((ix, w), (iy, h)):  # >= 2 bicubic footprints outside every edge
            assert p.min() <= -8 and p.max() >= size - 1 + 8, (s, p.min(), p.max())
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, 'warp_modes.npz')
    np.savez_compressed(path, **arrs)
    print('%-34s %7.1f kB' % ('warp_modes.npz', os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < 1 << 20

    # the non-finite set: its own generators, so that warp_modes.npz above does not move
    _, c, h, w = NONFINITE_SHAPE
    gen = torch.Generator().manual_seed(1419)
    rng = np.random.default_rng(1419)
    x = torch.randn(*NONFINITE_SHAPE, generator=gen)
    flo = nonfinite_flow(gen, rng, h, w)
    assert int(torch.isnan(flo).any(dim=1).sum()) == 15 and int(torch.isinf(flo).any(dim=1).sum()) == 5
    arrs = {}
    every_mode(arrs, 0, x, flo)
    path = os.path.join(out_dir, 'warp_nonfinite.npz')
    np.savez_compressed(path, **arrs)
    print('%-34s %7.1f kB' % ('warp_nonfinite.npz', os.path.getsize(path) / 1e3))
    assert os.path.getsize(path) < 1 << 20


if __name__ == '__main__':
    main()
