"""aivc_rgb8_to_yuv420u8 / aivc_yuv8_to_rgb8 (include/aivc_hip_color.h) against Pillow, byte for byte, under the guard-zone and
poison harness of tests/guarded.py: every input sits between guard zones, every output of aivc_amd.ops is allocated between
them, each case runs under both fills and the two results must agree (an output byte that was not written follows the fill).

Shapes are (h, w).  The vector kernels need w % 16 == 0 and aligned pointers; everything else runs the scalar kernels.  The
edge shapes are the smallest at which the 2 x 2 ownership, an odd last row / column, a chroma plane of size zero (h or w of 1),
a single 16-pixel group, a partly filled workgroup and more than one workgroup can go wrong.  All indices are size_t in the
kernels; an image past 2^31 bytes (715 M pixels) is out of reach of a test of a few seconds and stays uncovered."""
import os
import sys

import numpy as np
import pytest
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

# the issue's shapes, then three on the vector path: one group, odd height with several row pairs, > 256 threads' worth
SHAPES = [(1, 1), (2, 2), (3, 5), (5, 3), (17, 33), (64, 66), (1, 64), (64, 1), (2, 16), (5, 32), (35, 272)]


def pil_ycbcr(rgb):
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a), 'RGB').convert('YCbCr')) for a in rgb])


def pil_rgb(ycc):
    return np.stack([np.asarray(Image.fromarray(np.ascontiguousarray(a), 'YCbCr').convert('RGB')) for a in ycc])


def planes_of(out, n, h, w, ch, cw):
    y, u, v = out
    return (np.frombuffer(y, np.uint8).reshape(n, h, w), np.frombuffer(u, np.uint8).reshape(n, ch, cw),
            np.frombuffer(v, np.uint8).reshape(n, ch, cw))


def forward_case(rgb, dev, misalign=False):
    from aivc_amd import ops

    def case(fill):
        if misalign:  # a contiguous tensor one byte into a guarded buffer: the scalar kernel at a vector-path width
            flat = guarded(np.concatenate([np.zeros(1, np.uint8), rgb.reshape(-1)]), dev, fill)
            x = flat[1:].view(rgb.shape)
            assert x.is_contiguous() and x.data_ptr() % 2 == 1
        else:
            x = guarded(rgb, dev, fill)
        return ops.rgb8_to_yuv420u8(x)
    return case


def upsampled(p, h, w):
    """nearest x 2, cropped to (h, w); a floor-sized plane of an odd side is one short: its last sample repeats"""
    q = np.repeat(np.repeat(p, 2, axis=-2), 2, axis=-1)
    q = np.pad(q, [(0, 0)] * (q.ndim - 2) + [(0, max(h - q.shape[-2], 0)), (0, max(w - q.shape[-1], 0))], mode='edge')
    return q[..., :h, :w]


@pytest.fixture(scope='module')
def every_triple():
    """the 4096 x 4096 image holding every triple once, and Pillow's two conversions of it"""
    i, j = np.meshgrid(np.arange(4096), np.arange(4096), indexing='ij')
    img = np.stack([i >> 4, ((i & 15) << 4) | (j >> 8), j & 255], axis=-1).astype(np.uint8)
    flat = img.reshape(-1, 3).astype(np.uint32)
    assert np.unique((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2]).size == 1 << 24
    return img, pil_ycbcr(img[None])[0], pil_rgb(img[None])[0]


def test_every_rgb_triple_forward(cuda, every_triple):
    img, ycc, _ = every_triple
    y, u, v = planes_of(both_fills(forward_case(img[None], cuda)), 1, 4096, 4096, 2048, 2048)
    assert np.array_equal(y[0], ycc[..., 0])
    assert np.array_equal(u[0], ycc[::2, ::2, 1])
    assert np.array_equal(v[0], ycc[::2, ::2, 2])


def test_every_ycbcr_triple_inverse(cuda, every_triple):
    from aivc_amd import ops
    img, _, rgb = every_triple
    planes = [np.ascontiguousarray(img[None, :, :, k]) for k in range(3)]
    got = both_fills(lambda fill: ops.yuv8_to_rgb8(*(guarded(p, cuda, fill) for p in planes), chroma_shift=0))
    assert np.array_equal(np.frombuffer(got, np.uint8).reshape(4096, 4096, 3), rgb)


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w', SHAPES)
def test_edge_shapes_forward(cuda, h, w, n):
    rgb = np.random.default_rng(h * 1000 + w * 10 + n).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
    ycc = pil_ycbcr(rgb)
    ch, cw = h // 2, w // 2
    for misalign in (False, True):
        y, u, v = planes_of(both_fills(forward_case(rgb, cuda, misalign)), n, h, w, ch, cw)
        assert np.array_equal(y, ycc[..., 0])
        assert np.array_equal(u, ycc[:, ::2, ::2, 1][:, :ch, :cw])
        assert np.array_equal(v, ycc[:, ::2, ::2, 2][:, :ch, :cw])


@pytest.mark.parametrize('n', [1, 3])
@pytest.mark.parametrize('h,w', SHAPES)
def test_edge_shapes_inverse(cuda, h, w, n):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    rng = np.random.default_rng(h * 1000 + w * 10 + n + 5)
    y = rng.integers(0, 256, (n, h, w), dtype=np.uint8)
    sizes = {'floor': (h // 2, w // 2), 'ceil': ((h + 1) // 2, (w + 1) // 2), 'full': (h, w)}
    for kind, (ch, cw) in sizes.items():
        shift = 0 if kind == 'full' else 1
        u, v = (rng.integers(0, 256, (n, ch, cw), dtype=np.uint8) for _ in range(2))

        def case(fill):
            return ops.yuv8_to_rgb8(guarded(y, cuda, fill), guarded(u, cuda, fill), guarded(v, cuda, fill), chroma_shift=shift)
        if ch * cw == 0:  # h or w of 1 leaves a floor-sized plane empty: there is no chroma to read, the call says so
            with pytest.raises(AivcNativeError):
                both_fills(case)
            continue
        uu, vv = (u, v) if kind == 'full' else (upsampled(u, h, w), upsampled(v, h, w))
        want = pil_rgb(np.stack([y, uu, vv], axis=-1))
        got = np.frombuffer(both_fills(case), np.uint8).reshape(n, h, w, 3)
        assert np.array_equal(got, want), kind


def test_round_trip_sizes_and_rejections(cuda):
    """the planes rgb8_to_yuv420u8 returns have the floor size and go back through yuv8_to_rgb8; CPU tensors are rejected"""
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    rgb = torch.from_numpy(np.random.default_rng(1).integers(0, 256, (2, 7, 9, 3), dtype=np.uint8))
    with pytest.raises(AivcNativeError):
        ops.rgb8_to_yuv420u8(rgb)
    y, u, v = ops.rgb8_to_yuv420u8(rgb.to(cuda))
    assert y.shape == (2, 7, 9) and u.shape == v.shape == (2, 3, 4) and y.dtype == u.dtype == torch.uint8
    with pytest.raises(AivcNativeError):
        ops.yuv8_to_rgb8(y.cpu(), u.cpu(), v.cpu())
    assert ops.yuv8_to_rgb8(y, u, v).shape == (2, 7, 9, 3)
