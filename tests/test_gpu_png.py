"""ops.png_encode and png.assemble on the device, against Pillow and zlib reading the result (png_cases.py: check_file).  Every case
runs three times -- with plain tensors and under both fills of the guard harness (tests/guarded.py) -- and the three results must
be the same bytes: the workspaces (filtered stream, slots, segment table) are poison when the kernels get them."""
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as pcs  # noqa: E402
from guarded import both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

# device stream bytes / zlib Z_RLE bytes on the SAME filtered bytes cut into the SAME segments, for the 1080p analytic picture at
# sigma = 3 and sigma = 1, as measured on the MI355X (experiments/png.md); the output is deterministic, the 2 % leave room for a
# later change of the segment rule
RLE_RATIO = {3: 0.99984, 1: 0.99913}
MARGIN = 1.02


def coded(pictures, filter, dev):
    """the pictures (arrays [h, w, c] of one size) as one batch -> their files; plain and under both fills, identical bytes"""
    from aivc_amd import ops, png
    batch = np.stack(pictures)
    n, h, w, c = batch.shape

    def run(place):
        return [png.assemble(w, h, c, z) for z in ops.png_encode(place(batch), filter)]
    plain = run(lambda a: torch.from_numpy(a).to(dev))
    assert both_fills(lambda fill: run(lambda a: guarded(a, dev, fill))) == plain and len(plain) == n
    return plain


def stream_of(png):
    return dict(pcs.chunks(png))[b'IDAT']


@pytest.mark.parametrize('c', (1, 3))
@pytest.mark.parametrize('h,w', pcs.GEOMETRY)
def test_geometry(h, w, c, cuda):
    pix = pcs.random_picture(h, w, c, seed=31 * h + w + c)
    filtered = pcs.check_file(coded([pix], 5, cuda)[0], pix)
    # filter 5 is defined to the byte: the smallest sum of absolute residuals, the lowest type among equals
    assert filtered == pcs.filter_rows(pix, pcs.adaptive_types(pix)).tobytes()


def test_a_row_longer_than_the_segment_target(cuda):
    h, w, c = pcs.LONG_ROW
    pix = pcs.random_picture(h, w, c, seed=9)
    assert pcs.segment_lengths(h, w, c) == [18001] * 3
    pcs.check_file(coded([pix], 5, cuda)[0], pix)


def test_a_batch_codes_each_picture_as_it_codes_it_alone(cuda):
    pictures = [pcs.random_picture(38, 70, 3, seed=s) for s in (1, 2, 3)]
    batch = coded(pictures, 5, cuda)
    assert len(set(batch)) == 3
    for pix, png in zip(pictures, batch):
        pcs.check_file(png, pix)
        assert coded([pix], 5, cuda)[0] == png


@pytest.mark.parametrize('c', (1, 3))
@pytest.mark.parametrize('filter', range(6))
def test_every_filter(filter, c, cuda):
    pix = pcs.random_picture(38, 70, c, seed=40 + filter)
    filtered = pcs.check_file(coded([pix], filter, cuda)[0], pix, filter)
    types = pcs.adaptive_types(pix) if filter == 5 else np.full(38, filter)
    assert filtered == pcs.filter_rows(pix, types).tobytes()


# ---- the coder's edge cases ----------------------------------------------------------------------------------------------------------
def test_constant_picture_is_coded_by_runs(cuda):
    pix = np.full((256, 256, 3), 77, np.uint8)
    png = coded([pix], 5, cuda)[0]
    pcs.check_file(png, pix)
    raw = 256 * (1 + 256 * 3)
    print('constant 256 x 256 x 3: %d bytes of %d raw' % (len(stream_of(png)), raw))
    assert len(stream_of(png)) < raw / 16  # Huffman coding alone cannot go below 1 bit per byte, 1/8


def test_two_valued_picture(cuda):
    pix = (np.random.default_rng(2).integers(0, 2, (38, 70, 1)) * 255).astype(np.uint8)
    for filter in (0, 5):
        pcs.check_file(coded([pix], filter, cuda)[0], pix, filter)


def test_random_bytes_fall_back_to_stored_blocks(cuda):
    from aivc_amd import png
    h, w, c = 64, 64, 3
    pix = np.random.default_rng(3).integers(0, 256, (h, w, c)).astype(np.uint8)
    data = coded([pix], 0, cuda)[0]
    pcs.check_file(data, pix, 0)
    bound = 2 + sum(png.stored_bound(n) for n in pcs.segment_lengths(h, w, c)) + 5 + 4
    print('random 64 x 64 x 3: %d bytes, bound %d' % (len(stream_of(data)), bound))
    assert len(stream_of(data)) <= bound


def test_fibonacci_counts_need_the_length_limit(cuda):
    pix = pcs.fibonacci_picture()
    assert pcs.segment_lengths(*pix.shape) == [16384]
    pcs.check_file(coded([pix], 0, cuda)[0], pix, 0)


def test_a_segment_that_uses_all_256_values_equally(cuda):
    pix = pcs.all_values_picture()
    assert len(pcs.segment_lengths(*pix.shape)) == 1 and (np.bincount(pix.reshape(-1), minlength=256) == 63).all()
    pcs.check_file(coded([pix], 0, cuda)[0], pix, 0)


# ---- 1080p ------------------------------------------------------------------------------------------------------------------------
SIGMAS = (3, 1, 0)


@pytest.fixture(scope='module')
def batch_1080p(cuda):
    pictures = [pcs.analytic_picture(1080, 1920, s, seed=1 + s) for s in SIGMAS]
    return pictures, coded(pictures, 5, cuda)


def test_one_batch_of_three_1080p_pictures(batch_1080p):
    pictures, files = batch_1080p
    assert len(pcs.segment_lengths(1080, 1920, 3)) == 540
    for pix, png in zip(pictures, files):
        pcs.check_file(png, pix)


@pytest.mark.parametrize('sigma', (3, 1))
def test_size_against_zlib_rle_on_the_same_segments(sigma, batch_1080p):
    pictures, files = batch_1080p
    stream = stream_of(files[SIGMAS.index(sigma)])
    ref = pcs.stitched_stream(zlib.decompress(stream), pcs.segment_lengths(1080, 1920, 3), zlib.Z_RLE)
    ratio = len(stream) / len(ref)
    print('sigma %d: device %d bytes, zlib Z_RLE on the same segments %d bytes, ratio %.5f' % (sigma, len(stream), len(ref), ratio))
    assert ratio <= RLE_RATIO[sigma] * MARGIN
