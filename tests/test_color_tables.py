"""The committed colour tables (aivc_amd/csrc/color_tables.h), evaluated in numpy with the arithmetic that
include/aivc_hip_color.h states, equal Pillow on ALL 2^24 triples, in both directions, with zero mismatches.  This pins the
restatement of Pillow's 8-bit JFIF conversion where there is no GPU; tests/test_gpu_color.py pins the kernels that read the
same tables."""
import ctypes
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import gen_color_tables as gct  # noqa: E402


@pytest.fixture(scope='module')
def tables():
    with open(os.path.join(ROOT, 'aivc_amd', 'csrc', 'color_tables.h')) as f:
        return gct.parse_header(f.read())


@pytest.fixture(scope='module')
def triples():
    img = gct.all_triples()
    flat = img.reshape(-1, 3).astype(np.uint32)
    assert np.unique((flat[:, 0] << 16) | (flat[:, 1] << 8) | flat[:, 2]).size == 1 << 24  # every triple, once
    return img


def test_tables_are_int16_and_complete(tables):
    assert sorted(tables) == sorted(gct.FORWARD + gct.INVERSE + ('HALF',))
    for name, t in tables.items():
        assert t.shape == (256,) and t.min() >= -32768 and t.max() <= 32767, name


def test_rgb_to_ycbcr_equals_pillow_on_every_triple(tables, triples):
    want = np.asarray(Image.fromarray(triples, 'RGB').convert('YCbCr'))
    r, g, b = (triples[..., k].astype(np.intp) for k in range(3))
    for k, got in enumerate(gct.forward_np(tables, r, g, b)):
        assert got.min() >= 0 and got.max() <= 255
        assert np.count_nonzero(got != want[..., k]) == 0, 'Y Cb Cr'.split()[k]


def test_ycbcr_to_rgb_equals_pillow_on_every_triple(tables, triples):
    want = np.asarray(Image.fromarray(triples, 'YCbCr').convert('RGB'))
    cb, cr = triples[..., 1].astype(np.intp), triples[..., 2].astype(np.intp)
    for k, got in enumerate(gct.inverse_np(tables, triples[..., 0], cb, cr)):
        assert np.count_nonzero(got != want[..., k]) == 0, 'RGB'[k]


def test_library_binds_the_color_entry_points_and_validates_arguments():
    """error paths return codes without launching anything (no GPU needed)"""
    from aivc_amd import _lib, abi
    fns = _lib.load()
    assert abi.ABI_VERSION >= 19 and set(abi.COLOR_PROTOTYPES) == {'aivc_rgb8_to_yuv420u8', 'aivc_yuv8_to_rgb8'}
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    assert fns['aivc_rgb8_to_yuv420u8'](None, 1, 2, 2, p, p, p, None) == -1
    assert fns['aivc_rgb8_to_yuv420u8'](p, 1, 0, 2, p, p, p, None) == -1
    assert fns['aivc_rgb8_to_yuv420u8'](p, 1, 2, 2, p, None, None, None) == -1          # a chroma sample exists: planes needed
    assert fns['aivc_yuv8_to_rgb8'](p, p, p, 1, 2, 2, 1, 1, 2, p, None) == -1            # chroma_shift
    assert fns['aivc_yuv8_to_rgb8'](p, p, p, 1, 1, 1, 0, 0, 1, p, None) == -1            # a chroma plane of size zero
    assert fns['aivc_yuv8_to_rgb8'](p, p, p, 1, 4, 4, 2, 2, 0, p, None) == -1            # full resolution asked, half given
    assert fns['aivc_yuv8_to_rgb8'](p, p, p, 1, 5, 5, 1, 2, 1, p, None) == -1            # fewer rows than floor(h / 2)
