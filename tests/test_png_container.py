"""The host half of the device PNG coder (aivc_amd/png.py), no GPU: the container around stand-in zlib streams that are built the
way the device builds its own -- independent deflate segments of whole rows, each ended by a sync flush, stitched (png_cases.py:
stitched_stream) --, the Adler-32 fold against zlib.adler32, the segment rule and the slot capacity, the C ABI without a launch,
and the --png_coder flag."""
import ctypes
import io
import os
import sys
import zlib

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as pcs  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(h, w, c) for h, w in pcs.GEOMETRY for c in (1, 3)] + [pcs.LONG_ROW]


# ---- the container -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,c', SIZES)
def test_assemble_round_trip_of_stitched_segments(h, w, c):
    from aivc_amd import png
    pix = pcs.random_picture(h, w, c, seed=h * 1000 + w + c)
    for types, strategy in ((np.full(h, 1), zlib.Z_HUFFMAN_ONLY), (pcs.adaptive_types(pix), zlib.Z_RLE)):
        filtered = pcs.filter_rows(pix, types)
        assert png.segment_lengths(h, w, c) == pcs.segment_lengths(h, w, c)
        z = pcs.stitched_stream(filtered.tobytes(), png.segment_lengths(h, w, c), strategy)
        assert pcs.check_file(png.assemble(w, h, c, z), pix) == filtered.tobytes()


def test_assemble_is_the_file_pillow_reads_and_refuses_other_pictures():
    from PIL import Image
    from aivc_amd import png
    pix = pcs.random_picture(5, 7, 3, 1)
    z = zlib.compress(pcs.filter_rows(pix, np.zeros(5, np.int64)).tobytes())
    data = png.assemble(7, 5, 3, z)
    assert data[:8] == png.SIGNATURE and data[-12:] == b'\x00\x00\x00\x00IEND\xaeB`\x82'
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), pix)
    for bad in ((0, 5, 3), (7, 0, 3), (7, 5, 2), (7, 5, 4)):
        with pytest.raises(ValueError):
            png.assemble(bad[0], bad[1], bad[2], z)


# ---- Adler-32 ----------------------------------------------------------------------------------------------------------------------
def _fold(data, lengths):
    from aivc_amd import png
    parts, at = [], 0
    for n in lengths:
        parts.append(png.adler_partial(data[at:at + n]))
        at += n
    assert at == len(data)
    return png.adler_fold(parts)


@pytest.mark.parametrize('h,w,c', SIZES)
def test_adler_fold_over_every_segment_plan(h, w, c):
    from aivc_amd import png
    data = pcs.filter_rows(pcs.random_picture(h, w, c, seed=7), np.full(h, 4)).tobytes()
    assert _fold(data, png.segment_lengths(h, w, c)) == zlib.adler32(data) & 0xffffffff


def test_adler_fold_long_runs_of_ff_and_sums_past_32_bits():
    from aivc_amd import png
    data = b'\xff' * 20000  # one segment longer than 5552 bytes of 0xFF
    assert png.adler_fold([png.adler_partial(data)]) == zlib.adler32(data) & 0xffffffff
    # s2 of this segment, unreduced, is 255 * n (n + 1) / 2 > 2^32 for n = 6000: plain 32-bit sums would overflow
    n = 6000
    assert 255 * n * (n + 1) // 2 > 1 << 32
    data = b'\xff' * (3 * n + 17)
    assert _fold(data, [n, n, n, 17]) == zlib.adler32(data) & 0xffffffff
    rng = np.random.default_rng(3)
    data = rng.integers(200, 256, 100001).astype(np.uint8).tobytes()
    assert _fold(data, [1, 5552, 5553, 16384, 100001 - 1 - 5552 - 5553 - 16384]) == zlib.adler32(data) & 0xffffffff
    assert png.adler_fold([]) == 1 == zlib.adler32(b'')


# ---- segments ----------------------------------------------------------------------------------------------------------------------
def test_segment_plan_and_slot_capacity():
    from aivc_amd import png
    # (h, w, c) -> rows per segment, segments
    for (h, w, c), want in {(1, 1, 1): (1, 1), (1, 37, 3): (1, 1), (37, 1, 1): (37, 1), (37, 1, 3): (37, 1), (20000, 1, 1): (8192, 3),
                            (3, 6000, 3): (1, 3), (1080, 1920, 3): (2, 540), (129, 127, 1): (128, 2), (1, 70000, 1): (1, 1)}.items():
        rows, nseg, stride, slot = png.segment_plan(h, w, c)
        row = 1 + w * c
        assert (rows, nseg) == want and rows == pcs.rows_per_segment(h, w, c)
        lengths = png.segment_lengths(h, w, c)
        assert len(lengths) == nseg and sum(lengths) == h * row and max(lengths) == rows * row and all(n % row == 0 and n > 0 for n in lengths)
        assert rows * row <= max(png.SEGMENT_TARGET, row)  # a row longer than the target is a segment of its own
        assert stride % 16 == 0 and 0 <= stride - rows * row < 16
        # the slot holds the stored form of the segment and the empty stored block behind a coded one
        assert slot % 16 == 0 and slot >= png.stored_bound(rows * row) + 4
    assert png.stored_bound(1) == 6 and png.stored_bound(65535) == 65540 and png.stored_bound(65536) == 65546
    assert png.stored_bound(70001) == 70001 + 10
    # zlib's own stored form of incompressible bytes obeys the bound the slot is sized by
    data = np.random.default_rng(0).integers(0, 256, 70001).astype(np.uint8).tobytes()
    co = zlib.compressobj(0, zlib.DEFLATED, -15)
    assert len(co.compress(data) + co.flush(zlib.Z_SYNC_FLUSH)) <= png.slot_capacity(len(data))
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 2)):
        with pytest.raises(ValueError):
            png.segment_plan(*bad)


# ---- the C entry points, no launch ---------------------------------------------------------------------------------------------------
def test_library_exports_and_abi():
    from aivc_amd import abi
    assert abi.ABI_VERSION == 26 and set(abi.PNG_PROTOTYPES) == {'aivc_png_deflate', 'aivc_png_gather'}
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    for name in abi.PNG_PROTOTYPES:
        assert hasattr(lib, name), 'libaivc_hip.so does not export %s' % name
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == abi.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_png.h')).read()
    assert all('int %s(' % name in header for name in abi.PNG_PROTOTYPES)
    assert '#define AIVC_PNG_RUN %d ' % abi.PNG_RUN in header and '#define AIVC_PNG_SEG_WORDS %d ' % abi.PNG_SEG_WORDS in header
    from aivc_amd import _lib
    fns = _lib.load()  # the loader binds them beside what abi.declare binds, each with its stream argument
    for name, args in abi.PNG_PROTOTYPES.items():
        assert fns[name].argtypes == list(args) + [ctypes.c_void_p] and fns[name].restype is ctypes.c_int
    assert not set(abi.PNG_PROTOTYPES) & set(abi.declare(lib))  # what declare() binds stays as it is


def test_argument_errors_without_a_launch():
    from aivc_amd import _lib
    fns = _lib.load()

    def deflate(pix=1, n=1, h=4, w=4, c=3, filter=5, rows=2, filt=16, slots=16, info=16):
        return fns['aivc_png_deflate'](pix, n, h, w, c, filter, rows, filt, slots, info, None)

    def gather(slots=16, info=16, dst=16, n=1, h=4, w=4, c=3, rows=2, out=16):
        return fns['aivc_png_gather'](slots, info, dst, n, h, w, c, rows, out, None)
    for kw in (dict(pix=None), dict(filt=None), dict(slots=None), dict(info=None), dict(n=0), dict(n=-1), dict(h=0), dict(w=0), dict(w=-3),
               dict(c=0), dict(c=2), dict(c=4), dict(filter=-1), dict(filter=6), dict(rows=0)):
        assert deflate(**kw) == -1, kw
    for kw in (dict(slots=None), dict(info=None), dict(dst=None), dict(out=None), dict(n=0), dict(h=0), dict(w=0), dict(c=2), dict(rows=0)):
        assert gather(**kw) == -1, kw
    assert deflate(h=1, w=1 << 30, c=3, rows=1) == -2  # a segment of 2^31 bytes or more


# ---- the flag ------------------------------------------------------------------------------------------------------------------------
def test_png_coder_flag(tmp_path, capsys):
    from aivc_amd import aivc as aivc_cli
    from aivc_amd import decode as dec_cli
    from aivc_amd import png
    assert png.CODERS == ('pillow', 'device')
    folder = str(tmp_path / 'pictures') + '/'
    for cli in (dec_cli, aivc_cli):
        assert cli.parse_args(['-o', folder]).png_coder == 'pillow'
        assert cli.parse_args(['-o', folder, '--png_coder', 'pillow']).png_coder == 'pillow'
        assert cli.parse_args(['-o', folder, '--png_coder', 'device']).png_coder == 'device'
        assert cli.parse_args(['-o', str(tmp_path), '--png_coder', 'device']).png_coder == 'device'  # an existing directory
        assert cli.parse_args(['-o', str(tmp_path / 'out.yuv'), '--png_coder', 'pillow']).png_coder == 'pillow'
        for argv in (['-o', str(tmp_path / 'out.yuv'), '--png_coder', 'device'], ['-o', str(tmp_path / 'out.y4m'), '--png_coder', 'device'],
                     ['-o', folder, '--png_coder', 'zlib']):
            with pytest.raises(SystemExit) as e:
                cli.parse_args(argv)
            assert e.value.code == 2
        assert '--png_coder' in capsys.readouterr().err
    assert png.check_coder('device', folder, True) == 'device' and png.check_coder('device') == 'device'
    with pytest.raises(ValueError):
        png.check_coder('device', 'out.yuv', False)
    with pytest.raises(ValueError):
        png.check_coder('gpu')


def test_default_arguments_keep_the_pillow_path():
    import inspect
    from aivc_amd.func_util import img_processing
    from aivc_amd.real_life import decode
    assert inspect.signature(decode.write_png_folder).parameters['coder'].default == 'pillow'
    assert inspect.signature(img_processing.save_tensor_as_img).parameters['coder'].default == 'pillow'
    with pytest.raises(ValueError):
        decode.write_png_folder([], '/nonexistent/never-made', 'cpu', [], coder='zlib')
