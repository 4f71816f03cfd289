"""ops.inflate, ops.png_unfilter and png.read_pictures on the device against zlib.decompress, the numpy filters of png_cases.py and
Pillow's pixels (the cases: png_read_cases.py).  Every case runs three times -- with plain tensors and under both fills of the
guard harness (tests/guarded.py) -- and the three results must be the same bytes.  The damaged streams have all been through the
sanitized host build of the same decoder text (tests/test_png_read.py); here they show that a failing stream stays inside its own
destination range and its own status row."""
import io
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import png_cases as pcs  # noqa: E402
import png_read_cases as cases  # noqa: E402
from guarded import _as_bytes, both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

VALID = {name: (z, d) for name, z, d in cases.VALID}


def three_ways(case):
    """case(fill): fill None -- plain tensors; else inside guard_ops(fill).  -> the result, the same bytes all three times"""
    plain = _as_bytes(case(None))
    assert both_fills(case) == plain
    return plain


def place(array, dev, fill):
    return torch.from_numpy(np.ascontiguousarray(array)).to(dev) if fill is None else guarded(array, dev, fill)


# ---- inflate ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(VALID))
def test_inflate_each_valid_stream_alone(name, cuda):
    from aivc_amd import ops
    z, want = VALID[name]
    got = three_ways(lambda fill: ops.inflate([z], [len(want)], cuda))
    assert got == [want]


def test_inflate_all_valid_streams_in_one_batch(cuda):
    from aivc_amd import ops
    names = sorted(VALID)
    streams, wants = [VALID[n][0] for n in names], [VALID[n][1] for n in names]
    starts = 32 * len(names) + np.cumsum([0] + [len(z) for z in streams])[:-1]
    assert (starts % 2 == 1).any() and (starts % 4 != 0).any()  # sources back to back: whatever byte they fall on
    dst_starts = np.cumsum([3] + [len(d) + 3 for d in wants])[:-1]
    assert (dst_starts % 2 == 1).any()

    def case(fill):
        outs, rows, _ = ops.inflate(streams, [len(d) for d in wants], cuda, check=False, gap=3)
        assert (rows[:, 0] == 0).all() and rows[:, 1].tolist() == [len(d) for d in wants] and rows[:, 2].tolist() == [len(z) for z in streams]
        return outs
    assert three_ways(case) == wants


def test_inflate_more_streams_than_compute_units(cuda):
    from aivc_amd import ops
    data = next(d for d in (bytes(range(k)) * 2 for k in range(8, 40)) if len(zlib.compress(d)) == 40)
    z = zlib.compress(data)
    assert three_ways(lambda fill: ops.inflate([z] * 600, [len(data)] * 600, cuda)) == [data] * 600


def test_damaged_streams_stay_in_their_own_ranges(cuda):
    from aivc_amd import ops
    neighbours = ['stored-1', 'repeat-symbols', 'lone-distance-code', 'fibonacci-15-bits', 'text-rle', 'every-symbol']
    streams, sizes, valid_at = [], [], {}
    for k, (name, z, expect) in enumerate(cases.DAMAGED):
        streams.append(z), sizes.append(expect)
        if k % 2 == 0:  # a valid neighbour behind every second damaged stream
            n = neighbours[(k // 2) % len(neighbours)]
            valid_at[len(streams)] = n
            streams.append(VALID[n][0]), sizes.append(len(VALID[n][1]))
    gap = 5
    starts = np.cumsum([gap] + [s + gap for s in sizes])

    def case(fill):
        outs, rows, dst = ops.inflate(streams, sizes, cuda, check=False, gap=gap)
        host = dst.cpu().numpy()
        for i in range(len(streams)):
            if i in valid_at:
                assert rows[i, 0] == 0 and rows[i, 1] == sizes[i] and outs[i].cpu().numpy().tobytes() == VALID[valid_at[i]][1], valid_at[i]
            else:
                assert rows[i, 0] != 0 and rows[i, 1] <= sizes[i], i
            if fill is not None:  # the bytes between the ranges, and a damaged stream's range behind what it produced, keep the fill
                assert (host[starts[i] - gap:starts[i]] == fill).all(), i
                if i not in valid_at:
                    assert (host[starts[i] + int(rows[i, 1]):starts[i] + sizes[i]] == fill).all(), i
        if fill is not None:
            assert (host[starts[-1] - gap:] == fill).all()
        return rows, [outs[i] for i in valid_at]
    three_ways(case)
    with pytest.raises(ValueError, match=r'stream 0: '):
        ops.inflate(streams, sizes, cuda)
    with pytest.raises(ValueError, match=r'stream 1: '):
        ops.inflate(streams[1:3] + streams[:1], sizes[1:3] + sizes[:1], cuda)  # (stream 0 of this batch is the valid neighbour)


# ---- unfilter -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,c', cases.SIZES)
def test_unfilter_every_type_batch_and_alone(h, w, c, cuda):
    from aivc_amd import ops
    pictures = cases.picture_cases(h, w, c)

    def case(fill):
        filt = [place(f, cuda, fill) for _, f in pictures]
        batch = ops.png_unfilter(filt, [(h, w, c)] * len(pictures))
        alone = [ops.png_unfilter([f], [(h, w, c)])[0] for f in filt]
        return batch, alone
    batch, alone = three_ways(case)
    assert batch == [p.tobytes() for p, _ in pictures] and alone == batch


def test_unfilter_mixed_shapes_and_a_type_byte_of_five(cuda):
    from aivc_amd import ops
    good = [cases.picture_cases(h, w, c)[k] for (h, w, c), k in (((129, 127, 1), 4), ((65, 33, 3), 5), ((1, 37, 3), 3))]
    bad = cases.bad_type_picture()
    pictures = [good[0], bad, good[1], good[2]]

    def case(fill):
        pics, status = ops.png_unfilter([place(f, cuda, fill) for _, f in pictures], [p.shape for p, _ in pictures], check=False)
        return status, [pics[0], pics[2], pics[3]]
    status, pics = three_ways(case)
    assert np.frombuffer(status, np.uint32).tolist() == [0, 1, 0, 0]
    assert pics == [p.tobytes() for p, _ in good]
    with pytest.raises(ValueError, match='picture 1: '):
        ops.png_unfilter([torch.from_numpy(f.copy()).to(cuda) for _, f in pictures], [p.shape for p, _ in pictures])


# ---- files --------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp('png_read')
    paths = {}
    for name, (data, mode) in list(cases.FILES.items()) + list(cases.OTHER_KINDS.items()):
        paths[name] = (str(tmp / (name + '.png')), mode)
        with open(paths[name][0], 'wb') as f:
            f.write(data)
    return tmp, paths


def pillow_pixels(path, mode):
    from PIL import Image
    img = Image.open(path)
    if img.mode != mode:
        img = img.convert(mode)
    a = np.asarray(img)
    return a.reshape(a.shape[0], a.shape[1], -1)


def profiled(run):
    """-> (what run() returns, the names of the launches ops.PROFILE_HBM saw)"""
    from aivc_amd import ops
    ops.PROFILE_HBM = []
    try:
        out = run()
        return out, [name for name, _, _, _ in ops.PROFILE_HBM]
    finally:
        ops.PROFILE_HBM = None


@pytest.mark.parametrize('mode', ('L', 'RGB'))
def test_read_pictures_is_pillow_pixel_for_pixel(mode, files, cuda):
    from aivc_amd import png
    _, paths = files
    names = sorted(n for n in cases.FILES if paths[n][1] == mode)
    stats = {}

    def case(fill):
        pics, launches = profiled(lambda: png.read_pictures([paths[n][0] for n in names], cuda, mode, stats))
        assert launches == ['inflate', 'png_unfilter']  # one of each for the whole list
        return pics
    got = three_ways(case)
    assert stats == {'device': 3 * len(names), 'pillow': 0}
    for n, g in zip(names, got):
        assert g == pillow_pixels(paths[cases.PIXELS_FROM.get(n, n)][0], mode).tobytes(), n


def test_other_kinds_come_back_through_pillow(files, cuda):
    from aivc_amd import png
    _, paths = files
    stats = {}
    for mode in ('L', 'RGB'):
        names = sorted(cases.OTHER_KINDS) + ['grey-default', 'rgb-default']  # (one of the two is of the other colour type)
        pics, launches = profiled(lambda: png.read_pictures([paths[n][0] for n in names], cuda, mode, stats))
        assert launches == ['inflate', 'png_unfilter']  # the one eligible file
        for n, p in zip(names, pics):
            want = pillow_pixels(paths[n][0], mode)
            assert p.is_cuda and tuple(p.shape) == want.shape and np.array_equal(p.cpu().numpy(), want), (mode, n)
    assert stats == {'device': 2, 'pillow': 10}
    pics, launches = profiled(lambda: png.read_pictures([paths[n][0] for n in sorted(cases.OTHER_KINDS)], cuda, 'RGB'))
    assert launches == [] and len(pics) == 4


def test_a_broken_file_is_named(files, cuda):
    from aivc_amd import png
    tmp, paths = files
    bad = str(tmp / 'flipped-crc.png')
    with open(bad, 'wb') as f:
        f.write(cases.broken_files()['idat-crc'])
    with pytest.raises(png.PngError, match='flipped-crc.png.*CRC'):
        png.read_pictures([paths['grey-default'][0], bad], cuda, 'L')
    # a stream the device refuses: the file's CRCs are right, its zlib stream is not
    z = bytearray(dict(pcs.chunks(cases.FILES['grey-assembled'][0]))[b'IDAT'])
    z[-1] ^= 1
    wrong = str(tmp / 'wrong-adler.png')
    with open(wrong, 'wb') as f:
        f.write(png.assemble(33, 65, 1, bytes(z)))
    with pytest.raises(png.PngError, match='wrong-adler.png.*Adler'):
        png.read_pictures([paths['grey-default'][0], wrong], cuda, 'L')


def test_three_1080p_pictures_in_one_batch(cuda):
    """the only large case: an RGB picture, a luma plane and a half-size chroma plane, written by Pillow, one launch each of the two
    kernels"""
    from PIL import Image
    from aivc_amd import ops, png
    rgb = pcs.analytic_picture(1080, 1920, 3)
    ycc = np.asarray(Image.fromarray(rgb).convert('YCbCr'))
    pictures = [rgb, ycc[..., :1], ycc[::2, ::2, 1:2]]
    parsed = []
    for pix in pictures:
        buf = io.BytesIO()
        Image.fromarray(pix[..., 0] if pix.shape[2] == 1 else pix).save(buf, 'PNG')
        data = buf.getvalue()
        w, h, c, idats = png.parse(data)
        assert (h, w, c) == pix.shape
        parsed.append([data[o:o + n] for o, n in idats])
    assert len(parsed[0]) > 40  # Pillow cuts the stream into IDATs of 64 KiB
    shapes = [p.shape for p in pictures]

    def case(fill):
        filt = ops.inflate(parsed, [h * (1 + w * c) for h, w, c in shapes], cuda)
        return ops.png_unfilter(filt, shapes)
    assert three_ways(case) == [p.tobytes() for p in pictures]
