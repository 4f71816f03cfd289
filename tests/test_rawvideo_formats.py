"""aivc_amd/rawvideo.py without a GPU: the format table against known byte counts and the test suite's own table, the numpy
statement of tests/rawvideo_cases.py against Pillow's Image.reduce (its outside anchor), .y4m and file-name parsing, the command
lines' flags, and the C entry points' exports and error codes (no launch)."""
import contextlib
import ctypes
import io
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rawvideo_cases as rvc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = (1, 2, 3, 5, 9, 33, 67)


# ---- the table -------------------------------------------------------------------------------------------------------------------
def test_known_frame_sizes():
    from aivc_amd.rawvideo import PixFmt
    assert PixFmt('yuv420p10le').frame_bytes(1920, 1080) == 6220800
    assert PixFmt('nv12').frame_bytes(1920, 1080) == 3110400
    assert PixFmt('yuv444p').frame_bytes(3, 3) == 27
    assert PixFmt('yuv420p').frame_bytes(3, 3) == 17
    assert PixFmt('yuv444p10le').frame_bytes(1920, 1080) * 129 == 1604966400  # the 1.6 GB of the clip conversion is for


def test_table_is_the_suites_table():
    from aivc_amd import abi, rawvideo
    assert sorted(rawvideo.PIX_FMTS) == sorted(rvc.FORMATS)
    arrangement = {'': abi.CHROMA_NONE, 'p': abi.CHROMA_PLANAR, 'uv': abi.CHROMA_UV, 'vu': abi.CHROMA_VU}
    for name, (b, depth, top, sx, sy, arr) in rvc.FORMATS.items():
        f = rawvideo.PixFmt(name)
        assert (f.bytes_per_sample, f.depth, f.msb_aligned, f.chroma) == (b, depth, top, arrangement[arr])
        if arr:
            assert (f.shift_x, f.shift_y) == (sx, sy)
        assert f.writable == (name in rvc.WRITABLE)
        assert f.y4m_tag == rvc.Y4M_TAGS.get(name)
        for w, h, pad in ((1, 1, 0), (3, 3, 0), (5, 2, 3), (33, 9, 64), (1920, 1080, 0)):
            planes, total = rvc.planes_of(name, w, h, pad)
            offsets, pitches, nbytes = f.layout(w, h, pad)
            assert nbytes == total and offsets[:len(planes)] == [p[0] for p in planes] and pitches[:len(planes)] == [p[1] for p in planes]
            st = f.struct(w, h, offsets, pitches)
            assert (st.w, st.h, st.depth, list(st.offset), list(st.pitch)) == (w, h, depth, offsets, pitches)


def test_unknown_name_lists_the_table():
    from aivc_amd.rawvideo import PIX_FMTS, PixFmt
    with pytest.raises(ValueError) as e:
        PixFmt('yuv420p10be')
    assert all(n in str(e.value) for n in PIX_FMTS)
    for out_of_scope in ('nv16', 'yuyv422', 'rgb24', 'yuv420p9le'):
        with pytest.raises(ValueError):
            PixFmt(out_of_scope)


# ---- the numpy statement against Pillow -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', sorted(n for n, f in rvc.FORMATS.items() if f[0] == 1))
def test_numpy_ingest_is_image_reduce(name):
    """every 8-bit format, every size of SIDES x SIDES: luma is the plane, chroma is Image.reduce of the component's plane by the
    factor one 4:2:0 sample covers -- (2, 2) for 4:4:4, (1, 2) for 4:2:2 -- and the plane itself for 4:2:0"""
    from PIL import Image
    b, depth, top, sx, sy, arr = rvc.FORMATS[name]
    rng = np.random.default_rng(len(name))
    for w in SIDES:
        for h in SIDES:
            buf = rvc.make_frame(name, w, h, rng)
            y, u, v = rvc.ingest(buf, name, w, h)
            planes, _ = rvc.planes_of(name, w, h)

            def plane(p, first=0, step=1):
                off, pitch, rows, cols = p
                return np.ascontiguousarray(buf[off:off + rows * cols].reshape(rows, cols)[:, first::step])
            assert np.array_equal(y, plane(planes[0]))
            if arr == '':
                assert (u == 128).all() and (v == 128).all() and u.shape == ((h + 1) // 2, (w + 1) // 2)
                continue
            if arr == 'p':
                cu, cv = plane(planes[1]), plane(planes[2])
            else:
                cu, cv = plane(planes[1], arr == 'vu', 2), plane(planes[1], arr == 'uv', 2)
            factor = (2 >> sx, 2 >> sy)
            for got, src in ((u, cu), (v, cv)):
                want = src if factor == (1, 1) else np.asarray(Image.fromarray(src, 'L').reduce(factor))
                assert np.array_equal(got, want), (name, w, h)


def test_numpy_reduce_of_horizontal_pairs_is_pillow_too():
    """(2, 1), the factor no layout of the table has: the rule itself (edge-repeating sum, + t / 2) against Pillow"""
    from PIL import Image
    rng = np.random.default_rng(3)
    for w in SIDES:
        for h in SIDES:
            src = rng.integers(0, 256, (h, w), dtype=np.uint8)
            cols = np.minimum(2 * np.arange((w + 1) // 2)[:, None] + np.arange(2)[None, :], w - 1)
            got = ((src.astype(np.int64)[:, cols].sum(2) + 1) >> 1).astype(np.uint8)
            assert np.array_equal(got, np.asarray(Image.fromarray(src, 'L').reduce((2, 1))))


def test_export_then_ingest_is_the_identity_in_numpy():
    rng = np.random.default_rng(1)
    for name in rvc.WRITABLE:
        for w, h in ((1, 1), (3, 3), (16, 2), (33, 5)):
            y = rng.integers(0, 256, (h, w), dtype=np.uint8)
            u, v = (rng.integers(0, 256, ((h + 1) // 2, (w + 1) // 2), dtype=np.uint8) for _ in 'uv')
            buf = rvc.export(y, u, v, name)
            assert buf.size == rvc.frame_bytes(name, w, h)
            y2, u2, v2 = rvc.ingest(buf, name, w, h)
            assert np.array_equal(y, y2)
            if rvc.FORMATS[name][5]:
                assert np.array_equal(u, u2) and np.array_equal(v, v2)


# ---- .y4m ---------------------------------------------------------------------------------------------------------------------------
def _clip(tmp_path, name, w=6, h=4, n=3, file='clip.y4m', **kw):
    rng = np.random.default_rng(n)
    frames = [rvc.make_frame(name, w, h, rng) for _ in range(n)]
    return rvc.write_y4m(str(tmp_path / file), name, w, h, frames, **kw), frames


@pytest.mark.parametrize('tag,name', [('420', 'yuv420p'), ('420jpeg', 'yuv420p'), ('420mpeg2', 'yuv420p'), ('420paldv', 'yuv420p'),
                                      ('422', 'yuv422p'), ('444', 'yuv444p'), ('mono', 'gray'), ('', 'yuv420p'),
                                      ('420p10', 'yuv420p10le'), ('420p12', 'yuv420p12le'), ('420p16', 'yuv420p16le'),
                                      ('422p10', 'yuv422p10le'), ('422p12', 'yuv422p12le'), ('422p16', 'yuv422p16le'),
                                      ('444p10', 'yuv444p10le'), ('444p12', 'yuv444p12le'), ('444p16', 'yuv444p16le'),
                                      ('monop10', 'gray10le'), ('mono12', 'gray12le'), ('monop16', 'gray16le')])
def test_y4m_accepted_tags(tag, name, tmp_path):
    from aivc_amd import rawvideo
    path, frames = _clip(tmp_path, name, tag=tag, fps=(30000, 1001), header_extra=' XYSCSS=whatever')
    rd = rawvideo.open_raw(path)
    assert (rd.pix_fmt.name, rd.w, rd.h, rd.fps, rd.n_frames) == (name, 6, 4, (30000, 1001), 3)
    assert rd.frame_bytes == frames[0].size
    data = open(path, 'rb').read()
    for off, fr in zip(rd.offsets, frames):
        assert data[off:off + fr.size] == fr.tobytes() and data[off - 6:off] == b'FRAME\n'
    rd.close()


@pytest.mark.parametrize('interlace', ['Ip', 'I?', ''])
def test_y4m_progressive_markers(interlace, tmp_path):
    from aivc_amd import rawvideo
    path, _ = _clip(tmp_path, 'yuv420p', interlace=interlace)
    assert rawvideo.open_raw(path).n_frames == 3


def test_y4m_frame_lines_with_parameters_are_walked(tmp_path):
    from aivc_amd import rawvideo
    path, frames = _clip(tmp_path, 'yuv422p10le', n=4, frame_params=' Ip XFOO=1')
    rd = rawvideo.open_raw(path)
    data = open(path, 'rb').read()
    assert rd.n_frames == 4
    for i, (off, fr) in enumerate(zip(rd.offsets, frames)):
        assert data[off:off + fr.size] == fr.tobytes()
        rd._check_frame_line(i)
    assert rd.offsets[1] - rd.offsets[0] == frames[0].size + len(b'FRAME Ip XFOO=1\n')


@pytest.mark.parametrize('interlace', ['It', 'Ib', 'Im'])
def test_y4m_interlaced_is_refused_by_name(interlace, tmp_path):
    from aivc_amd import rawvideo
    path, _ = _clip(tmp_path, 'yuv420p', interlace=interlace)
    with pytest.raises(rawvideo.RawVideoError) as e:
        rawvideo.open_raw(path)
    assert interlace in str(e.value)


@pytest.mark.parametrize('tag', ['411', '420p9', '444alpha', '420p14'])
def test_y4m_unknown_colour_space_is_refused_by_name(tag, tmp_path):
    from aivc_amd import rawvideo
    path, _ = _clip(tmp_path, 'yuv420p', tag=tag)
    with pytest.raises(rawvideo.RawVideoError) as e:
        rawvideo.open_raw(path)
    assert 'C' + tag in str(e.value)


def test_y4m_other_refusals(tmp_path):
    from aivc_amd import rawvideo
    bad = tmp_path / 'bad.y4m'
    bad.write_bytes(b'RIFF....AVI LIST\n' + b'\0' * 64)
    with pytest.raises(rawvideo.RawVideoError):
        rawvideo.open_raw(str(bad))
    path, frames = _clip(tmp_path, 'yuv420p', n=3)
    data = bytearray(open(path, 'rb').read())
    at = data.index(b'FRAME', data.index(b'FRAME') + 1)
    data[at:at + 5] = b'FRAMF'  # frame 1's line is damaged: counted by the walk, refused when it is read
    (tmp_path / 'damaged.y4m').write_bytes(bytes(data))
    rd = rawvideo.open_raw(str(tmp_path / 'damaged.y4m'))
    rd._check_frame_line(0)
    with pytest.raises(rawvideo.RawVideoError) as e:
        rd._check_frame_line(1)
    assert 'frame 1' in str(e.value)


def test_y4m_truncated_last_frame_is_not_counted(tmp_path):
    from aivc_amd import rawvideo
    path, frames = _clip(tmp_path, 'yuv444p12le', n=3)
    data = open(path, 'rb').read()
    for cut in (1, frames[0].size - 1, frames[0].size, frames[0].size + 3):
        (tmp_path / 'cut.y4m').write_bytes(data[:-cut])
        assert rawvideo.open_raw(str(tmp_path / 'cut.y4m')).n_frames == 2
    (tmp_path / 'cut.y4m').write_bytes(data[:-(frames[0].size + 6)])
    assert rawvideo.open_raw(str(tmp_path / 'cut.y4m')).n_frames == 2


def test_request_past_the_end_names_the_range(tmp_path):
    """encode.py: `[ERROR]` with the file's range and exit status 2, like a partial decode's request outside the stream -- before
    a device is looked for, so it is the same with and without a GPU"""
    from aivc_amd import encode as enc_cli
    from aivc_amd import rawvideo
    path, _ = _clip(tmp_path, 'yuv420p10le', n=3)
    rd = rawvideo.open_raw(path)
    assert rd.frame_range(0, -1) == (0, 2) and rd.frame_range(1, 2) == (1, 2)
    for first, last in ((0, 3), (3, -1), (2, 1), (-1, 1)):
        with pytest.raises(rawvideo.RawVideoError) as e:
            rd.frame_range(first, last)
        assert '0 ... 2' in str(e.value)
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit) as e:
        enc_cli.main(['-i', path, '-o', str(tmp_path / 'x.bin'), '--end_frame', '7'])
    assert e.value.code == 2
    assert '[ERROR]' in buf.getvalue() and '0 ... 2' in buf.getvalue() and not os.path.exists(tmp_path / 'x.bin')
    raw = tmp_path / 'clip_6x4_25_420_10b.yuv'
    raw.write_bytes(b'\0' * (36 * 2 * 2 + 5))  # two frames and a truncated one
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit) as e:
        enc_cli.main(['-i', str(raw), '-o', str(tmp_path / 'x.bin'), '--start_frame', '2'])
    assert e.value.code == 2 and '0 ... 1' in buf.getvalue()


# ---- headerless names -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('file,name', [('BQMall_832x480_60_420.yuv', 'yuv420p'), ('clip_64x48_30.yuv', 'yuv420p'),
                                       ('Beauty_1920x1080_120fps_420_10bit_YUV.yuv', 'yuv420p10le'),
                                       ('clip_64x48_30_444_10b.yuv', 'yuv444p10le'), ('clip_64x48_422.yuv', 'yuv422p'),
                                       ('a_8x8_420_12b.yuv', 'yuv420p12le'), ('a_8x8_16bit_444.yuv', 'yuv444p16le'),
                                       ('a_8x8_8bit.yuv', 'yuv420p'), ('a_8x8_25_422_16b.raw', 'yuv422p16le')])
def test_headerless_names(file, name, tmp_path):
    from aivc_amd import rawvideo
    assert rawvideo.pix_fmt_from_name('/some/dir/' + file).name == name
    w, h = rawvideo.parse_size_name(file)
    path = tmp_path / file
    path.write_bytes(b'\0' * (rvc.frame_bytes(name, w, h) * 2 + 1))
    rd = rawvideo.open_raw(str(path))
    assert (rd.w, rd.h, rd.fps, rd.n_frames, rd.pix_fmt.name) == (w, h, None, 2, name)
    # the reader's one predicate (whether read_yuv announces a conversion), where needs_conversion(name, pix_fmt) was asked
    assert (not rd.is_plain) == (name != 'yuv420p')
    y4m, _ = _clip(tmp_path, 'yuv420p', file='x.y4m')
    assert not rawvideo.open_raw(str(path), 'nv12').is_plain and not rawvideo.open_raw(y4m).is_plain
    rd = rawvideo.open_raw(str(path), 'gray', (2, 2))  # pix_fmt and size given: the name is not consulted
    assert (rd.w, rd.h, rd.pix_fmt.name, rd.n_frames) == (2, 2, 'gray', (rvc.frame_bytes(name, w, h) * 2 + 1) // 4)
    with pytest.raises(rawvideo.RawVideoError):
        rawvideo.parse_size_name('nosize_420.yuv')


def test_plain_files_go_through_the_one_reader(tmp_path):
    """a plain *_420.yuv is a file of the reader like any other: frames back to back, a truncated tail not counted, a request
    outside it refused with its range -- by encode.py with exit status 2 before a device is looked for, as for a .y4m.  (That the
    planes are the file's bytes is tests/test_gpu_rawvideo.py::test_plain_file_planes_are_the_files_bytes.)"""
    from aivc_amd import encode as enc_cli
    from aivc_amd import rawvideo
    for w, h in ((4, 2), (5, 3), (1, 1)):
        fb = w * h + 2 * ((w + 1) // 2) * ((h + 1) // 2)
        path = tmp_path / ('clip_%dx%d_25_420.yuv' % (w, h))
        for tail in (0, 1, fb - 1):
            path.write_bytes(b'\1' * (3 * fb + tail))
            with rawvideo.open_raw(str(path)) as rd:
                assert rd.is_plain and (rd.w, rd.h, rd.frame_bytes, rd.n_frames) == (w, h, fb, 3)
                assert rd.offsets == [i * fb for i in range(3)]
                assert rd.frame_range(0, -1) == (0, 2) and rd.frame_range(1, 2) == (1, 2)
                for first, last in ((0, 3), (3, -1), (2, 1), (-1, 1)):
                    with pytest.raises(rawvideo.RawVideoError) as e:
                        rd.frame_range(first, last)
                    assert '0 ... 2' in str(e.value)
    path = tmp_path / 'clip_4x2_25_420.yuv'
    path.write_bytes(b'\0' * (12 * 2 + 5))  # two frames and a truncated one
    buf = io.StringIO()
    with contextlib.redirect_stdout(buf), pytest.raises(SystemExit) as e:
        enc_cli.main(['-i', str(path), '-o', str(tmp_path / 'x.bin'), '--start_frame', '2'])
    assert e.value.code == 2 and '[ERROR]' in buf.getvalue() and '0 ... 1' in buf.getvalue() and not os.path.exists(tmp_path / 'x.bin')


# ---- flags --------------------------------------------------------------------------------------------------------------------------
def _error(parse, argv):
    err = io.StringIO()
    with contextlib.redirect_stderr(err), pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    return err.getvalue()


def test_flags():
    from aivc_amd import aivc, decode, encode
    assert encode.parse_args([]).pix_fmt is None and encode.parse_args(['--pix_fmt', 'p010le']).pix_fmt == 'p010le'
    assert 'yuv420p10be' in _error(encode.parse_args, ['--pix_fmt', 'yuv420p10be'])
    a = decode.parse_args([])
    assert (a.out_pix_fmt, a.fps) == ('yuv420p', (25, 1))
    a = decode.parse_args(['-o', 'out.y4m', '--out_pix_fmt', 'yuv420p10le', '--fps', '30000:1001'])
    assert (a.out_pix_fmt, a.fps) == ('yuv420p10le', (30000, 1001))
    assert decode.parse_args(['--fps', '50']).fps == (50, 1)
    assert decode.parse_args(['-o', 'out_8x8.yuv', '--out_pix_fmt', 'nv12']).out_pix_fmt == 'nv12'
    for bad in ('yuv444p', 'yuv422p10le', 'rgb24'):  # 4:2:0 and grey layouts only
        _error(decode.parse_args, ['--out_pix_fmt', bad])
    for fmt in ('nv12', 'nv21', 'p010le', 'p016le'):  # no .y4m tag
        assert '.y4m' in _error(decode.parse_args, ['-o', 'out.y4m', '--out_pix_fmt', fmt])
    for bad in ('0', '25:0', 'fast', '25:1:1'):
        _error(decode.parse_args, ['--fps', bad])
    assert 'no frame rate' in decode_help()
    a = aivc.parse_args(['-i', 'clip.y4m', '-o', 'out.y4m', '--out_pix_fmt', 'gray10le', '--fps', '24', '--pix_fmt', 'yuv444p'])
    assert (a.pix_fmt, a.out_pix_fmt, a.fps) == ('yuv444p', 'gray10le', (24, 1))
    _error(aivc.parse_args, ['-o', 'out.y4m', '--out_pix_fmt', 'p010le'])


def decode_help():
    from aivc_amd import decode
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit):
        decode.parse_args(['-h'])
    return ' '.join(out.getvalue().split())


def test_evaluate_flags(monkeypatch):
    from aivc_amd import evaluate
    seen = {}
    monkeypatch.setattr(evaluate, 'evaluate_yuv', lambda *a: seen.update(args=a) or {'PSNR': 1.0, 'MSSSIM': 1.0, 'MSSSIM_dB': 1.0})
    with contextlib.redirect_stdout(io.StringIO()):
        evaluate.main(['--raw', 'a_8x8_444_10b.yuv', '--compressed', 'out.y4m', '--pix_fmt', 'yuv444p10le',
                       '--compressed_pix_fmt', 'nv12', '--start_frame', '2', '--bitstream', '/nonexistent'])
    assert seen['args'] == ('a_8x8_444_10b.yuv', 'out.y4m', 2, 'yuv444p10le', 'nv12')
    with contextlib.redirect_stdout(io.StringIO()):
        evaluate.main(['--raw', 'a_8x8_420.yuv', '--compressed', 'out', '--bitstream', '/nonexistent'])
    assert seen['args'] == ('a_8x8_420.yuv', 'out.yuv', 0, None, None)


def test_writer_refusals(tmp_path):
    from aivc_amd import rawvideo
    for fmt in ('nv12', 'nv21', 'p010le', 'p016le'):
        with pytest.raises(ValueError) as e:
            rawvideo.check_writable(fmt, 'out.y4m')
        assert fmt in str(e.value) and '.y4m' in str(e.value)
        assert rawvideo.check_writable(fmt, 'out.yuv').name == fmt
    for fmt in ('yuv422p', 'yuv444p16le'):
        with pytest.raises(ValueError):
            rawvideo.check_writable(fmt, 'out.yuv')


# ---- the C entry points, no launch ---------------------------------------------------------------------------------------------------
def test_library_exports_and_abi():
    from aivc_amd import abi
    assert abi.ABI_VERSION == 26 and set(abi.RAWVIDEO_PROTOTYPES) == {'aivc_rawvideo_to_yuv420u8', 'aivc_yuv420u8_to_rawvideo'}
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    for name in abi.RAWVIDEO_PROTOTYPES:
        assert hasattr(lib, name), 'libaivc_hip.so does not export %s' % name
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == 26
    assert '#define AIVC_ABI_VERSION 26\n' in open(os.path.join(ROOT, 'include', 'aivc_hip.h')).read()
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_rawvideo.h')).read()
    assert all('int %s(' % name in header for name in abi.RAWVIDEO_PROTOTYPES)
    assert ctypes.sizeof(abi.RawVideoFmt) == 8 * 4 + 6 * 8
    from aivc_amd import _lib
    fns = _lib.load()  # the loader binds them beside what abi.declare binds, each with its stream argument
    for name, args in abi.RAWVIDEO_PROTOTYPES.items():
        assert fns[name].argtypes == list(args) + [ctypes.c_void_p] and fns[name].restype is ctypes.c_int


def _codes(st, n=1, ptrs=(1, 1, 1, 1)):
    """(ingest's code, export's code) for a call that must not launch; 1 stands for any non-NULL pointer"""
    from aivc_amd import _lib
    fns = _lib.load()
    frames, y, u, v = ptrs
    ref = None if st is None else ctypes.byref(st)
    return (fns['aivc_rawvideo_to_yuv420u8'](frames, n, ref, y, u, v, None), fns['aivc_yuv420u8_to_rawvideo'](y, u, v, n, ref, frames, None))


def test_error_codes_without_a_gpu():
    from aivc_amd import abi, rawvideo
    ARG, UNSUPPORTED = -1, abi.ERR_UNSUPPORTED

    def fmt(name='yuv420p10le', w=16, h=8, **change):
        st = rawvideo.PixFmt(name).struct(w, h)
        for k, val in change.items():
            if k in ('offset', 'pitch'):
                arr = list(getattr(st, k))
                arr[val[0]] = val[1]
                setattr(st, k, (ctypes.c_int64 * 3)(*arr))
            else:
                setattr(st, k, val)
        return st
    assert _codes(fmt(), n=0) == (0, 0) and _codes(None, n=0, ptrs=(None,) * 4) == (0, 0)  # n == 0: nothing is done
    assert _codes(fmt(), n=-1) == (ARG, ARG)
    for k in range(4):  # a NULL pointer with n > 0
        ptrs = tuple(None if i == k else 1 for i in range(4))
        assert _codes(fmt(), ptrs=ptrs) == (ARG, ARG)
    assert _codes(None) == (ARG, ARG)
    for change in ({'w': 0}, {'h': 0}, {'w': -3}, {'depth': 7}, {'depth': 17}, {'bytes_per_sample': 3}, {'bytes_per_sample': 0},
                   {'chroma': 4}, {'chroma': -1}, {'msb_aligned': 2}, {'shift_x': 2}, {'shift_y': -1},
                   {'pitch': (0, 31)}, {'pitch': (1, 15)}, {'pitch': (2, 0)}, {'offset': (1, -1)}):
        assert _codes(fmt(**change)) == (ARG, ARG), change
    assert _codes(fmt('yuv420p', depth=10)) == (ARG, ARG)  # depth > 8 with one byte per sample
    assert _codes(fmt('nv12', pitch=(1, 15))) == (ARG, ARG)  # the interleaved plane's tight row is 2 x 8 bytes
    # a frame of 2^31 bytes or more
    assert _codes(fmt('gray', 65536, 32768)) == (UNSUPPORTED, UNSUPPORTED)
    assert _codes(fmt('yuv444p16le', 32768, 16384)) == (UNSUPPORTED, UNSUPPORTED)
    assert _codes(fmt('gray', 16, 8, pitch=(0, 1 << 31))) == (UNSUPPORTED, UNSUPPORTED)
    assert _codes(fmt('nv12', shift_x=0, pitch=(1, 32))) == (UNSUPPORTED, UNSUPPORTED)  # interleaved 4:4:4 (NV24): no kernel
    # export covers 4:2:0 and grey layouts only; the same struct is an ingest that would launch, so only export is called
    from aivc_amd import _lib
    for name in ('yuv422p', 'yuv444p10le'):
        st = fmt(name)
        assert _lib.load()['aivc_yuv420u8_to_rawvideo'](1, 1, 1, 1, ctypes.byref(st), 1, None) == UNSUPPORTED
