"""aivc_rawvideo_to_yuv420u8 / aivc_yuv420u8_to_rawvideo (include/aivc_hip_rawvideo.h) through aivc_amd.ops and the file reader,
against the numpy statement of tests/rawvideo_cases.py: every format of the table, bytes compared with ==, no tolerance.  Each
case runs plain and under the guard-zone and poison harness of tests/guarded.py with both fills: the blob of frames between
guard zones, and every buffer aivc_amd.ops allocates -- pointer table, planes, exported frames -- an arena whose untouched
payload is poison; the three runs must agree byte for byte.

Sizes.  A lane owns one aligned 16-byte chunk of an output row, so w in {1, 2, 15, 16, 17, 63, 65, 257} puts rows below, at and
above one chunk, across a wavefront's 64 lanes' worth of chunks for 8-bit luma (257 = 16 chunks + 1 byte; chroma 129), with odd
widths for the repeated edge column; h in {1, 2, 3, 5} gives one row, the repeated edge row and several rows whose starts fall on
different alignments (rows of a stack are back to back).  Three frames lie in one blob at byte offsets 0, 1 and 7 past multiples
of the frame size: 16-bit samples at odd addresses and another alignment per frame."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rawvideo_cases as rvc  # noqa: E402
from guarded import FILLS, both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

WIDTHS, HEIGHTS = (1, 2, 15, 16, 17, 63, 65, 257), (1, 2, 3, 5)
GAPS = (0, 1, 7)
_CACHE = {}


def clip(name, w, h, pad=0):
    """three frames of the layout in one blob, frame k at k * (frame bytes) + the sum of GAPS[:k + 1] -> (blob, offsets, the numpy
    planes [(y, u, v)] per frame); computed once per (format, size, pad) and left unchanged"""
    key = (name, w, h, pad)
    if key not in _CACHE:
        rng = np.random.default_rng([w, h, pad] + [ord(c) for c in name])
        frames = [rvc.make_frame(name, w, h, rng, pad) for _ in GAPS]
        parts, offsets, at = [], [], 0
        for gap, fr in zip(GAPS, frames):
            parts.append(rng.integers(0, 256, gap, dtype=np.uint8))
            at += gap
            offsets.append(at)
            parts.append(fr)
            at += fr.size
        blob = np.concatenate(parts)
        blob.setflags(write=False)
        _CACHE[key] = (blob, offsets, [rvc.ingest(fr, name, w, h, pad) for fr in frames])
    return _CACHE[key]


def layout_of(name, w, h, pad):
    planes, total = rvc.planes_of(name, w, h, pad)
    return ([p[0] for p in planes] + [0] * (3 - len(planes)), [p[1] for p in planes] + [0] * (3 - len(planes)), total)


def ingest_both_ways(name, w, h, cuda, pad=0):
    """ops.raw_to_yuv420u8 on clip(...): plain, then under guard_ops with both fills -> the plain (y, u, v) as numpy arrays"""
    from aivc_amd import ops
    blob, offsets, _ = clip(name, w, h, pad)

    def call(fill):
        dev = torch.from_numpy(blob.copy()).to(cuda) if fill is None else guarded(blob.copy(), cuda, fill)
        return list(ops.raw_to_yuv420u8(dev, offsets, name, w, h, layout_of(name, w, h, pad) if pad else None))
    plain = [t.cpu().numpy() for t in call(None)]
    assert both_fills(call) == [a.tobytes() for a in plain]
    return plain


def assert_planes(got, want, what):
    for k, c in enumerate('yuv'):
        for f in range(len(want)):
            assert got[k][f].shape == want[f][k].shape, (what, c, f)
            assert np.array_equal(got[k][f], want[f][k]), (what, c, f, np.argwhere(got[k][f] != want[f][k])[:4].tolist())


@pytest.mark.parametrize('name', sorted(rvc.FORMATS))
def test_ingest_every_format_and_size(name, cuda):
    for w in WIDTHS:
        for h in HEIGHTS:
            got = ingest_both_ways(name, w, h, cuda)
            assert_planes(got, clip(name, w, h)[2], (name, w, h))


@pytest.mark.parametrize('name', ['gray12le', 'yuv420p', 'yuv422p10le', 'yuv444p16le', 'nv12', 'nv21', 'p010le'])
@pytest.mark.parametrize('pad', [3, 64])
def test_ingest_pitched_rows(name, pad, cuda):
    """one layout per arrangement with rows of tight + 3 and tight + 64 bytes; the bytes behind a tight row are random"""
    for w, h in ((17, 5), (65, 3), (2, 2)):
        got = ingest_both_ways(name, w, h, cuda, pad)
        assert_planes(got, clip(name, w, h, pad)[2], (name, w, h, pad))


@pytest.mark.parametrize('lead', [b'', b'FRAME\n'])
@pytest.mark.parametrize('name', rvc.WRITABLE)
def test_export_and_back(name, lead, cuda):
    """export against numpy, tight frames and frames behind a 6-byte lead (odd addresses for 16-bit words), and export followed by
    ingest equal to the input"""
    from aivc_amd import ops
    grey = rvc.FORMATS[name][5] == ''
    for w in WIDTHS:
        for h in HEIGHTS:
            rng = np.random.default_rng([w, h, 77])
            hc, wc = (h + 1) // 2, (w + 1) // 2
            y, u, v = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((3, h, w), (3, hc, wc), (3, hc, wc)))
            y[0].reshape(-1)[:2] = (0, 255)[:y[0].size]
            want = [rvc.export(y[f], u[f], v[f], name) for f in range(3)]
            if True:
                def call(fill):
                    put = (lambda a: torch.from_numpy(a).to(cuda)) if fill is None else (lambda a: guarded(a, cuda, fill))
                    out = ops.yuv420u8_to_raw(put(y), put(u), put(v), name, lead)
                    back = ops.raw_to_yuv420u8(out, [len(lead) + f * out.shape[1] for f in range(3)], name, w, h)
                    return [out] + list(back)
                res = [t.cpu().numpy() for t in call(None)]
                assert both_fills(call) == [a.tobytes() for a in res]
                out = res[0]
                assert out.shape == (3, len(lead) + want[0].size)
                for f in range(3):
                    assert out[f, :len(lead)].tobytes() == lead
                    assert np.array_equal(out[f, len(lead):], want[f]), (name, w, h, lead, f)
                assert np.array_equal(res[1], y)
                if grey:
                    assert (res[2] == 128).all() and (res[3] == 128).all()
                else:
                    assert np.array_equal(res[2], u) and np.array_equal(res[3], v)


def test_nothing_is_written_for_no_frames(cuda):
    from aivc_amd import _lib, abi, ops, rawvideo
    import ctypes
    fns = _lib.load()
    st = rawvideo.PixFmt('yuv420p10le').struct(16, 4)
    for fill in FILLS:
        bufs = [guarded(np.full(256, fill, np.uint8), cuda, fill) for _ in range(4)]
        a, b, c, d = (t.data_ptr() for t in bufs)
        assert fns['aivc_rawvideo_to_yuv420u8'](a, 0, ctypes.byref(st), b, c, d, ops._stream()) == abi.AIVC_OK
        assert fns['aivc_yuv420u8_to_rawvideo'](b, c, d, 0, ctypes.byref(st), a, ops._stream()) == abi.AIVC_OK
        torch.cuda.synchronize()
        assert all(bool((t == fill).all()) for t in bufs)
        from guarded import check_guards
        check_guards(*bufs)
    y, u, v = ops.raw_to_yuv420u8(torch.zeros(8, dtype=torch.uint8, device=cuda), [], 'nv12', 4, 2)
    assert tuple(y.shape) == (0, 2, 4) and tuple(u.shape) == (0, 1, 2) and tuple(v.shape) == (0, 1, 2)


def test_ops_rejections(cuda):
    from aivc_amd import ops
    blob = torch.zeros(100, dtype=torch.uint8, device=cuda)
    with pytest.raises(ValueError):
        ops.raw_to_yuv420u8(blob, [0], 'yuv420p9', 4, 4)  # unknown name: the message lists the table
    with pytest.raises(ValueError):
        ops.raw_to_yuv420u8(blob, [90], 'yuv420p', 4, 4)  # 24 bytes from offset 90: outside the blob
    with pytest.raises(ValueError):
        ops.yuv420u8_to_raw(torch.zeros(1, 4, 4, dtype=torch.uint8, device=cuda), blob[:4].reshape(1, 2, 2), blob[:4].reshape(1, 2, 2),
                            'yuv444p')  # not written


# ---- the file reader -------------------------------------------------------------------------------------------------------------
def _y4m(tmp_path, name, w, h, n, file='clip.y4m', **kw):
    rng = np.random.default_rng(n)
    frames = [rvc.make_frame(name, w, h, rng) for _ in range(n)]
    path = rvc.write_y4m(str(tmp_path / file), name, w, h, frames, **kw)
    return path, frames


def test_reader_y4m_frames_at_odd_bytes(tmp_path, cuda):
    """the header length decides where frame 0 starts: five characters more move it from an even byte to an odd one or back; a
    FRAME line with parameters moves every frame again"""
    from aivc_amd import rawvideo
    name, w, h = 'yuv444p10le', 33, 5
    parities = set()
    for k, (extra, params) in enumerate((('', ''), (' XODD', ''), ('', ' Ip'))):
        path, frames = _y4m(tmp_path, name, w, h, 4, 'clip%d.y4m' % k, header_extra=extra, frame_params=params)
        rd = rawvideo.open_raw(path)
        assert rd.offsets[0] == open(path, 'rb').read().index(b'\n') + 1 + 6 + len(params)
        parities.add((rd.offsets[0] % 2, rd.offsets[1] % 2))
        assert (rd.w, rd.h, rd.fps, rd.n_frames, rd.pix_fmt.name) == (w, h, (30, 1), 4, name)
        got = rd.read(1, 3, cuda)
        rd.close()
        assert len(got) == 3
        for fr, raw in zip(got, frames[1:]):
            want = rvc.ingest(raw, name, w, h)
            assert all(fr[c].shape[0] == 1 and fr[c].is_cuda and np.array_equal(fr[c][0].cpu().numpy(), want[i])
                       for i, c in enumerate('yuv'))
    assert {p[0] for p in parities} == {0, 1}  # (frame bytes are even here, so every frame of a file shares frame 0's parity)


def test_reader_spans_two_batches(tmp_path, cuda, monkeypatch):
    """BATCH_BYTES shrunk to two and a half frames: five frames arrive in three copies and three launches, same planes"""
    from aivc_amd import ops, rawvideo
    name, w, h = 'p010le', 18, 6
    rng = np.random.default_rng(5)
    frames = [rvc.make_frame(name, w, h, rng) for _ in range(5)]
    path = str(tmp_path / 'clip_18x6_25.yuv')
    np.concatenate(frames).tofile(path)
    monkeypatch.setattr(rawvideo, 'BATCH_BYTES', frames[0].size * 5 // 2)
    calls = []
    real = ops.raw_to_yuv420u8
    monkeypatch.setattr(ops, 'raw_to_yuv420u8', lambda *a, **k: calls.append(len(a[1])) or real(*a, **k))
    rd = rawvideo.open_raw(path, 'p010le')
    got = rd.read(0, -1, cuda)
    assert calls == [2, 2, 1] and len(got) == 5
    for fr, raw in zip(got, frames):
        want = rvc.ingest(raw, name, w, h)
        assert all(np.array_equal(fr[k][0].cpu().numpy(), want[i]) for i, k in enumerate('yuv'))


@pytest.mark.parametrize('w,h', [(1, 1), (5, 3), (17, 5), (257, 2)])
def test_plain_file_planes_are_the_files_bytes(w, h, tmp_path, cuda, capsys):
    """a headerless planar 8-bit 4:2:0 file through read_yuv -- the one reader -- and back through write_raw -- the one writer:
    the planes are numpy's slices of the file, the file written from them is the file.  5 x 3: 27-byte frames, so odd frame
    starts, odd sides, ceil-sized chroma; 17 and 257: a row one byte past one and sixteen 16-byte chunks; 1 x 1: the smallest"""
    from aivc_amd import rawvideo
    from aivc_amd.real_life.encode import read_yuv
    hc, wc = (h + 1) // 2, (w + 1) // 2
    data = np.random.default_rng([w, h]).integers(0, 256, (3, h * w + 2 * hc * wc), dtype=np.uint8)
    path = str(tmp_path / ('clip_%dx%d_25_420.yuv' % (w, h)))
    data.tofile(path)
    want = [{'y': fr[:h * w].reshape(1, h, w), 'u': fr[h * w:h * w + hc * wc].reshape(1, hc, wc),
             'v': fr[h * w + hc * wc:].reshape(1, hc, wc)} for fr in data]
    for (first, last), span in (((0, -1), (0, 2)), ((1, 2), (1, 2))):
        frames, a, b = read_yuv(path, first, last, cuda)
        assert (a, b) == span and len(frames) == b - a + 1
        for fr, ref in zip(frames, want[a:]):
            for k in 'yuv':
                assert fr[k].is_cuda and fr[k].dtype == torch.uint8 and tuple(fr[k].shape) == ref[k].shape
                assert np.array_equal(fr[k].cpu().numpy(), ref[k]), (w, h, first, k)
        assert both_fills(lambda fill: read_yuv(path, first, last, cuda)[0]) == [{k: ref[k].tobytes() for k in 'yuv'} for ref in want[a:]]
        out = str(tmp_path / 'back.yuv')
        rawvideo.write_raw(frames, out, 'yuv420p')
        assert open(out, 'rb').read() == data[a:].tobytes()
    assert '[INFO] input:' not in capsys.readouterr().out


def test_write_raw_y4m_reads_back(tmp_path, cuda):
    from aivc_amd import rawvideo
    rng = np.random.default_rng(9)
    w, h = 21, 7
    planes = [{'y': rng.integers(0, 256, (1, h, w), dtype=np.uint8), 'u': rng.integers(0, 256, (1, 4, 11), dtype=np.uint8),
               'v': rng.integers(0, 256, (1, 4, 11), dtype=np.uint8)} for _ in range(3)]
    path = str(tmp_path / 'out.y4m')
    rawvideo.write_raw([{k: torch.from_numpy(v).to(cuda) for k, v in fr.items()} for fr in planes], path, 'yuv420p12le', (24, 1), cuda)
    toks, name, w2, h2, frames = rvc.read_y4m(path)
    assert (name, w2, h2) == ('yuv420p12le', w, h) and 'F24:1' in toks and 'C420p12' in toks and len(frames) == 3
    for fr, raw in zip(planes, frames):
        assert np.array_equal(raw, rvc.export(fr['y'][0], fr['u'][0], fr['v'][0], 'yuv420p12le'))
    with pytest.raises(ValueError):
        rawvideo.write_raw([], str(tmp_path / 'x.y4m'), 'nv12')
