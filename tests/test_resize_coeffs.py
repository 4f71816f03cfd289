"""The resize contract without a GPU: the numpy statement of tests/resize_cases.py equals Pillow's Image.resize on every shape and
filter, the host tables of aivc_amd/resize.py (and their device layout) equal the statement's, the C entry rejects what its
header says, and the command lines parse --size / --out_size / --resample.  Every comparison is equality."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resize_cases as rc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AXES = sorted({(s[1], s[3]) for s in rc.SHAPES} | {(s[0], s[2]) for s in rc.SHAPES} | {(2160, 1080), (1920, 3840), (48, 32), (96, 64)})


def test_the_eleven_shapes():
    assert len(rc.SHAPES) == 11 and len(rc.FILTER_NAMES) == 5
    from aivc_amd import resize
    assert list(resize.FILTERS) == rc.FILTER_NAMES and resize.DEFAULT_FILTER == 'bicubic'
    assert [resize.FILTERS[f][0] for f in rc.FILTER_NAMES] == [rc.STATEMENT_FILTERS[f][0] for f in rc.FILTER_NAMES]


@pytest.mark.parametrize('name', rc.FILTER_NAMES)
@pytest.mark.parametrize('shape', rc.SHAPES, ids=rc.shape_id)
def test_statement_equals_pillow(shape, name):
    for plane, want in zip(rc.planes(shape, 2), rc.pil_planes(shape, 2, name)):
        got = rc.statement_resize(plane, shape[2], shape[3], name)
        assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want)


def test_the_extremes_case_clips_both_ways():
    """{0, 255} content under the filters with negative lobes: sums below 0 and above 255 occur, so both clips are exercised"""
    shape = rc.SHAPES[6]
    assert shape[4] == 'extremes' and set(np.unique(rc.planes(shape, 1)[0])) == {0, 255}
    plane = rc.planes(shape, 1)[0].astype(np.int64)
    for name in ('bicubic', 'lanczos'):
        lo = hi = False
        for xx, (xmin, K) in enumerate(rc.statement_axis(shape[1], shape[3], name)):
            acc = (plane[:, xmin:xmin + len(K)] * np.asarray(K)).sum(-1) + (1 << 21)
            lo, hi = lo or bool((acc >> 22 < 0).any()), hi or bool((acc >> 22 > 255).any())
        assert lo and hi, name


@pytest.mark.parametrize('name', rc.FILTER_NAMES)
def test_host_tables_equal_the_statement(name):
    from aivc_amd import resize
    for n_in, n_out in AXES:
        bounds, coeffs = resize.axis_tables(n_in, n_out, name)
        rows = rc.statement_axis(n_in, n_out, name)
        assert bounds.dtype == np.int32 and coeffs.dtype == np.int32 and bounds.shape == (n_out, 2)
        assert coeffs.shape == (n_out, max(len(K) for _, K in rows))
        for i, (xmin, K) in enumerate(rows):
            assert bounds[i].tolist() == [xmin, len(K)] and coeffs[i, :len(K)].tolist() == K and not coeffs[i, len(K):].any()
            assert 0 <= xmin and len(K) >= 1 and xmin + len(K) <= n_in
            # the row sums to 1 up to one rounding per tap, and an int32 accumulator holds every partial sum of 8-bit samples
            assert abs(sum(K) - (1 << 22)) <= len(K), (n_in, n_out, i)
            assert 255 * sum(abs(v) for v in K) + (1 << 21) < 1 << 31 and max(abs(v) for v in K) < 1 << 23


def test_the_long_row_has_its_257_taps():
    from aivc_amd import resize
    bounds, coeffs = resize.axis_tables(300, 7, 'lanczos')  # 2 x 3 x 300 / 7 = 257.1 input columns under the filter
    assert bounds[:, 1].max() == coeffs.shape[1] and coeffs.shape[1] in (257, 258)  # (258 where the window's ends both round out)
    assert resize.device_tables(300, 7, 'lanczos', 256)[1].shape == (260, 8)


@pytest.mark.parametrize('name', ['box', 'bicubic', 'lanczos'])
def test_device_layout(name):
    from aivc_amd import abi, resize
    for n_in, n_out in AXES:
        bounds, coeffs = resize.axis_tables(n_in, n_out, name)
        b, t, span = resize.device_tables(n_in, n_out, name, abi.RESIZE_TILE_W)
        assert b is bounds and t.dtype == np.int32 and t.flags['C_CONTIGUOUS']
        taps, pitch = t.shape
        assert taps % 4 == 0 and pitch % 4 == 0 and 0 <= taps - coeffs.shape[1] < 4 and 0 <= pitch - n_out < 4
        assert np.array_equal(t[:coeffs.shape[1], :n_out], coeffs.T) and not t[coeffs.shape[1]:].any() and not t[:, n_out:].any()
        want = max(int(bounds[min(x0 + abi.RESIZE_TILE_W, n_out) - 1, 0]) + taps - int(bounds[x0, 0])
                   for x0 in range(0, n_out, abi.RESIZE_TILE_W))
        assert span == want
        # what the kernel relies on: the windows move right with the column
        assert (np.diff(bounds[:, 0]) >= 0).all() and (np.diff(bounds.sum(1)) >= 0).all()


def test_tables_are_cached_and_read_only():
    from aivc_amd import resize
    a = resize.axis_tables(61, 30, 'hamming')
    assert resize.axis_tables(61, 30, 'hamming')[1] is a[1]
    with pytest.raises(ValueError):
        a[1][0, 0] = 1
    with pytest.raises(ValueError):
        resize.axis_tables(61, 30, 'nearest')
    with pytest.raises(ValueError):
        resize.axis_tables(0, 30, 'box')


def test_abi_binds_and_library_exports_resize():
    import ctypes
    from aivc_amd import abi
    assert abi.ABI_VERSION >= 25 and set(abi.RESIZE_PROTOTYPES) == {'aivc_resize_u8'}
    assert not set(abi.RESIZE_PROTOTYPES) & set(abi.PROTOTYPES)  # device only: the oracle has no `_ref` twin
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)
    assert hasattr(lib, 'aivc_resize_u8')
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_resize.h')).read()
    assert 'int aivc_resize_u8(const uint8_t *const *planes, int32_t n, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out,' in header
    assert '#define AIVC_RESIZE_TILE_W %d\n' % abi.RESIZE_TILE_W in header
    assert '#define AIVC_RESIZE_MAX_SPAN %d\n' % abi.RESIZE_MAX_SPAN in header
    assert len(abi.RESIZE_PROTOTYPES['aivc_resize_u8']) == 14  # (+ the stream) as the header's 15 parameters


def test_resize_argument_errors_without_gpu():
    """every rejection of the header, with stand-in pointers: no kernel is launched"""
    from aivc_amd import _lib
    f = _lib.load()['aivc_resize_u8']
    P = 1 << 20  # a stand-in for a device pointer
    ok = dict(planes=P, n=1, h_in=8, w_in=8, h_out=4, w_out=4, xb=P, xk=P, x_taps=8, x_span=20, yb=P, yk=P, tmp=P, out=P)

    def call(**kw):
        a = dict(ok, **kw)
        return f(a['planes'], a['n'], a['h_in'], a['w_in'], a['h_out'], a['w_out'], a['xb'], a['xk'], a['x_taps'], a['x_span'],
                 a['yb'], a['yk'], a['tmp'], a['out'], None)
    assert call(n=0) == 0 and call(n=0, planes=None, out=None) == 0  # nothing to do
    assert call(n=-1) == -1
    for bad in (dict(planes=None), dict(out=None), dict(h_in=0), dict(w_in=0), dict(h_out=0), dict(w_out=-3), dict(xk=None),
                dict(xb=None), dict(yk=None), dict(yb=None), dict(xb=None, xk=None), dict(yb=None, yk=None), dict(x_taps=0),
                dict(x_taps=6), dict(x_span=0), dict(tmp=None)):
        assert call(**bad) == -1, bad
    assert call(xb=None, xk=None, yb=None, yk=None) == -1  # a copy of 8 x 8 into 4 x 4
    from aivc_amd import abi
    assert call(x_span=abi.RESIZE_MAX_SPAN + 1) == abi.ERR_UNSUPPORTED
    assert call(w_out=65536 * abi.RESIZE_TILE_W) == abi.ERR_UNSUPPORTED
    assert call(n=1 << 30, h_in=64) == abi.ERR_UNSUPPORTED and call(n=1 << 30, h_out=64) == abi.ERR_UNSUPPORTED


def test_ops_refuses_before_it_touches_the_device():
    """CPU tensors like everywhere in ops; and the shapes no launch can express, named in the message"""
    import torch
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    with pytest.raises(AivcNativeError):
        ops.resize_u8([torch.zeros(8, 8, dtype=torch.uint8)], 4, 4)
    with pytest.raises(ValueError):
        ops.resize_u8([], 4, 4)


# ---- the command lines ---------------------------------------------------------------------------------------------------

def test_parse_size():
    from aivc_amd import resize
    assert resize.parse_size('1920x1080') == (1920, 1080) and resize.parse_size('7X9') == (7, 9)
    for bad in ('1920', '1920x', 'x1080', '0x4', '4x0', '-4x4', '4x4x4', '4.5x4', 'axb', '', '4 x 4'):
        with pytest.raises(ValueError):
            resize.parse_size(bad)
    assert resize.chroma_size(33, 47) == (17, 24)


def _exits(parse, argv, capsys, needle):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2
    assert needle in capsys.readouterr().err


def test_encode_flags(capsys):
    from aivc_amd import encode
    a = encode.parse_args([])
    assert a.size is None and a.resample == 'bicubic'
    a = encode.parse_args(['--size', '64x48'])
    assert a.size == (64, 48) and a.resample == 'bicubic'
    for name in rc.FILTER_NAMES:
        assert encode.parse_args(['--size', '33x47', '--resample', name]).resample == name
    _exits(encode.parse_args, ['--resample', 'box'], capsys, 'needs --size')
    _exits(encode.parse_args, ['--size', '64x48', '--resample', 'nearest'], capsys, 'invalid choice')
    for bad in ('64', '0x48', '64x-48', '64x48x3', 'WxH'):
        _exits(encode.parse_args, ['--size', bad], capsys, 'argument --size')


def test_decode_flags(capsys, tmp_path):
    from aivc_amd import decode
    a = decode.parse_args([])
    assert a.out_size is None and a.resample == 'bicubic'
    a = decode.parse_args(['--out_size', '97x23', '--resample', 'lanczos', '-o', str(tmp_path / 'out.yuv')])
    assert a.out_size == (97, 23) and a.resample == 'lanczos'
    _exits(decode.parse_args, ['--resample', 'lanczos'], capsys, 'needs --out_size')
    _exits(decode.parse_args, ['--out_size', '0x0'], capsys, 'argument --out_size')
    # RGB pictures as output: even sides only (-o names a folder by its trailing '/' or by being one)
    assert decode.parse_args(['--out_size', '96x64', '-o', str(tmp_path) + '/']).out_size == (96, 64)
    _exits(decode.parse_args, ['--out_size', '97x64', '-o', str(tmp_path) + '/'], capsys, 'even sides')
    _exits(decode.parse_args, ['--out_size', '96x63', '-o', str(tmp_path)], capsys, 'even sides')


def test_aivc_flags(capsys, tmp_path):
    from aivc_amd import aivc
    a = aivc.parse_args([])
    assert a.size is None and a.out_size is None and a.resample == 'bicubic'
    a = aivc.parse_args(['--size', '1920x1080', '--out_size', '3840x2160', '--resample', 'hamming'])
    assert a.size == (1920, 1080) and a.out_size == (3840, 2160) and a.resample == 'hamming'
    assert aivc.parse_args(['--out_size', '64x48', '--resample', 'box']).resample == 'box'
    _exits(aivc.parse_args, ['--resample', 'box'], capsys, 'needs --size or --out_size')
    _exits(aivc.parse_args, ['--size', '1920'], capsys, 'argument --size')
    _exits(aivc.parse_args, ['--out_size', '63x48', '-o', str(tmp_path) + '/'], capsys, 'even sides')
