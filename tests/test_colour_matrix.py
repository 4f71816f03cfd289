"""aivc_amd/color.py, the statement of the colour conversion by matrix and range (include/aivc_hip_color_matrix.h), without a GPU:
the known-answer integers, the row sums and grey exactness the G correction buys, the derived error bound against the fp64
formula on ALL 2^24 triples in both directions, the single rounding of box chroma, the ABI beside the pinned one, and the flags
of the three command lines.

The bound.  A coefficient is round(real x 2^14): off by at most 2^-15, a corrected G entry by at most 3 x 2^-15; the inputs are
at most 255.  The unrounded fixed-point value is therefore within 255 x 5 x 2^-15 < 0.04 of the real-valued formula, and the
floor of (value + 1/2) within 0.5 of that: 0.54 in all.  The fp64 formula below is written from Kr, Kb, ys, cs and yo, not from
the module's integers."""
import ctypes
import os

import numpy as np
import pytest

from aivc_amd import color

KR_KB = {'bt601': (0.299, 0.114), 'bt709': (0.2126, 0.0722), 'bt2020': (0.2627, 0.0593)}
YS_CS_YO = {'full': (1.0, 1.0, 0.0), 'limited': (219.0 / 255.0, 224.0 / 255.0, 16.0)}
SPECS = [(m, r) for m in ('bt601', 'bt709', 'bt2020') for r in ('full', 'limited')]
BOUND = 0.54

KNOWN = {
    ('bt601', 'full'): ([[4899, 9617, 1868], [-2765, -5427, 8192], [8192, -6860, -1332]], [16384, 22970, -5638, -11700, 29032]),
    ('bt709', 'limited'): ([[2991, 10064, 1016], [-1649, -5547, 7196], [7196, -6536, -660]], [19077, 29372, -3494, -8731, 34610]),
    ('bt2020', 'limited'): ([[3696, 9541, 834], [-2010, -5186, 7196], [7196, -6617, -579]], [19077, 27503, -3069, -10657, 35091]),
}


def ys14(rng):
    return {'full': 16384, 'limited': 14071}[rng]  # round(219 / 255 x 2^14) = round(14070.96)


def test_module_names_what_it_offers():
    assert list(color.MATRICES) == ['bt601', 'bt709', 'bt2020'] and list(color.RANGES) == ['full', 'limited']
    assert color.ColourSpec('bt709') == ('bt709', 'limited') and color.ColourSpec('bt601', 'full').range == 'full'
    for bad in (('bt470', 'full'), ('bt709', 'tv')):
        with pytest.raises(ValueError):
            color.ColourSpec(*bad)
    with pytest.raises(ValueError):
        color.forward_numpy(np.zeros((1, 2, 2, 3), np.uint8), ('bt709', 'limited'), 'bilinear')


@pytest.mark.parametrize('spec', sorted(KNOWN))
def test_known_answer_coefficients(spec):
    c = color.coefficients(color.ColourSpec(*spec))
    fwd, inv = KNOWN[spec]
    assert [list(r) for r in c.fwd] == fwd and list(c.inv) == inv
    yo = 16 if spec[1] == 'limited' else 0
    assert tuple(c.fwd_off) == (yo, 128, 128) and c.inv_yoff == yo


@pytest.mark.parametrize('spec', SPECS)
def test_row_sums_and_grey_exactness(spec):
    c = color.coefficients(spec)
    assert ys14('limited') == round(219 / 255 * 2 ** 14)
    assert sum(c.fwd[0]) == ys14(spec[1]) and sum(c.fwd[1]) == 0 and sum(c.fwd[2]) == 0
    yo = 16 if spec[1] == 'limited' else 0
    v = np.arange(256)
    grey = np.stack([v, v, v], axis=-1).astype(np.uint8)
    got = color.forward_pixels(grey, spec)
    assert np.array_equal(got[:, 1], np.full(256, 128)) and np.array_equal(got[:, 2], np.full(256, 128))
    assert np.array_equal(got[:, 0], (ys14(spec[1]) * v + (yo << 14) + 8192) >> 14)
    y, u, v2 = color.forward_numpy(grey.reshape(1, 16, 16, 3), spec, 'box')
    assert (u == 128).all() and (v2 == 128).all()


def slabs():
    """all 2^24 triples, 2^21 at a time: uint8 [32, 256, 256, 3]"""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing='ij')
    for r0 in range(0, 256, 32):
        t = np.empty((32, 256, 256, 3), np.uint8)
        t[..., 0] = np.arange(r0, r0 + 32, dtype=np.uint8)[:, None, None]
        t[..., 1], t[..., 2] = g, b
        yield t


def real_forward(t, spec):
    kr, kb = KR_KB[spec[0]]
    kg = 1.0 - kr - kb
    ys, cs, yo = YS_CS_YO[spec[1]]
    r, g, b = (t[..., k].astype(np.float64) for k in range(3))
    return np.stack([ys * (kr * r + kg * g + kb * b) + yo,
                     cs * (-kr * r - kg * g + (1.0 - kb) * b) / (2.0 * (1.0 - kb)) + 128.0,
                     cs * ((1.0 - kr) * r - kg * g - kb * b) / (2.0 * (1.0 - kr)) + 128.0], axis=-1)


def real_inverse(t, spec):
    kr, kb = KR_KB[spec[0]]
    kg = 1.0 - kr - kb
    ys, cs, yo = YS_CS_YO[spec[1]]
    y, cb, cr = t[..., 0].astype(np.float64) - yo, t[..., 1].astype(np.float64) - 128.0, t[..., 2].astype(np.float64) - 128.0
    return np.stack([y / ys + 2.0 * (1.0 - kr) / cs * cr,
                     y / ys - kb * 2.0 * (1.0 - kb) / (kg * cs) * cb - kr * 2.0 * (1.0 - kr) / (kg * cs) * cr,
                     y / ys + 2.0 * (1.0 - kb) / cs * cb], axis=-1)


def worst_over_every_triple(fixed, real):
    worst = {}
    for spec in SPECS:
        w = 0.0
        for t in slabs():
            w = max(w, float(np.abs(fixed(t, spec, clamp=False) - real(t, spec)).max()))
        worst[spec] = w
    print('worst |fixed - real| per matrix and range:', {'%s %s' % s: round(w, 4) for s, w in worst.items()})
    return worst


def test_forward_within_the_derived_bound_on_every_triple():
    worst = worst_over_every_triple(color.forward_pixels, real_forward)
    assert all(w <= BOUND for w in worst.values()), worst


def test_inverse_within_the_derived_bound_on_every_triple():
    worst = worst_over_every_triple(color.inverse_pixels, real_inverse)
    assert all(w <= BOUND for w in worst.values()), worst


def test_planes_are_the_pixels_and_clamped():
    """forward_numpy / inverse_numpy are forward_pixels / inverse_pixels in the plane geometry; the clamp is 0 ... 255"""
    rng = np.random.default_rng(0)
    rgb = rng.integers(0, 256, (2, 7, 9, 3), dtype=np.uint8)
    spec = ('bt709', 'limited')
    y, u, v = color.forward_numpy(rgb, spec)
    px = color.forward_pixels(rgb, spec)
    assert y.shape == (2, 7, 9) and u.shape == v.shape == (2, 3, 4) and y.dtype == u.dtype == np.uint8
    assert np.array_equal(y, px[..., 0]) and np.array_equal(u, px[:, 0:6:2, 0:8:2, 1]) and np.array_equal(v, px[:, 0:6:2, 0:8:2, 2])
    for (ch, cw) in ((3, 4), (4, 5)):  # floor- and ceil-sized planes: the indices clamp to the plane
        uu, vv = (rng.integers(0, 256, (2, ch, cw), dtype=np.uint8) for _ in range(2))
        got = color.inverse_numpy(y, uu, vv, spec, 1)
        for (i, j) in ((0, 0), (6, 8), (5, 8), (6, 7), (3, 2)):
            want = color.inverse_pixels(np.stack([y[:, i, j], uu[:, min(i // 2, ch - 1), min(j // 2, cw - 1)],
                                                  vv[:, min(i // 2, ch - 1), min(j // 2, cw - 1)]], axis=-1), spec)
            assert np.array_equal(got[:, i, j], want)
    # full-range chroma reaches 256 in front of the clamp; limited-range planes below black go through the same formula
    assert color.forward_pixels(np.array([[0, 0, 255]], np.uint8), ('bt601', 'full'), clamp=False)[0, 1] == 256
    assert color.forward_pixels(np.array([[0, 0, 255]], np.uint8), ('bt601', 'full'))[0, 1] == 255
    assert tuple(color.inverse_pixels(np.array([[0, 128, 128]], np.uint8), spec, clamp=False)[0]) == ((19077 * -16 + 8192) >> 14,) * 3
    assert tuple(color.inverse_pixels(np.array([[0, 128, 128]], np.uint8), spec)[0]) == (0, 0, 0)
    with pytest.raises(ValueError):
        color.inverse_numpy(y, u[:, :2], v[:, :2], spec, 1)


@pytest.mark.parametrize('spec', SPECS)
def test_box_chroma_is_rounded_once(spec):
    rng = np.random.default_rng(5)
    corners = np.array([[a, b, c] for a in (0, 255) for b in (0, 255) for c in (0, 255)], np.uint8)
    extremes = corners[rng.integers(0, 8, (64, 2, 2))]                  # blocks whose four pixels are 0 / 255 corners
    uniform = np.repeat(np.repeat(corners[:, None, None], 2, 1), 2, 2)  # ... and the eight blocks of one corner
    blocks = np.concatenate([rng.integers(0, 256, (4096, 2, 2, 3), dtype=np.uint8), extremes, uniform])
    m = color.coefficients(spec).fwd
    s = blocks.astype(np.int64).sum(axis=(1, 2))
    _, u, v = color.forward_numpy(blocks, spec, 'box')
    for k, got in ((1, u), (2, v)):
        want = np.clip((m[k][0] * s[:, 0] + m[k][1] * s[:, 1] + m[k][2] * s[:, 2] + (128 << 16) + (1 << 15)) >> 16, 0, 255)
        assert np.array_equal(got.reshape(-1), want)
    # a picture: every whole block, nothing of an odd last row / column
    rgb = rng.integers(0, 256, (1, 5, 7, 3), dtype=np.uint8)
    y, u, v = color.forward_numpy(rgb, spec, 'box')
    assert u.shape == (1, 2, 3) and np.array_equal(y, color.forward_numpy(rgb, spec, 'point')[0])
    one = color.forward_numpy(rgb[:, 2:4, 4:6], spec, 'box')
    assert u[0, 1, 2] == one[1][0, 0, 0] and v[0, 1, 2] == one[2][0, 0, 0]


# ---- ABI -------------------------------------------------------------------------------------------------------------------
NAMES = {'aivc_rgb8_to_yuv420u8_matrix', 'aivc_yuv8_to_rgb8_matrix'}


def test_abi_is_the_pinned_one_with_two_entries_added():
    from aivc_amd import _lib, abi
    assert abi.ABI_VERSION == 26
    assert set(abi.COLOR_MATRIX_PROTOTYPES) == NAMES and set(abi.COLOR_PROTOTYPES) == {'aivc_rgb8_to_yuv420u8', 'aivc_yuv8_to_rgb8'}
    fns = _lib.load()
    assert NAMES <= set(fns) and fns['aivc_abi_version']() == 26
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NAMES:
        getattr(lib, name)  # exported
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'aivc_hip_color_matrix.h')).read()
    assert all('int %s(' % name in header for name in NAMES) and 'typedef struct aivc_color_matrix' in header
    assert ctypes.sizeof(abi.ColorMatrix) == 4 * (9 + 3 + 5 + 1)
    assert '#define AIVC_ABI_VERSION 26' in open(os.path.join(root, 'include', 'aivc_hip.h')).read()


def test_argument_errors_return_codes_without_a_device():
    from aivc_amd import _lib
    fns = _lib.load()
    fwd, inv = fns['aivc_rgb8_to_yuv420u8_matrix'], fns['aivc_yuv8_to_rgb8_matrix']
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)

    def matrix(**change):
        m = color._struct(('bt709', 'limited'))
        for k, (idx, val) in change.items():
            field = getattr(m, k)
            if idx is None:
                setattr(m, k, val)
            elif isinstance(idx, tuple):
                field[idx[0]][idx[1]] = val
            else:
                field[idx] = val
        return ctypes.byref(m)
    ok = matrix()
    # the existing pair's errors
    assert fwd(None, 1, 2, 2, ok, 0, p, p, p, None) == -1
    assert fwd(p, 1, 0, 2, ok, 0, p, p, p, None) == -1
    assert fwd(p, 1, 2, 2, ok, 0, p, None, None, None) == -1          # a chroma sample exists: planes needed
    assert inv(p, p, p, 1, 2, 2, 1, 1, 2, ok, p, None) == -1          # chroma_shift
    assert inv(p, p, p, 1, 1, 1, 0, 0, 1, ok, p, None) == -1          # a chroma plane of size zero
    assert inv(p, p, p, 1, 4, 4, 2, 2, 0, ok, p, None) == -1          # full resolution asked, half given
    assert inv(p, p, p, 1, 5, 5, 1, 2, 1, ok, p, None) == -1          # fewer rows than floor(h / 2)
    # the new ones
    assert fwd(p, 1, 2, 2, None, 0, p, p, p, None) == -1 and inv(p, p, p, 1, 2, 2, 1, 1, 1, None, p, None) == -1   # NULL m
    for down in (-1, 2):
        assert fwd(p, 1, 2, 2, ok, down, p, p, p, None) == -1
    for bad in (matrix(fwd=((1, 1), 65537)), matrix(fwd=((2, 0), -65537)), matrix(inv=(4, 65537)), matrix(inv=(2, -65537)),
                matrix(fwd_off=(0, 256)), matrix(fwd_off=(2, -1)), matrix(inv_yoff=(None, 256)), matrix(inv_yoff=(None, -1))):
        assert fwd(p, 1, 2, 2, bad, 0, p, p, p, None) == -1
        assert inv(p, p, p, 1, 2, 2, 1, 1, 1, bad, p, None) == -1


# ---- flags -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp('colour_flags')
    rgb, planes = tmp / 'rgb', tmp / 'planes'
    os.makedirs(rgb), os.makedirs(planes)
    Image.fromarray(np.zeros((4, 4, 3), np.uint8), 'RGB').save(rgb / '0.png')
    for k in 'yuv':
        Image.fromarray(np.zeros((4, 4) if k == 'y' else (2, 2), np.uint8), 'L').save(planes / ('0_%s.png' % k))
    return {'rgb': str(rgb), 'planes': str(planes), 'raw': str(tmp / 'clip_4x4_25_420.yuv'), 'out': str(tmp / 'out') + '/',
            'yuv': str(tmp / 'out.yuv')}


def exits_2(parse, argv):
    with pytest.raises(SystemExit) as e:
        parse(argv)
    assert e.value.code == 2, argv


def test_encoder_flags(folders, capsys):
    from aivc_amd.encode import parse_args
    a = parse_args(['-i', folders['rgb']])
    assert a.colour is None and a.matrix is None and a.range is None and a.chroma_down == 'point'
    a = parse_args(['-i', folders['rgb'], '--matrix', 'bt709'])
    assert a.colour == color.ColourSpec('bt709', 'limited') and a.chroma_down == 'point'
    a = parse_args(['-i', folders['rgb'], '--matrix', 'bt2020', '--range', 'full', '--chroma_down', 'box'])
    assert a.colour == ('bt2020', 'full') and a.chroma_down == 'box'
    assert parse_args(['-i', folders['rgb'], '--chroma_down', 'point']).colour is None
    for src in ('raw', 'planes'):
        assert parse_args(['-i', folders[src]]).colour is None
    exits_2(parse_args, ['-i', folders['rgb'], '--range', 'limited'])
    exits_2(parse_args, ['-i', folders['rgb'], '--chroma_down', 'box'])
    exits_2(parse_args, ['-i', folders['rgb'], '--matrix', 'bt470'])
    for src in ('raw', 'planes'):
        exits_2(parse_args, ['-i', folders[src], '--matrix', 'bt709'])
        exits_2(parse_args, ['-i', folders[src], '--matrix', 'bt709', '--range', 'full'])
        exits_2(parse_args, ['-i', folders[src], '--matrix', 'bt709', '--chroma_down', 'box'])
    capsys.readouterr()
    with pytest.raises(SystemExit):
        parse_args(['--help'])
    assert '--matrix alone means --range limited' in ' '.join(capsys.readouterr().out.split())


def test_decoder_flags(folders):
    from aivc_amd.decode import parse_args
    assert parse_args(['-o', folders['out']]).colour is None and parse_args(['-o', folders['yuv']]).colour is None
    assert parse_args(['-o', folders['out'], '--matrix', 'bt709']).colour == ('bt709', 'limited')
    assert parse_args(['-o', folders['out'], '--matrix', 'bt601', '--range', 'full']).colour == ('bt601', 'full')
    exits_2(parse_args, ['-o', folders['out'], '--range', 'full'])
    exits_2(parse_args, ['-o', folders['yuv'], '--matrix', 'bt709'])
    exits_2(parse_args, ['-o', folders['yuv'], '--matrix', 'bt709', '--range', 'limited'])
    exits_2(parse_args, ['-o', folders['out'], '--matrix', 'bt709', '--chroma_down', 'box'])  # (the encoder's flag)


def test_aivc_flags(folders):
    from aivc_amd.aivc import parse_args
    assert parse_args(['-i', folders['rgb'], '-o', folders['out']]).colour is None
    a = parse_args(['-i', folders['rgb'], '-o', folders['out'], '--matrix', 'bt709', '--chroma_down', 'box'])
    assert a.colour == ('bt709', 'limited') and a.chroma_down == 'box'
    exits_2(parse_args, ['-i', folders['rgb'], '-o', folders['out'], '--range', 'full'])
    exits_2(parse_args, ['-i', folders['rgb'], '-o', folders['out'], '--chroma_down', 'box'])
    exits_2(parse_args, ['-i', folders['raw'], '-o', folders['out'], '--matrix', 'bt709'])
    exits_2(parse_args, ['-i', folders['planes'], '-o', folders['out'], '--matrix', 'bt709'])
    exits_2(parse_args, ['-i', folders['rgb'], '-o', folders['yuv'], '--matrix', 'bt709'])


def test_library_defaults_and_refusals(folders):
    """the keyword defaults are None / 'point'; what holds planes already is refused before anything is read"""
    import inspect
    from aivc_amd.func_util import img_processing as ip
    from aivc_amd.real_life import decode as dec
    from aivc_amd.real_life import encode as enc
    sig = inspect.signature
    assert sig(ip.load_RGB_as_YUV420_dic).parameters['colour'].default is None
    assert sig(ip.load_RGB_as_YUV420_dic).parameters['chroma_down'].default == 'point'
    assert sig(ip.save_tensor_as_img).parameters['colour'].default is None
    assert sig(enc.read_png_folder).parameters['colour'].default is None and sig(enc.read_png_folder).parameters['chroma_down'].default == 'point'
    from aivc_amd.options import Source
    assert Source().colour is None and Source().chroma_down == 'point'
    assert sig(dec.write_png_folder).parameters['colour'].default is None
    assert list(sig(dec.write_png_folder).parameters)[:5] == ['frames', 'directory', 'device', 'indices', 'coder']
    spec = color.ColourSpec('bt709')
    for seq in (folders['raw'], folders['planes']):
        with pytest.raises(ValueError):
            enc._source(seq, 0, -1, None, Source(colour=spec))
    with pytest.raises(ValueError):
        enc._source(folders['rgb'], 0, -1, None, Source(chroma_down='box'))
    with pytest.raises(ValueError):
        ip.save_tensor_as_img(None, 'x.png', mode='rgb', colour=spec)
    assert color.info_line(spec) == '[INFO] colour: bt709 limited' and color.info_line(spec, 'box') == '[INFO] colour: bt709 limited, box chroma'
