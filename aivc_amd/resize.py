"""Pillow's 8-bit resampling, host half: the integer coefficient tables of one axis (include/aivc_hip_resize.h states the
arithmetic, aivc_amd.ops.resize_u8 runs it on the device) and the WxH sizes of the command lines (aivc_amd/options.py).

The tables are Image.resize's on an 'L' picture (reducing_gap=None, the whole picture as box), bit for bit: doubles, math.sin /
math.cos and the expression order of Pillow's precompute_coeffs / normalize_coeffs_8bpc.  tests/resize_cases.py restates the
arithmetic on its own and tests/test_resize_coeffs.py holds both against Pillow."""
import functools
import math

import numpy as np

PRECISION_BITS = 22  # 32 - 8 - 2: a coefficient is a multiple of 2^-22, an accumulator an int32


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (0.54 + 0.46 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


# name -> (support, f): the five filters of Image.resize that share one code path ('nearest' is another one and is not offered)
FILTERS = {'box': (0.5, _box), 'bilinear': (1.0, _bilinear), 'hamming': (1.0, _hamming), 'bicubic': (2.0, _bicubic),
           'lanczos': (3.0, _lanczos)}
DEFAULT_FILTER = 'bicubic'  # Pillow's own default


def check_filter(name):
    if name not in FILTERS:
        raise ValueError('resample filter %r: expected one of %s' % (name, ', '.join(FILTERS)))
    return name


@functools.lru_cache(maxsize=64)
def axis_tables(n_in, n_out, name):
    """One axis, n_in -> n_out samples under filter `name` -> (bounds, coeffs), read-only arrays:
    bounds  int32 [n_out, 2]: (xmin, count) -- output i is the weighted sum of the inputs xmin ... xmin + count - 1;
    coeffs  int32 [n_out, taps], taps = max count: row i holds its count coefficients in units of 2^-22, zeros behind them."""
    support, f = FILTERS[check_filter(name)]
    n_in, n_out = int(n_in), int(n_out)
    if n_in < 1 or n_out < 1:
        raise ValueError('axis_tables: %d -> %d samples' % (n_in, n_out))
    scale = n_in / n_out
    filterscale = max(scale, 1.0)
    support = support * filterscale
    ss = 1.0 / filterscale
    bounds = np.zeros((n_out, 2), np.int32)
    rows = []
    for xx in range(n_out):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), n_in) - xmin
        k = [f((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        rows.append([int(-0.5 + w * (1 << PRECISION_BITS)) if w < 0 else int(0.5 + w * (1 << PRECISION_BITS)) for w in k])
        bounds[xx] = xmin, xmax
    coeffs = np.zeros((n_out, max(int(bounds[:, 1].max()), 1)), np.int32)
    for xx, row in enumerate(rows):
        coeffs[xx, :len(row)] = row
    bounds.setflags(write=False)
    coeffs.setflags(write=False)
    return bounds, coeffs


@functools.lru_cache(maxsize=64)
def device_tables(n_in, n_out, name, tile):
    """axis_tables in the layout of include/aivc_hip_resize.h -> (bounds int32 [n_out, 2], coeffs int32 [taps, pitch], span):
    the coefficients TRANSPOSED, rows padded to pitch = n_out rounded up to 4, taps rounded up to 4, zeros in all padding;
    span = max over the tiles of `tile` outputs of first[last of the tile] + taps - first[first of the tile]."""
    bounds, coeffs = axis_tables(n_in, n_out, name)
    if int(np.abs(coeffs).max()) >= 1 << 23:  # (normalised weights stay below 2: never seen)
        raise ValueError('resize %d -> %d (%s): a coefficient of %d / 2^22 does not fit the 24-bit multiply'
                         % (n_in, n_out, name, int(np.abs(coeffs).max())))
    taps, pitch = -(-coeffs.shape[1] // 4) * 4, -(-n_out // 4) * 4
    t = np.zeros((taps, pitch), np.int32)
    t[:coeffs.shape[1], :n_out] = coeffs.T
    first = bounds[:, 0].astype(np.int64)
    starts = np.arange(0, n_out, tile)
    span = int((first[np.minimum(starts + tile - 1, n_out - 1)] + taps - first[starts]).max())
    t.setflags(write=False)
    return bounds, t, span


def chroma_size(w, h):
    """the 4:2:0 chroma planes of a w x h frame: ceil-sized, as the planar files and the codec hold them"""
    return (w + 1) // 2, (h + 1) // 2


def parse_size(text):
    """'WxH' -> (w, h), both positive; ValueError otherwise"""
    parts = str(text).lower().split('x')
    if len(parts) != 2 or not all(p.isdigit() for p in parts):
        raise ValueError('%r: expected WxH, two positive integers (1920x1080)' % (text,))
    w, h = int(parts[0]), int(parts[1])
    if w < 1 or h < 1:
        raise ValueError('%r: width and height must be positive' % (text,))
    return w, h


def check_resample(resample, sizes):
    """a ValueError for a filter where nothing is resized: `sizes`, {flag: size or None}, holds no size.  In the style of
    aivc_amd.png.check_reader / check_coder."""
    if resample is not None and all(v is None for v in sizes.values()):
        raise ValueError('--resample %s: needs %s (nothing is resized without a size)' % (resample, ' or '.join(sizes)))
