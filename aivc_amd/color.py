"""8-bit RGB <-> YCbCr by matrix and range: BT.601 / BT.709 / BT.2020, full or limited range (include/aivc_hip_color_matrix.h).

The package's default colour conversion is Pillow's JFIF arithmetic (ops.rgb8_to_yuv420u8 / ops.yuv8_to_rgb8: BT.601, full range,
floored), which is the reference's.  This module is the conversion a caller asks for by saying what the planes carry; nothing
here runs unless a ColourSpec is given.  THE STATEMENT of the arithmetic is this file: `coefficients` (fractions) and
`forward_numpy` / `inverse_numpy` (numpy); the header repeats it and the kernels equal it byte for byte.

Integer only, S = 14 fractional bits, `>>` an arithmetic shift (a floor), every result clamped to 0 ... 255.

  Kr, Kb      exact decimal fractions (MATRICES), Kg = 1 - Kr - Kb
  range       full: ys = cs = 1, yo = 0;  limited: ys = 219 / 255, cs = 224 / 255, yo = 16
  forward     real rows  Y = ys (Kr, Kg, Kb),  Cb = cs (-Kr, -Kg, 1 - Kb) / (2 (1 - Kb)),  Cr = cs (1 - Kr, -Kg, -Kb) / (2 (1 - Kr));
              m = round(real x 2^S), half to even, on Fractions; the G entry of each row is then corrected so that the Y row sums
              to exactly round(ys x 2^S) and the chroma rows to 0: a grey pixel gives Cb = Cr = 128 exactly.
              out_i = clamp((m_i . (r, g, b) + (off_i << S) + (1 << (S - 1))) >> S),  off = (yo, 128, 128)
  chroma      'point': the Cb, Cr of pixel (2i, 2j), floor-sized planes (the geometry of ops.rgb8_to_yuv420u8);
              'box': from the exact sums of R, G and B over the 2 x 2 block, rounded ONCE:
              clamp((m_i . sum + (128 << (S + 2)) + (1 << (S + 1))) >> (S + 2)).  Floor-sized planes hold whole blocks only.
  inverse     (cy, rv, gu, gv, bu) = round(2^S x) of 1 / ys, 2 (1 - Kr) / cs, -Kb 2 (1 - Kb) / (Kg cs), -Kr 2 (1 - Kr) / (Kg cs),
              2 (1 - Kb) / cs;  R = clamp((cy (Y - yo) + rv (Cr - 128) + (1 << (S - 1))) >> S), G likewise with
              gu (Cb - 128) + gv (Cr - 128), B with bu (Cb - 128).  Inputs outside the nominal range take the same formula.
              Chroma geometry: that of ops.yuv8_to_rgb8 (chroma_shift 0 or 1, nearest x 2, cropped, indices clamped).

Error (derived): a coefficient is off by at most 2^-15 (3 x 2^-15 for a corrected G), inputs are at most 255, so every output
before the clamp is within 0.5 + 255 x 5 x 2^-15 < 0.54 of the real-valued formula (tests/test_colour_matrix.py: all 2^24 triples).

The stream stores no colour description, as it stores no frame rate and no display size: encoder and decoder are both told.
"""
import collections
import ctypes as C
from fractions import Fraction

import numpy as np

SHIFT = 14  # S
MATRICES = {'bt601': (Fraction(299, 1000), Fraction(114, 1000)),  # Kr, Kb
            'bt709': (Fraction(2126, 10000), Fraction(722, 10000)),
            'bt2020': (Fraction(2627, 10000), Fraction(593, 10000))}
RANGES = {'full': (Fraction(1), Fraction(1), 0),  # ys, cs, yo
          'limited': (Fraction(219, 255), Fraction(224, 255), 16)}
CHROMA_DOWN = ('point', 'box')

Coefficients = collections.namedtuple('Coefficients', 'fwd fwd_off inv inv_yoff')  # fwd: rows Y, Cb, Cr; inv: cy, rv, gu, gv, bu


class ColourSpec(collections.namedtuple('ColourSpec', 'matrix range')):
    """what the planes carry: a name of MATRICES and a name of RANGES (default 'limited', video's convention)"""
    __slots__ = ()

    def __new__(cls, matrix, range='limited'):
        if matrix not in MATRICES:
            raise ValueError('colour matrix %r (expected one of %s)' % (matrix, ', '.join(MATRICES)))
        if range not in RANGES:
            raise ValueError('colour range %r (expected one of %s)' % (range, ', '.join(RANGES)))
        return super().__new__(cls, matrix, range)

    def __str__(self):
        return '%s %s' % (self.matrix, self.range)


def as_spec(spec):
    """a ColourSpec, a (matrix, range) pair or a matrix name -> ColourSpec"""
    if isinstance(spec, ColourSpec):
        return spec
    if isinstance(spec, str):
        return ColourSpec(spec)
    return ColourSpec(*spec)


def check_chroma_down(chroma_down):
    if chroma_down not in CHROMA_DOWN:
        raise ValueError('chroma_down %r (expected point or box)' % (chroma_down,))
    return chroma_down


def info_line(spec, chroma_down='point'):
    """the one line a command prints when this arithmetic runs"""
    return '[INFO] colour: %s%s' % (as_spec(spec), ', box chroma' if chroma_down == 'box' else '')


def check_convertible(colour, chroma_down, path, rgb_pictures, flag='-i'):
    """a ValueError for a colour (or box chroma) where nothing is converted: `path` (the input, or with flag '-o' the output) is
    not a folder of RGB pictures.  In the style of aivc_amd.png.check_reader / check_coder."""
    check_chroma_down(chroma_down)
    if colour is None and chroma_down == 'point':
        return
    if colour is None:
        raise ValueError('--chroma_down box needs --matrix: Pillow\'s conversion, the default, keeps the chroma of pixel (2i, 2j)')
    as_spec(colour)
    if not rgb_pictures:
        raise ValueError('--matrix / --range%s convert RGB pictures: %s %s %s'
                         % (' / --chroma_down' if flag == '-i' else '', flag, path,
                            'is not a folder of RGB pictures (a raw video file and a folder of PNG triplets hold planes already)'
                            if flag == '-i' else 'is a raw video file (name a folder, or end the name with /)'))


def is_rgb_folder(path):
    """whether `path` is a folder whose pictures are one RGB PNG per frame (func_util.img_processing.detect_folder_layout)"""
    import os
    if not os.path.isdir(path):
        return False
    from .func_util.img_processing import detect_folder_layout
    try:
        return bool(detect_folder_layout(path)[1])
    except ValueError:
        return False


def _fix(x):
    return int(round(x * (1 << SHIFT)))  # (round() of a Fraction: exact, half to even)


def coefficients(spec):
    """-> Coefficients of plain ints (the integers of the module docstring)"""
    spec = as_spec(spec)
    kr, kb = MATRICES[spec.matrix]
    kg = 1 - kr - kb
    ys, cs, yo = RANGES[spec.range]
    rows = [[ys * kr, ys * kg, ys * kb],
            [cs * -kr / (2 * (1 - kb)), cs * -kg / (2 * (1 - kb)), cs * (1 - kb) / (2 * (1 - kb))],
            [cs * (1 - kr) / (2 * (1 - kr)), cs * -kg / (2 * (1 - kr)), cs * -kb / (2 * (1 - kr))]]
    fwd = [[_fix(x) for x in row] for row in rows]
    for row, total in zip(fwd, (_fix(ys), 0, 0)):
        row[1] = total - row[0] - row[2]
    inv = [_fix(1 / ys), _fix(2 * (1 - kr) / cs), _fix(-kb * 2 * (1 - kb) / (kg * cs)), _fix(-kr * 2 * (1 - kr) / (kg * cs)),
           _fix(2 * (1 - kb) / cs)]
    return Coefficients(tuple(tuple(r) for r in fwd), (yo, 128, 128), tuple(inv), yo)


def _clamp8(a, clamp):
    return np.clip(a, 0, 255).astype(np.uint8) if clamp else a


def forward_pixels(rgb, spec, clamp=True):
    """uint8 [..., 3] (R, G, B) -> [..., 3] (Y, Cb, Cr) of every pixel: uint8, or with clamp=False the int32 values in front of
    the clamp"""
    c = coefficients(spec)
    p = np.asarray(rgb).astype(np.int32)
    out = np.empty(p.shape, np.int32)
    for i in range(3):
        m = c.fwd[i]
        out[..., i] = (m[0] * p[..., 0] + m[1] * p[..., 1] + m[2] * p[..., 2] + (c.fwd_off[i] << SHIFT) + (1 << (SHIFT - 1))) >> SHIFT
    return _clamp8(out, clamp)


def box_chroma(rgb, spec, clamp=True):
    """uint8 [n, h, w, 3] -> [n, h // 2, w // 2, 2] (Cb, Cr) from the sums over the whole 2 x 2 blocks, rounded once"""
    c = coefficients(spec)
    p = np.asarray(rgb).astype(np.int32)
    n, h, w, _ = p.shape
    ch, cw = h // 2, w // 2
    s = p[:, :2 * ch, :2 * cw].reshape(n, ch, 2, cw, 2, 3).sum(axis=(2, 4))
    out = np.empty((n, ch, cw, 2), np.int32)
    for k, i in enumerate((1, 2)):
        m = c.fwd[i]
        out[..., k] = (m[0] * s[..., 0] + m[1] * s[..., 1] + m[2] * s[..., 2] + (c.fwd_off[i] << (SHIFT + 2)) + (1 << (SHIFT + 1))) >> (SHIFT + 2)
    return _clamp8(out, clamp)


def forward_numpy(rgb, spec, chroma_down='point', clamp=True):
    """uint8 [n, h, w, 3] -> (y [n, h, w], u, v [n, h // 2, w // 2]): what aivc_rgb8_to_yuv420u8_matrix must equal"""
    check_chroma_down(chroma_down)
    rgb = np.asarray(rgb)
    n, h, w, _ = rgb.shape
    ch, cw = h // 2, w // 2
    ycc = forward_pixels(rgb, spec, clamp)
    if chroma_down == 'box':
        c2 = box_chroma(rgb, spec, clamp)
        u, v = c2[..., 0], c2[..., 1]
    else:
        u, v = ycc[:, ::2, ::2, 1][:, :ch, :cw], ycc[:, ::2, ::2, 2][:, :ch, :cw]
    return np.ascontiguousarray(ycc[..., 0]), np.ascontiguousarray(u), np.ascontiguousarray(v)


def inverse_pixels(ycc, spec, clamp=True):
    """uint8 [..., 3] (Y, Cb, Cr) -> [..., 3] (R, G, B) of every pixel: uint8, or with clamp=False the int32 values in front of
    the clamp"""
    c = coefficients(spec)
    cy, rv, gu, gv, bu = c.inv
    p = np.asarray(ycc).astype(np.int32)
    yy = cy * (p[..., 0] - c.inv_yoff) + (1 << (SHIFT - 1))
    cb, cr = p[..., 1] - 128, p[..., 2] - 128
    out = np.empty(p.shape, np.int32)
    out[..., 0] = (yy + rv * cr) >> SHIFT
    out[..., 1] = (yy + gu * cb + gv * cr) >> SHIFT
    out[..., 2] = (yy + bu * cb) >> SHIFT
    return _clamp8(out, clamp)


def inverse_numpy(y, u, v, spec, chroma_shift=1, clamp=True):
    """uint8 planes y [n, h, w], u and v [n, ch, cw] -> [n, h, w, 3]: what aivc_yuv8_to_rgb8_matrix must equal.  chroma_shift 1:
    pixel (i, j) reads chroma sample (min(i // 2, ch - 1), min(j // 2, cw - 1)); 0: full-resolution chroma"""
    y, u, v = np.asarray(y), np.asarray(u), np.asarray(v)
    n, h, w = y.shape
    ch, cw = u.shape[1:]
    if chroma_shift not in (0, 1) or u.shape != v.shape or u.shape[0] != n or ch * cw == 0 \
            or (chroma_shift == 0 and (ch, cw) != (h, w)) or (chroma_shift == 1 and (ch < h // 2 or cw < w // 2)):
        raise ValueError('inverse_numpy: planes %s / %s / %s at chroma_shift %r' % (y.shape, u.shape, v.shape, chroma_shift))
    ii = np.minimum(np.arange(h) >> chroma_shift, ch - 1)
    jj = np.minimum(np.arange(w) >> chroma_shift, cw - 1)
    return inverse_pixels(np.stack([y, u[:, ii][:, :, jj], v[:, ii][:, :, jj]], axis=-1), spec, clamp)


# ---- the device ------------------------------------------------------------------------------------------------------------
def _struct(spec):
    """the aivc_color_matrix of a spec: a host structure, read by the library before the call returns"""
    from . import abi
    c = coefficients(spec)
    m = abi.ColorMatrix()
    for i in range(3):
        for j in range(3):
            m.fwd[i][j] = c.fwd[i][j]
        m.fwd_off[i] = c.fwd_off[i]
    for i in range(5):
        m.inv[i] = c.inv[i]
    m.inv_yoff = c.inv_yoff
    return m


def _plane(t, name, shape):
    """a uint8 CUDA tensor of this shape (None on an axis: any size but zero) as the kernels take it: contiguous (a strided view
    is copied, like every input of aivc_amd.ops)"""
    import torch
    from . import ops
    if not isinstance(t, torch.Tensor):
        raise ValueError('aivc_amd.color: %s is %s, expected a tensor' % (name, type(t).__name__))
    t = ops._shaped(t, torch.uint8, shape, name)
    if t.numel() == 0:
        raise ValueError('aivc_amd.color: %s has shape %s: no pixels' % (name, tuple(t.shape)))
    return t


def rgb_to_yuv420(rgb, spec, chroma_down='point'):
    """interleaved uint8 RGB [n, h, w, 3] on the device -> uint8 planes y [n, h, w], u and v [n, h // 2, w // 2] under `spec`
    (forward_numpy byte for byte; aivc_rgb8_to_yuv420u8_matrix on torch's current stream).  The shapes are those of
    ops.rgb8_to_yuv420u8: FLOOR-sized chroma planes."""
    from . import ops
    torch = ops.torch  # (the allocations of a guarded test run go through the same proxy as those of aivc_amd.ops)
    m = _struct(spec)
    down = CHROMA_DOWN.index(check_chroma_down(chroma_down))
    rgb = _plane(rgb, 'rgb', (None, None, None, 3))
    n, h, w, _ = rgb.shape
    y = torch.empty((n, h, w), dtype=torch.uint8, device=rgb.device)
    u = torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=rgb.device)
    v = torch.empty((n, h // 2, w // 2), dtype=torch.uint8, device=rgb.device)
    empty = u.numel() == 0
    ops._hbm_profiled('rgb8_to_yuv420u8_matrix', n * (h * w * 4 + 2 * (h // 2) * (w // 2)),
                      lambda: ops.call('aivc_rgb8_to_yuv420u8_matrix', ops._p(rgb), n, h, w, C.byref(m), down, ops._p(y),
                                       None if empty else ops._p(u), None if empty else ops._p(v), ops._stream()))
    return y, u, v


def yuv_to_rgb(y, u, v, spec, chroma_shift=1):
    """uint8 planes y [n, h, w], u and v [n, ch, cw] on the device -> interleaved uint8 RGB [n, h, w, 3] under `spec`
    (inverse_numpy byte for byte; aivc_yuv8_to_rgb8_matrix on torch's current stream).  chroma_shift and the plane sizes are
    those of ops.yuv8_to_rgb8: 1 -- half-resolution chroma of the floor or the ceil size, nearest x 2 and cropped; 0 -- full."""
    from . import ops
    torch = ops.torch
    m = _struct(spec)
    if chroma_shift not in (0, 1):
        raise ValueError('yuv_to_rgb: chroma_shift %r (expected 0 or 1)' % (chroma_shift,))
    y = _plane(y, 'y', (None, None, None))
    n, h, w = y.shape
    u = _plane(u, 'u', (n, None, None))
    ch, cw = u.shape[1:]
    v = _plane(v, 'v', (n, ch, cw))
    if (chroma_shift == 0 and (ch, cw) != (h, w)) or (chroma_shift == 1 and (ch < h // 2 or cw < w // 2)):
        raise ValueError('yuv_to_rgb: chroma planes %d x %d for luma %d x %d at chroma_shift %d' % (cw, ch, w, h, chroma_shift))
    rgb = torch.empty((n, h, w, 3), dtype=torch.uint8, device=y.device)
    ops._hbm_profiled('yuv8_to_rgb8_matrix', n * (h * w * 4 + 2 * ch * cw),
                      lambda: ops.call('aivc_yuv8_to_rgb8_matrix', ops._p(y), ops._p(u), ops._p(v), n, h, w, ch, cw, chroma_shift,
                                       C.byref(m), ops._p(rgb), ops._stream()))
    return rgb
