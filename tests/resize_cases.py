"""The shapes, inputs and the numpy statement of the resize tests (tests/test_resize_coeffs.py, tests/test_gpu_resize.py,
tests/test_gpu_resize_cli.py), each stated once.  Not a test module.  Builders make no device tensor.

The statement restates Pillow's 8-bit Image.resize on an 'L' picture (reducing_gap=None, the whole picture as box) without
looking at aivc_amd/resize.py; the reference of every comparison is Pillow itself (pil_resize), and every comparison is equality.

One axis, n_in -> n_out, filter f of support S:  scale = n_in / n_out, fs = max(scale, 1), support = S fs, ss = 1 / fs; for output
xx: c = (xx + 0.5) scale, xmin = max(int(c - support + 0.5), 0), xmax = min(int(c + support + 0.5), n_in) - xmin,
k[x] = f((x + xmin - c + 0.5) ss), ww their sum in index order, k[x] /= ww when ww != 0, K = int(+-0.5 + k 2^22) by the sign of k,
out = clip((2^21 + sum in[xmin + x] K[x]) >> 22, 0, 255) in int32.  Horizontal pass first, its result ROUNDED TO uint8, then the
vertical pass; a pass whose axis keeps its size is skipped."""
import functools
import math

import numpy as np

FILTER_NAMES = ['box', 'bilinear', 'hamming', 'bicubic', 'lanczos']

# (h_in, w_in, h_out, w_out, kind of content)
SHAPES = [
    (1, 1, 4, 4, 'random'),          # smallest input
    (7, 9, 3, 4, 'random'),          # small downscale
    (5, 5, 11, 13, 'random'),        # upscale
    (16, 16, 16, 8, 'random'),       # one pass only
    (33, 61, 17, 30, 'random'),      # odd sizes
    (2, 300, 2, 7, 'random'),        # 257 taps on the horizontal axis (lanczos)
    (40, 64, 23, 97, 'extremes'),    # pixels drawn from {0, 255}: both clips, negative lobes
    (135, 240, 68, 120, 'random'),   # codec-sized downscale
    (270, 480, 540, 960, 'random'),  # several workgroups, upscale
    (200, 333, 77, 129, 'random'),   # width not a multiple of 4, tile edges on both axes
    (9, 9, 9, 9, 'random'),          # no pass: a copy
]


def shape_id(s):
    return '%dx%d-%dx%d' % s[:4]


def planes(shape, n, seed=0):
    """n different uint8 planes [h_in, w_in] of a shape's kind of content"""
    h, w, _, _, kind = shape
    rng = np.random.default_rng([h, w, shape[2], shape[3], seed])
    if kind == 'extremes':
        return [(rng.integers(0, 2, (h, w)) * 255).astype(np.uint8) for _ in range(n)]
    return [rng.integers(0, 256, (h, w), dtype=np.uint8) for _ in range(n)]


def pil_filter(name):
    from PIL import Image
    return getattr(Image.Resampling, name.upper())


def pil_resize(plane, h_out, w_out, name):
    """the reference: Image.resize of one uint8 plane [h, w] -> [h_out, w_out]"""
    from PIL import Image
    return np.asarray(Image.fromarray(np.ascontiguousarray(plane), 'L').resize((w_out, h_out), pil_filter(name)))


@functools.lru_cache(maxsize=None)
def pil_planes(shape, n, name, seed=0):
    """Pillow's resize of planes(shape, n, seed), computed once per session"""
    out = tuple(pil_resize(p, shape[2], shape[3], name) for p in planes(shape, n, seed))
    for a in out:
        a.setflags(write=False)
    return out


def pil_resize_frame(fr, w, h, name):
    """a 4:2:0 frame {'y','u','v'} of planes [h, w] / [1, h, w] to w x h: y to h x w, u and v to ceil(h / 2) x ceil(w / 2), each
    plane on its own (what resizing each picture of a PNG triplet gives) -> planes of the rank that came in"""
    out = {}
    for k in 'yuv':
        p = np.asarray(fr[k])
        hh, ww = (h, w) if k == 'y' else ((h + 1) // 2, (w + 1) // 2)
        out[k] = pil_resize(p.reshape(p.shape[-2:]), hh, ww, name).reshape(p.shape[:-2] + (hh, ww))
    return out


# ---- the numpy statement ------------------------------------------------------------------------------------------------

def _sinc(x):
    if x == 0.0:
        return 1.0
    t = x * math.pi
    return math.sin(t) / t


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    t = x * math.pi
    return math.sin(t) / t * (0.54 + 0.46 * math.cos(t))


def _bicubic(x):
    a, x = -0.5, abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


STATEMENT_FILTERS = {
    'box': (0.5, lambda x: 1.0 if -0.5 < x <= 0.5 else 0.0),
    'bilinear': (1.0, lambda x: 1.0 - abs(x) if abs(x) < 1.0 else 0.0),
    'hamming': (1.0, _hamming),
    'bicubic': (2.0, _bicubic),
    'lanczos': (3.0, lambda x: _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0),
}


@functools.lru_cache(maxsize=None)
def statement_axis(n_in, n_out, name):
    """-> [(xmin, [K ...])] per output index"""
    S, f = STATEMENT_FILTERS[name]
    scale = n_in / n_out
    fs = max(scale, 1.0)
    support, ss = S * fs, 1.0 / fs
    rows = []
    for xx in range(n_out):
        c = (xx + 0.5) * scale
        xmin = max(int(c - support + 0.5), 0)
        xmax = min(int(c + support + 0.5), n_in) - xmin
        k = np.array([f((x + xmin - c + 0.5) * ss) for x in range(xmax)], np.float64)
        ww = 0.0
        for v in k:
            ww += float(v)
        if ww != 0.0:
            k = k / ww
        rows.append((xmin, [int(0.5 + v * (1 << 22)) if v >= 0 else int(-0.5 + v * (1 << 22)) for v in k.tolist()]))
    return rows


def statement_pass(a, n_out, name):
    """the pass along the LAST axis of the uint8 array a"""
    out = np.empty(a.shape[:-1] + (n_out,), np.uint8)
    for xx, (xmin, K) in enumerate(statement_axis(a.shape[-1], n_out, name)):
        acc = (a[..., xmin:xmin + len(K)].astype(np.int64) * np.asarray(K, np.int64)).sum(-1) + (1 << 21)
        assert np.abs(acc).max(initial=0) < 1 << 31  # an int32 accumulator holds it
        out[..., xx] = np.clip(acc >> 22, 0, 255)
    return out


def statement_resize(plane, h_out, w_out, name):
    a = np.ascontiguousarray(plane)
    if a.shape[1] != w_out:
        a = statement_pass(a, w_out, name)
    if a.shape[0] != h_out:
        a = np.ascontiguousarray(statement_pass(np.ascontiguousarray(a.T), h_out, name).T)
    return a
