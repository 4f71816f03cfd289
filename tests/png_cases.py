"""The statements the PNG tests share (not a test module): pictures, the row filters restated in numpy, a stand-in zlib stream made
of independent segments, and what every coded picture is checked against -- Pillow reading the file and zlib inflating its IDAT.
Nothing here imports the code under test but for check_file's caller handing it the file."""
import io
import struct
import zlib

import numpy as np

TARGET = 16384  # the segment rule restated: whole rows, about this many filtered bytes, at least one row

# (h, w) of the geometry cases, each with c = 1 and c = 3: row bytes that are no multiple of 4, pictures of one segment, single
# rows and columns; and 129 x 127: grey rows of 128 bytes, 128 to a segment, so a last segment of ONE row (RGB: 42 + 42 + 42 + 3)
GEOMETRY = [(1, 1), (1, 37), (37, 1), (38, 70), (64, 64), (129, 127)]
LONG_ROW = (3, 6000, 3)  # a row of 18001 bytes: longer than the target, a segment of its own


def rows_per_segment(h, w, c):
    return min(h, max(1, TARGET // (1 + w * c)))


def segment_lengths(h, w, c):
    rows, row = rows_per_segment(h, w, c), 1 + w * c
    return [min(rows, h - r) * row for r in range(0, h, rows)]


def random_picture(h, w, c, seed):
    """smooth in places, noisy in others, so that every filter type wins some rows"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = (xx * 3 + yy * 5)[..., None] + np.arange(c) * 40
    noise = rng.integers(0, 256, (h, w, c)) * (rng.random((h, 1, 1)) < 0.3)
    return ((base + noise) % 256).astype(np.uint8)


def analytic_picture(h, w, sigma, seed=1):
    """the measurement picture: an analytic RGB picture (a gradient, two sinusoids, a disc) plus Gaussian noise of `sigma` levels"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    r = 128 + 60 * np.sin(xx / 97.0) + 40 * np.cos(yy / 61.0)
    g = 255.0 * xx / max(w - 1, 1) * 0.5 + 255.0 * yy / max(h - 1, 1) * 0.5
    b = 90 + 80 * np.sin((xx + yy) / 143.0) + 50 * (((xx - w / 2) ** 2 + (yy - h / 2) ** 2) < (min(h, w) / 4) ** 2)
    pic = np.stack([r, g, b], -1)
    if sigma:
        pic = pic + rng.normal(0.0, sigma, pic.shape)
    return np.clip(np.rint(pic), 0, 255).astype(np.uint8)


def fibonacci_picture(seed=5):
    """grey 128 x 127, filter 0: ONE segment of 16384 bytes whose pixel values 1, 2, 3, ... occur 1, 1, 2, 3, 5, ... times (the last
    value takes what is left), shuffled: an unlimited Huffman tree for it is deeper than 15"""
    h, w = 128, 127
    vals, a, b, v = [], 1, 1, 1
    while len(vals) + a <= h * w:
        vals += [v] * a
        a, b, v = b, a + b, v + 1
    vals += [v] * (h * w - len(vals))
    assert v >= 18  # (18 Fibonacci weights and more: the two-queue tree is a chain deeper than 15)
    arr = np.array(vals, np.uint8)
    np.random.default_rng(seed).shuffle(arr)
    return arr.reshape(h, w, 1)


def all_values_picture(seed=6):
    """grey 63 x 256, filter 0: one segment in which every pixel value occurs 63 times"""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(256) for _ in range(63)]).astype(np.uint8)[..., None]


# ---- the filters, restated -------------------------------------------------------------------------------------------------------
def filter_rows(pix, types):
    """pix [h, w, c] uint8, types: one filter type per row -> the filtered stream [h, 1 + w c] uint8 (PNG specification, 9.2)"""
    h, w, c = pix.shape
    x = pix.reshape(h, w * c).astype(np.int64)
    a = np.zeros_like(x)
    a[:, c:] = x[:, :-c] if w > 1 else 0
    b = np.zeros_like(x)
    b[1:] = x[:-1]
    d = np.zeros_like(x)
    d[1:, c:] = x[:-1, :-c] if w > 1 else 0
    p = a + b - d
    pa, pb, pd = np.abs(p - a), np.abs(p - b), np.abs(p - d)
    paeth = np.where((pa <= pb) & (pa <= pd), a, np.where(pb <= pd, b, d))
    pred = np.stack([np.zeros_like(x), a, b, (a + b) // 2, paeth])
    types = np.asarray(types)
    out = np.empty((h, 1 + w * c), np.uint8)
    out[:, 0] = types
    out[:, 1:] = (x - pred[types, np.arange(h)]) % 256
    return out


def unfilter_types(filtered, h, w, c):
    return filtered.reshape(h, 1 + w * c)[:, 0]


def adaptive_types(pix):
    """filter 5: per row the type whose residuals, as signed bytes, have the smallest sum of absolute values; the lowest among equals"""
    h = pix.shape[0]
    cost = np.stack([np.abs(filter_rows(pix, np.full(h, t))[:, 1:].view(np.int8).astype(np.int64)).sum(1) for t in range(5)])
    return cost.argmin(0)  # (argmin takes the first of equals)


# ---- streams ------------------------------------------------------------------------------------------------------------------------
def stitched_stream(filtered, lengths, strategy=zlib.Z_RLE, level=6):
    """a zlib stream of independent segments: each a raw deflate of its own ended by a sync flush, then the final empty stored
    block and the Adler-32 of everything"""
    data = bytes(filtered)
    assert sum(lengths) == len(data)
    out, at = [b'\x78\x01'], 0
    for n in lengths:
        co = zlib.compressobj(level, zlib.DEFLATED, -15, 9, strategy)
        out.append(co.compress(data[at:at + n]) + co.flush(zlib.Z_SYNC_FLUSH))
        at += n
    out.append(b'\x01\x00\x00\xff\xff' + struct.pack('>I', zlib.adler32(data) & 0xffffffff))
    return b''.join(out)


def chunks(png):
    """the file -> [(kind, data)], every CRC checked"""
    assert png[:8] == b'\x89PNG\r\n\x1a\n'
    out, at = [], 8
    while at < len(png):
        n, = struct.unpack('>I', png[at:at + 4])
        kind, data = png[at + 4:at + 8], png[at + 8:at + 8 + n]
        assert struct.unpack('>I', png[at + 8 + n:at + 12 + n])[0] == zlib.crc32(kind + data) & 0xffffffff
        out.append((kind, data))
        at += 12 + n
    assert at == len(png)
    return out


def check_file(png, pix, filter=None):
    """everything a coded picture owes: Pillow verifies it and reads the pixels back exactly; it is signature, IHDR, ONE IDAT, IEND;
    the IDAT inflates to h (1 + w c) bytes whose filter bytes are the requested type (0 ... 4), or lie in 0 ... 4 (5, None).
    -> the filtered stream"""
    from PIL import Image
    h, w, c = pix.shape
    Image.open(io.BytesIO(png)).verify()
    img = Image.open(io.BytesIO(png))
    assert img.mode == ('L' if c == 1 else 'RGB') and img.size == (w, h)
    assert np.array_equal(np.asarray(img).reshape(h, w, c), pix)
    parts = chunks(png)
    assert [k for k, _ in parts] == [b'IHDR', b'IDAT', b'IEND']
    assert parts[0][1] == struct.pack('>IIBBBBB', w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    filtered = zlib.decompress(parts[1][1])
    assert len(filtered) == h * (1 + w * c)
    types = unfilter_types(np.frombuffer(filtered, np.uint8), h, w, c)
    if filter in (0, 1, 2, 3, 4):
        assert (types == filter).all()
    else:
        assert types.max() <= 4
    return filtered
