"""The statements the raw video tests share (not a test module): the arithmetic of include/aivc_hip_rawvideo.h restated in numpy,
with a format table, a frame generator and a .y4m writer of their own -- nothing here imports the code under test.

Ingest, to 8-bit 4:2:0 with ceil-sized chroma: a sample's value is its byte, its little-endian word, or word >> (16 - depth)
where the bits sit at the top; luma is one tap; chroma (j, i) is the exact sum s of the t samples at rows min(ty j + a, rows - 1),
columns min(tx i + b, cols - 1) one 4:2:0 sample covers; with sh = depth - 8 + log2 t: out = s if sh == 0 else
min(255, (s + (1 << (sh - 1))) >> sh).  Grey gives chroma 128.  Export: v << (depth - 8), << (16 - depth) again at the top."""
import numpy as np

# name -> (bytes per sample, depth, bits at the top, shift_x, shift_y, arrangement: '' grey, 'p' planar, 'uv', 'vu')
FORMATS = {'gray': (1, 8, 0, 1, 1, ''), 'nv12': (1, 8, 0, 1, 1, 'uv'), 'nv21': (1, 8, 0, 1, 1, 'vu'),
           'p010le': (2, 10, 1, 1, 1, 'uv'), 'p016le': (2, 16, 1, 1, 1, 'uv')}
for _sub, _sx, _sy in (('420', 1, 1), ('422', 1, 0), ('444', 0, 0)):
    FORMATS['yuv%sp' % _sub] = (1, 8, 0, _sx, _sy, 'p')
    for _d in (10, 12, 16):
        FORMATS['yuv%sp%dle' % (_sub, _d)] = (2, _d, 0, _sx, _sy, 'p')
        FORMATS['gray%dle' % _d] = (2, _d, 0, 1, 1, '')
WRITABLE = sorted(n for n, f in FORMATS.items() if f[5] == '' or (f[3], f[4]) == (1, 1))
Y4M_TAGS = {'yuv420p': '420', 'yuv422p': '422', 'yuv444p': '444', 'gray': 'mono'}
for _d in (10, 12, 16):
    Y4M_TAGS.update({'yuv420p%dle' % _d: '420p%d' % _d, 'yuv422p%dle' % _d: '422p%d' % _d, 'yuv444p%dle' % _d: '444p%d' % _d,
                     'gray%dle' % _d: 'mono%d' % _d})


def ceil_shift(n, s):
    return -(-n >> s)


def planes_of(name, w, h, pad=0):
    """-> ([(byte offset, row pitch, rows, samples per row)] per plane of the layout, bytes per frame); rows are tight + pad bytes"""
    b, _, _, sx, sy, arr = FORMATS[name]
    cw, ch = ceil_shift(w, sx), ceil_shift(h, sy)
    shapes = [(h, w)] + {'': [], 'p': [(ch, cw)] * 2}.get(arr, [(ch, 2 * cw)])
    out, at = [], 0
    for rows, cols in shapes:
        out.append((at, cols * b + pad, rows, cols))
        at += (cols * b + pad) * rows
    return out, at - pad


def frame_bytes(name, w, h):
    return planes_of(name, w, h)[1]


def _get(buf, plane, b):
    off, pitch, rows, cols = plane
    a = np.stack([buf[off + r * pitch:off + r * pitch + cols * b] for r in range(rows)])
    return a.astype(np.int64) if b == 1 else a[:, 0::2].astype(np.int64) | (a[:, 1::2].astype(np.int64) << 8)


def _put(buf, plane, b, words):
    off, pitch, rows, cols = plane
    for r in range(rows):
        row = words[r].astype(np.int64)
        raw = row.astype(np.uint8) if b == 1 else np.stack([row & 255, row >> 8], 1).reshape(-1).astype(np.uint8)
        buf[off + r * pitch:off + r * pitch + cols * b] = raw


def _round(s, sh):
    if sh == 0:
        assert s.max() <= 255
        return s.astype(np.uint8)
    return np.minimum(255, (s + (1 << (sh - 1))) >> sh).astype(np.uint8)


def ingest(buf, name, w, h, pad=0):
    """one frame's bytes (uint8 array) -> y [h, w], u, v [ceil(h/2), ceil(w/2)] uint8"""
    b, depth, top, sx, sy, arr = FORMATS[name]
    planes, total = planes_of(name, w, h, pad)
    assert buf.dtype == np.uint8 and buf.size >= total

    def values(p):
        words = _get(buf, p, b)
        return words >> (16 - depth) if top else words
    y = _round(values(planes[0]), depth - 8)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    if arr == '':
        return y, np.full((hc, wc), 128, np.uint8), np.full((hc, wc), 128, np.uint8)
    if arr == 'p':
        cu, cv = values(planes[1]), values(planes[2])
    else:
        both = values(planes[1])
        cu, cv = (both[:, 0::2], both[:, 1::2]) if arr == 'uv' else (both[:, 1::2], both[:, 0::2])
    tx, ty = 2 >> sx, 2 >> sy
    rows = np.minimum(ty * np.arange(hc)[:, None] + np.arange(ty)[None, :], cu.shape[0] - 1)  # [hc, ty]
    cols = np.minimum(tx * np.arange(wc)[:, None] + np.arange(tx)[None, :], cu.shape[1] - 1)  # [wc, tx]
    sh = depth - 8 + (1 - sx) + (1 - sy)
    u, v = (_round(c[rows[:, None, :, None], cols[None, :, None, :]].sum((2, 3)), sh) for c in (cu, cv))
    return y, u, v


def export(y, u, v, name):
    """8-bit 4:2:0 planes -> one tight frame's bytes in a 4:2:0 or grey layout"""
    b, depth, top, sx, sy, arr = FORMATS[name]
    assert arr == '' or (sx, sy) == (1, 1)
    h, w = y.shape
    planes, total = planes_of(name, w, h)
    buf = np.zeros(total, np.uint8)
    up = (depth - 8) + (16 - depth if top else 0)
    _put(buf, planes[0], b, y.astype(np.int64) << up)
    if arr == 'p':
        _put(buf, planes[1], b, u.astype(np.int64) << up)
        _put(buf, planes[2], b, v.astype(np.int64) << up)
    elif arr:
        first, second = (u, v) if arr == 'uv' else (v, u)
        _put(buf, planes[1], b, np.stack([first, second], 2).reshape(first.shape[0], -1).astype(np.int64) << up)
    return buf


def make_frame(name, w, h, rng, pad=0):
    """One frame's bytes with every plane random and, planted: in the chroma planes of 4:2:2 / 4:4:4, pairs and quads whose sums
    sit on, just below and just above a rounding tie; in every plane 0, the format's maximum, for LSB-aligned 16-bit layouts
    words with garbage above the depth (0xFFFF, and the bit just above it), and values on both sides of every rounding tie
    of a single sample: dropped bits 0...01, 01...1, 10...0 and 10...01.  The bytes between a tight row and the pitch are random."""
    b, depth, top, sx, sy, arr = FORMATS[name]
    planes, total = planes_of(name, w, h, pad)
    buf = rng.integers(0, 256, total, dtype=np.uint8)
    peak = (1 << depth) - 1
    lift = 16 - depth if top else 0
    drop = depth - 8
    for k, p in enumerate(planes):
        rows, cols = p[2], p[3]
        a = rng.integers(0, 1 << (8 * b), (rows, cols), dtype=np.int64) if top else rng.integers(0, peak + 1, (rows, cols), dtype=np.int64)
        step = 2 if (k and arr in ('uv', 'vu')) else 1  # samples of one component
        tx, ty = ((2 >> sx), (2 >> sy)) if k else (1, 1)
        sh = drop + (tx * ty).bit_length() - 1
        if k and sh and tx * ty > 1:
            targets = [1 << (sh - 1), (1 << (sh - 1)) - 1, (1 << (sh - 1)) + 1]
            blocks = [(j, i) for j in range(rows // ty) for i in range(cols // (tx * step))][:6]
            for n, (j, i) in enumerate(blocks):
                q = int(rng.integers(0, peak // 2 + 1))
                a[ty * j:ty * j + ty, tx * step * i:tx * step * (i + 1):step] = q << lift
                delta = (targets[n % 3] - tx * ty * q) % (1 << sh)
                a[ty * j, tx * step * i] = (q + delta) << lift
        plant = [0, peak << lift]
        if b == 2 and not top and depth < 16:
            plant += [0xFFFF, (1 << depth) | 5]
        if drop:
            base = int(rng.integers(1, 200)) << drop
            plant += [(base | t) << lift for t in (1, (1 << (drop - 1)) - 1, 1 << (drop - 1), (1 << (drop - 1)) | 1)]
        flat = a.reshape(-1)
        m = min(len(plant), flat.size)
        flat[flat.size - m:] = plant[:m]  # (from the back: the blocks above sit at the front)
        _put(buf, p, b, a)
    return buf


def write_y4m(path, name, w, h, frames, fps=(30, 1), header_extra='', frame_params='', interlace='Ip', tag=None):
    """frames: a list of uint8 arrays, each one tight frame of the layout `name` -> a .y4m file.  header_extra: appended to the
    header line (e.g. ' XYSCSS=420P10', or padding that moves frame 0 to an odd byte), frame_params: to every FRAME line."""
    tag = Y4M_TAGS[name] if tag is None else tag
    head = 'YUV4MPEG2 W%d H%d F%d:%d %s A1:1' % (w, h, fps[0], fps[1], interlace) + (' C%s' % tag if tag else '') + header_extra
    with open(path, 'wb') as f:
        f.write(' '.join(head.split(' ')).replace('  ', ' ').encode() + b'\n')
        for fr in frames:
            f.write(b'FRAME' + frame_params.encode() + b'\n')
            f.write(np.asarray(fr, np.uint8).tobytes())
    return path


def read_y4m(path):
    """a small independent parser for what the product WRITES: -> (header tokens, [frame bytes as uint8 arrays]); the frame size in
    bytes comes from the caller-visible tag through FORMATS"""
    data = open(path, 'rb').read()
    end = data.index(b'\n')
    toks = data[:end].decode().split(' ')
    assert toks[0] == 'YUV4MPEG2'
    kv = {t[0]: t[1:] for t in toks[1:]}
    name = {v: k for k, v in Y4M_TAGS.items()}[kv.get('C', '420')]
    w, h = int(kv['W']), int(kv['H'])
    size = frame_bytes(name, w, h)
    frames, at = [], end + 1
    while at < len(data):
        nl = data.index(b'\n', at)
        assert data[at:at + 5] == b'FRAME'
        frames.append(np.frombuffer(data[nl + 1:nl + 1 + size], np.uint8))
        assert frames[-1].size == size
        at = nl + 1 + size
    return toks, name, w, h, frames
