"""The statements the tests of the device PNG reader share (not a test module): zlib streams, valid and damaged, built by zlib and
by hand with a small deflate bit writer; filtered pictures; PNG files.  Every valid stream round-trips through zlib.decompress
and every damaged one is refused by it (or gives another length) when this module is imported, on the CPU.  Nothing here imports
the code under test but for png.assemble, which writes two of the files."""
import io
import struct
import zlib

import numpy as np

import png_cases as pcs

# ---- deflate, written by hand ---------------------------------------------------------------------------------------------------------
LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0] * 8 + [1] * 4 + [2] * 4 + [3] * 4 + [4] * 4 + [5] * 4 + [0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193,
             12289, 16385, 24577]
DIST_EXTRA = [0, 0, 0, 0] + [e for e in range(1, 14) for _ in (0, 1)]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
# what the hand-made VALID streams use, noted as they are written
USED = {'types': set(), 'len': set(), 'dist': set(), 'cl': set(), 'maxbits': 0}


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, value, count):  # least significant bit first
        assert 0 <= value < 1 << count
        self.acc |= value << self.n
        self.n += count
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, pair):  # a Huffman code: most significant bit first
        code, length = pair
        self.bits(int(format(code, '0%db' % length)[::-1], 2), length)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def raw(self, data):
        assert self.n == 0
        self.out += data


def canonical(lengths):
    """code lengths per symbol -> {symbol: (code, length)} (RFC 1951, 3.2.2)"""
    codes, code = {}, 0
    for length in range(1, 16):
        for sym, l in enumerate(lengths):
            if l == length:
                codes[sym] = (code, length)
                code += 1
        code <<= 1
    return codes


FIXED_LIT = canonical([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8)
FIXED_DIST = {s: (s, 5) for s in range(32)}


def length_token(length, hi=False):
    """-> (symbol, extra bits, extra value); 258 as symbol 285, or -- hi -- as symbol 284 with extra 31"""
    if length == 258 and not hi:
        return 285, 0, 0
    sym = max(k for k in range(28) if LEN_BASE[k] <= length)
    return 257 + sym, LEN_EXTRA[sym], length - LEN_BASE[sym]


def dist_token(dist):
    sym = max(k for k in range(30) if DIST_BASE[k] <= dist)
    return sym, DIST_EXTRA[sym], dist - DIST_BASE[sym]


class Block:
    """the tokens of one Huffman block; note=False for damaged streams, which prove nothing about coverage"""

    def __init__(self, w, lit, dist, note=True):
        self.w, self.lit, self.dist, self.note = w, lit, dist, note

    def literal(self, b):
        self.w.code(self.lit[b])

    def literals(self, data):
        for b in data:
            self.w.code(self.lit[b])

    def match(self, length, dist, hi=False):
        sym, eb, ev = length_token(length, hi)
        self.w.code(self.lit[sym])
        self.w.bits(ev, eb)
        dsym, deb, dev = dist_token(dist)
        self.w.code(self.dist[dsym])
        self.w.bits(dev, deb)
        if self.note:
            USED['len'].add(sym)
            USED['dist'].add(dsym)

    def symbols(self, lit_sym=None, dist_sym=None):  # raw symbols (damaged streams)
        if lit_sym is not None:
            self.w.code(self.lit[lit_sym])
        if dist_sym is not None:
            self.w.code(self.dist[dist_sym])

    def end(self):
        self.w.code(self.lit[256])


def fixed_block(w, final, note=True):
    w.bits(1 if final else 0, 1)
    w.bits(1, 2)
    if note:
        USED['types'].add(1)
    return Block(w, FIXED_LIT, FIXED_DIST, note)


def stored_block(w, final, data, nlen=None, note=True):
    w.bits(1 if final else 0, 1)
    w.bits(0, 2)
    w.align()
    w.raw(struct.pack('<HH', len(data), (~len(data) & 0xffff) if nlen is None else nlen) + bytes(data))
    if note:
        USED['types'].add(0)


CL_LENS = [4] * 13 + [5] * 6  # a complete code-length code: 13/16 + 6/32 = 1


def run_length_tokens(lengths):
    """the code lengths -> [(code-length symbol, extra value)] with the repeat symbols wherever they fit"""
    out, i = [], 0
    while i < len(lengths):
        v, run = lengths[i], 1
        while i + run < len(lengths) and lengths[i + run] == v:
            run += 1
        i += run
        if v == 0:
            while run >= 11:
                take = min(run, 138)
                out.append((18, take - 11))
                run -= take
            if run >= 3:
                out.append((17, run - 3))
                run = 0
        else:
            out.append((v, 0))
            run -= 1
            while run >= 3:
                take = min(run, 6)
                out.append((16, take - 3))
                run -= take
        out += [(v, 0)] * run
    return out


def dynamic_block(w, final, lit_lens, dist_lens, tokens=None, note=True):
    """the header of a dynamic block (tokens: the code-length tokens instead of the ones the lengths give) -> Block"""
    w.bits(1 if final else 0, 1)
    w.bits(2, 2)
    w.bits(len(lit_lens) - 257, 5)
    w.bits(len(dist_lens) - 1, 5)
    w.bits(19 - 4, 4)
    for s in CL_ORDER:
        w.bits(CL_LENS[s], 3)
    cl = canonical(CL_LENS)
    for sym, extra in (run_length_tokens(list(lit_lens) + list(dist_lens)) if tokens is None else tokens):
        w.code(cl[sym])
        if sym >= 16:
            w.bits(extra, {16: 2, 17: 3, 18: 7}[sym])
            if note:
                USED['cl'].add(sym)
    if note:
        USED['types'].add(2)
        USED['maxbits'] = max([USED['maxbits']] + list(lit_lens) + list(dist_lens))
    return Block(w, canonical(lit_lens), canonical(dist_lens), note)


def zwrap(w, data=None, adler=None):
    """the deflate bits -> a zlib stream; the Adler-32 is that of `data`, or of what zlib makes of the bits"""
    w.align()
    raw = bytes(w.out)
    if adler is None:
        if data is None:
            data = zlib.decompressobj(-15).decompress(raw)
        adler = zlib.adler32(bytes(data)) & 0xffffffff
    return b'\x78\x9c' + raw + struct.pack('>I', adler)


# lit/len lengths of the general hand-made blocks: every literal 9 bits, end of block 2, the length symbols 257 ... 272 6 bits
PLAIN_LIT = [9] * 256 + [2] + [6] * 16
assert sum(2.0 ** -l for l in PLAIN_LIT) == 1.0


def _every_symbol_stream():
    """fixed codes: 32768 literals, then a match for every length symbol at its lowest and highest length and for every distance
    symbol at its lowest and highest distance; more than 64 KiB, so a 32 KiB ring wraps twice"""
    rng = np.random.default_rng(11)
    w = BitWriter()
    b = fixed_block(w, True)
    n = 0
    spans = []

    def match(length, dist, hi=False):
        nonlocal n
        assert dist <= n
        b.match(length, dist, hi)
        spans.append((n, n + length))
        n += length
    b.literals(rng.integers(0, 256, 32768).astype(np.uint8).tobytes())
    n = 32768
    for k in range(29):
        lo = LEN_BASE[k]
        hi = 258 if k == 28 else lo + (1 << LEN_EXTRA[k]) - 1
        match(lo, 1 + 37 * k)
        match(hi, 32768 - 113 * k, hi=(k == 27))  # (symbol 284 with all extra bits set is 258 too)
    match(258, 32768)
    match(258, 2)
    match(258, 3)
    fill = 2 * 32768 - 100 - n  # the next match lies across the ring's second wrap
    assert fill > 0
    b.literals(rng.integers(0, 256, fill).astype(np.uint8).tobytes())
    n += fill
    for k in range(30):
        lo = DIST_BASE[k]
        hi = lo + (1 << DIST_EXTRA[k]) - 1
        match(258, lo)
        match(257 - k, hi)
    b.literals(b'the end')
    n += 7
    b.end()
    assert n > 65536 + 4096 and any(a < 32768 * 2 < e for a, e in spans), 'a match straddles the second wrap of a 32 KiB ring'
    return zwrap(w)


def _fibonacci_stream():
    """a dynamic block whose literal/length code is the chain 1, 2, ..., 14, 15, 15 bits -- what Fibonacci-weighted counts give
    (png_cases.fibonacci_picture for the writer) -- and no distance code"""
    syms = list(range(97, 112)) + [256]
    lit = [0] * 257
    for k, s in enumerate(syms):
        lit[s] = min(k + 1, 15)
    data, a, c = [], 1, 1
    for s in reversed(syms[:-1]):  # the longest code the fewest times
        data += [s] * a
        a, c = c, a + c
    data = np.array(data, np.uint8)
    np.random.default_rng(5).shuffle(data)
    w = BitWriter()
    b = dynamic_block(w, True, lit, [0])
    b.literals(data.tobytes())
    b.end()
    return zwrap(w)


def _repeat_symbols_stream():
    """a code-length alphabet with 16, 17 and 18: 32 zeros, 96 sevens, 4 zeros, 124 zeros, a two"""
    lit = [0] * 32 + [7] * 96 + [0] * 128 + [2]
    lit[128:132] = [0, 0, 0, 0]
    w = BitWriter()
    toks = [(18, 32 - 11), (7, 0)] + [(16, 3)] * 15 + [(7, 0)] * 5 + [(17, 4 - 3), (18, 124 - 11), (2, 0), (0, 0)]
    assert sum({16: 6, 17: 4}.get(s, e + 11 if s == 18 else 1) for s, e in toks) == 258
    b = dynamic_block(w, True, lit, [0], toks)
    b.literals(b'Lanes in lockstep walk one prefix code; the ring keeps what matches need.')
    b.end()
    return zwrap(w)


def _lone_distance_stream():
    """the only distance code has one entry of one bit: zlib's permitted incomplete set (distance symbol 4 alone)"""
    w = BitWriter()
    b = dynamic_block(w, True, PLAIN_LIT, [0, 0, 0, 0, 1])
    b.literals(b'abcdefgh')
    b.match(20, 5)
    b.match(3, 6)
    b.literals(b'xyz')
    b.end()
    return zwrap(w)


def _literals_only_stream():
    w = BitWriter()
    b = dynamic_block(w, True, PLAIN_LIT, [0])
    b.literals(bytes(range(256)) * 3)
    b.end()
    return zwrap(w)


def _stored_after_dynamic_stream():
    w = BitWriter()
    b = dynamic_block(w, False, PLAIN_LIT, [0, 1])
    b.literals(b'mid-byte')
    b.match(9, 2)
    b.end()
    assert w.n % 8 != 0, 'the dynamic block ends mid-byte'
    stored_block(w, True, b'stored bytes behind it')
    return zwrap(w)


def _empty_final_stored_stream():
    w = BitWriter()
    b = fixed_block(w, False)
    b.literals(b'what the writer of this project emits last')
    b.end()
    stored_block(w, True, b'')
    return zwrap(w)


def markov_text(n, seed=3):
    """n letters of a 6-letter alphabet, each drawn given the one before: many mid-range matches"""
    rng = np.random.default_rng(seed)
    p = rng.dirichlet(np.full(6, 0.4), 6).cumsum(1)
    u, out, s = rng.random(n), np.empty(n, np.uint8), 0
    for i in range(n):
        s = min(int(np.searchsorted(p[s], u[i])), 5)
        out[i] = 97 + s
    return out.tobytes()


def _zlib(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY):
    co = zlib.compressobj(level, zlib.DEFLATED, 15, 9, strategy)
    return co.compress(data) + co.flush()


def _valid_streams():
    rng = np.random.default_rng(2)
    random_bytes = rng.integers(0, 256, 70000).astype(np.uint8).tobytes()
    run = b'\x07' * 100000
    text = markov_text(200000)
    pic = pcs.analytic_picture(129, 127, 3)
    filtered = pcs.filter_rows(pic, pcs.adaptive_types(pic)).tobytes()
    out = [('stored-70000', _zlib(random_bytes, 0)), ('stored-1', _zlib(b'Z', 0))]
    USED['types'].add(0)
    for name, data in (('random', random_bytes), ('run', run), ('text', text), ('filtered', filtered)):
        for level in (1, 6, 9):
            out.append(('%s-level%d' % (name, level), _zlib(data, level)))
        for sname, strategy in (('rle', zlib.Z_RLE), ('fixed', zlib.Z_FIXED), ('huffman', zlib.Z_HUFFMAN_ONLY)):
            out.append(('%s-%s' % (name, sname), _zlib(data, 6, strategy)))
    out += [('every-symbol', _every_symbol_stream()), ('repeat-symbols', _repeat_symbols_stream()), ('fibonacci-15-bits', _fibonacci_stream()),
            ('lone-distance-code', _lone_distance_stream()), ('literals-only', _literals_only_stream()),
            ('stored-after-dynamic', _stored_after_dynamic_stream()), ('empty-final-stored', _empty_final_stored_stream())]
    pix = pcs.random_picture(129, 127, 1, seed=8)
    out.append(('stitched', pcs.stitched_stream(pcs.filter_rows(pix, pcs.adaptive_types(pix)).tobytes(), pcs.segment_lengths(129, 127, 1))))
    return out


# [(name, the stream, the bytes it inflates to)]
VALID = [(name, z, zlib.decompress(z)) for name, z in _valid_streams()]
assert USED['types'] == {0, 1, 2} and USED['len'] == set(range(257, 286)) and USED['dist'] == set(range(30)) \
    and USED['cl'] == {16, 17, 18} and USED['maxbits'] == 15, USED
assert [len(d) > 65536 for n, _, d in VALID if n == 'every-symbol'] == [True]


def _header(cmf, fdict=False, good=True):
    flg = next(f for f in range(256) if bool(f & 32) == fdict and ((cmf << 8 | f) % 31 == 0) == good)
    return bytes([cmf, flg])


def _bad_dynamic(lit, dist, tokens=None):
    w = BitWriter()
    b = dynamic_block(w, True, lit, dist, tokens, note=False)
    return w, b


def _damaged_streams():
    """[(name, stream, bytes expected)]"""
    valid = {n: (z, d) for n, z, d in VALID}
    out = []
    for name in ('text-level6', 'every-symbol'):
        z, d = valid[name]
        for cut in (0, 1, 2, 3, 10, len(z) // 2, len(z) - 4, len(z) - 1):  # (10: inside the header of text-level6's dynamic block)
            out.append(('%s-cut-%d' % (name, cut), z[:cut], len(d)))
    body = valid['stored-1'][0][2:]
    out.append(('cm-9', _header(0x79) + body, 1))
    out.append(('flg-check', _header(0x78, good=False) + body, 1))
    out.append(('fdict', _header(0x78, fdict=True) + body, 1))
    w = BitWriter()
    w.bits(1, 1), w.bits(3, 2)
    out.append(('block-type-3', zwrap(w, b''), 0))
    w = BitWriter()
    stored_block(w, True, b'abcd', nlen=0x1234, note=False)
    out.append(('stored-nlen', zwrap(w, b'abcd'), 4))
    w = BitWriter()
    w.bits(1, 3), w.align(), w.raw(struct.pack('<HH', 100, 0xffff - 100) + b'ten bytes.')
    out.append(('stored-past-the-end', b'\x78\x9c' + bytes(w.out), 100))
    w, b = _bad_dynamic([1, 1, 1] + [0] * 253 + [1], [0])
    out.append(('over-subscribed', zwrap(w, b''), 0))
    w, b = _bad_dynamic(PLAIN_LIT, [2, 2])
    b.literals(b'ab'), b.end()
    out.append(('incomplete-distances', zwrap(w, b'ab'), 2))
    w, b = _bad_dynamic(PLAIN_LIT, [0], [(16, 0)] + run_length_tokens(PLAIN_LIT + [0])[1:])
    out.append(('repeat-first', zwrap(w, b''), 0))
    w, b = _bad_dynamic(PLAIN_LIT, [0], run_length_tokens(PLAIN_LIT) + [(18, 5)])
    out.append(('lengths-past-the-end', zwrap(w, b''), 0))
    for name, lit_sym, dist_sym in (('literal-286', 286, None), ('distance-30', 257, 30)):
        w = BitWriter()
        b = fixed_block(w, True, note=False)
        b.literals(b'0123456789')
        b.symbols(lit_sym, dist_sym)
        b.end()
        out.append((name, zwrap(w, b'0123456789'), 10))
    w = BitWriter()
    b = fixed_block(w, True, note=False)
    b.match(3, 1), b.end()
    out.append(('distance-before-the-start', zwrap(w, b'aaa'), 3))
    w = BitWriter()
    b = fixed_block(w, True, note=False)
    b.literals(bytes(299)), b.match(5, 300), b.end()
    out.append(('distance-300-after-299', zwrap(w, bytes(304)), 304))
    z, d = valid['text-level6']
    out.append(('one-byte-longer', z, len(d) - 1))
    out.append(('one-byte-shorter', z, len(d) + 1))
    out.append(('trailer-bit', z[:-1] + bytes([z[-1] ^ 0x10]), len(d)))
    return out


DAMAGED = _damaged_streams()
for _name, _z, _expect in DAMAGED:
    try:
        assert len(zlib.decompress(_z)) != _expect, _name
    except zlib.error:
        pass

# ---- filtered pictures ------------------------------------------------------------------------------------------------------------------
SIZES = sorted({(h, w, c) for h, w in pcs.GEOMETRY + [(65, 33), (128, 5), (1, 1), pcs.LONG_ROW[:2]] for c in (1, 3)})
TYPE_MODES = (0, 1, 2, 3, 4, 'random')


def picture_cases(h, w, c):
    """[(pixels, the filtered rows)] of one size: every row of one type 0 ... 4, then seeded random types per row"""
    pix = pcs.random_picture(h, w, c, seed=h * 1000 + w * 3 + c)
    rng = np.random.default_rng(h + w + c)
    return [(pix, pcs.filter_rows(pix, rng.integers(0, 5, h) if mode == 'random' else np.full(h, mode))) for mode in TYPE_MODES]


def bad_type_picture():
    """(pixels, filtered rows with the type byte 5 in row 3)"""
    pix = pcs.random_picture(9, 11, 3, seed=77)
    filtered = pcs.filter_rows(pix, np.full(9, 1))
    filtered[3, 0] = 5
    return pix, filtered


# ---- files ----------------------------------------------------------------------------------------------------------------------------
def chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def _pillow_file(pix, **kw):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(pix[..., 0] if pix.shape[2] == 1 else pix).save(buf, 'PNG', **kw)
    return buf.getvalue()


def rechunk(png):
    """the same picture with its IDAT payload in chunks of ONE byte, a zero-length IDAT and a tEXt chunk among them.  Pillow ends
    the stream at the tEXt chunk and calls the file truncated, so the pixels this file is checked against are Pillow's of the file
    it was made from (PIXELS_FROM): the same IDAT payload, byte for byte."""
    parts = pcs.chunks(png)
    payload = b''.join(d for k, d in parts if k == b'IDAT')
    out = [b'\x89PNG\r\n\x1a\n', chunk(b'IHDR', parts[0][1])]
    for i, byte in enumerate(payload):
        out.append(chunk(b'IDAT', bytes([byte])))
        if i == 2:
            out += [chunk(b'IDAT', b''), chunk(b'tEXt', b'Comment\x00between the IDATs')]
    return b''.join(out + [chunk(b'IEND', b'')])


def adam7_file(pix):
    """an interlaced 8-bit file written by hand (Pillow writes none): the seven passes, every row of type 0"""
    h, w, c = pix.shape
    rows = []
    for x0, y0, dx, dy in ((0, 0, 8, 8), (4, 0, 8, 8), (0, 4, 4, 8), (2, 0, 4, 4), (0, 2, 2, 4), (1, 0, 2, 2), (0, 1, 1, 2)):
        sub = pix[y0::dy, x0::dx]
        if sub.shape[0] and sub.shape[1]:
            rows += [b'\x00' + r.tobytes() for r in sub]
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if c == 1 else 2, 0, 0, 1)
    return b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', ihdr) + chunk(b'IDAT', zlib.compress(b''.join(rows))) + chunk(b'IEND', b'')


def _files():
    """-> ({name: (bytes of the file, mode to read it in)} of the files the device reads, the same of the other kinds)"""
    from PIL import Image
    from aivc_amd import png
    rgb, grey = pcs.random_picture(129, 127, 3, seed=21), pcs.random_picture(65, 33, 1, seed=22)
    smooth = pcs.analytic_picture(70, 38, 3)
    eligible = {}
    for name, pix in (('rgb', rgb), ('grey', grey), ('smooth', smooth)):
        mode = 'L' if pix.shape[2] == 1 else 'RGB'
        eligible[name + '-default'] = (_pillow_file(pix), mode)
        for level in (0, 1, 9):
            eligible['%s-level%d' % (name, level)] = (_pillow_file(pix, compress_level=level), mode)
        eligible[name + '-optimize'] = (_pillow_file(pix, optimize=True), mode)
    for name, pix in (('rgb', rgb), ('grey', grey)):
        h, w, c = pix.shape
        filtered = pcs.filter_rows(pix, pcs.adaptive_types(pix)).tobytes()
        mode = 'L' if c == 1 else 'RGB'
        eligible[name + '-assembled'] = (png.assemble(w, h, c, zlib.compress(filtered)), mode)
        eligible[name + '-stitched'] = (png.assemble(w, h, c, pcs.stitched_stream(filtered, pcs.segment_lengths(h, w, c))), mode)
    eligible['rechunked-from'] = (_pillow_file(pcs.random_picture(5, 7, 3, seed=23)), 'RGB')
    eligible['rechunked'] = (rechunk(eligible['rechunked-from'][0]), 'RGB')
    buf = {}
    for name, img in (('palette', Image.fromarray(rgb).convert('P', palette=Image.ADAPTIVE, colors=64)),
                      ('rgba', Image.fromarray(np.dstack([rgb, 255 - rgb[..., :1]]))),
                      ('grey16', Image.fromarray(grey[..., 0].astype(np.uint16) * 257))):
        b = io.BytesIO()
        img.save(b, 'PNG')
        buf[name] = (b.getvalue(), 'RGB' if name != 'grey16' else 'L')
    buf['adam7'] = (adam7_file(rgb[:19, :21]), 'RGB')
    return eligible, buf


FILES, OTHER_KINDS = _files()
PIXELS_FROM = {'rechunked': 'rechunked-from'}  # the file whose pixels, as Pillow reads them, a file must give (default: its own)


def filter_types_of(png):
    parts = pcs.chunks(png)
    w, h, depth, colour = struct.unpack('>IIBB', parts[0][1][:10])
    data = zlib.decompress(b''.join(d for k, d in parts if k == b'IDAT'))
    return set(np.frombuffer(data, np.uint8).reshape(h, -1)[:, 0].tolist())


assert set().union(*(filter_types_of(f) for n, (f, _) in FILES.items() if 'assembled' not in n and 'stitched' not in n and 'rechunked' not in n)) \
    == {0, 1, 2, 3, 4}, 'the Pillow-written files together use all five filter types'


def broken_files():
    """{what is wrong: bytes of the file}"""
    good = FILES['grey-default'][0]
    parts = pcs.chunks(good)
    at = good.index(b'IDAT') + 8
    return {'idat-crc': good[:at] + bytes([good[at] ^ 1]) + good[at + 1:],
            'no-iend': good[:-12],
            'no-idat': b'\x89PNG\r\n\x1a\n' + chunk(b'IHDR', parts[0][1]) + chunk(b'IEND', b''),
            'truncated-chunk': good[:at + 5],
            'signature': b'\x89PNX' + good[4:]}
