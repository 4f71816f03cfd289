"""PNG files of 8-bit grey and RGB pictures, coded on the device (include/aivc_hip_png.h: row filters, and a dynamic-Huffman
deflate of independent segments of whole rows; aivc_amd.ops.png_encode).  What stays on the host is what needs every byte of a
picture in order and costs next to nothing: the fold of the segments' Adler-32 sums, the container (signature, IHDR, one IDAT,
IEND) and the CRC-32 of each chunk (zlib.crc32 over bytes that are on the host anyway, to be written).

Out of scope: reading PNGs on the device (a PNG is one serial inflate stream per picture), PNG triplets as decoder output,
16-bit samples, palette, alpha, Adam7 and general LZ77 matching."""
import struct
import zlib

SEGMENT_TARGET = 16384  # filtered bytes per segment, about: whole rows, at least one
ADLER_MOD = 65521
SIGNATURE = b'\x89PNG\r\n\x1a\n'
FILTERS = (0, 1, 2, 3, 4, 5)  # None, Sub, Up, Average, Paeth; 5: per row, the smallest sum of absolute residuals
CODERS = ('pillow', 'device')


def check_size(h, w, c):
    h, w, c = int(h), int(w), int(c)
    if h < 1 or w < 1 or c not in (1, 3):
        raise ValueError('png: a picture of %d x %d with %d channels (w x h): sides of at least 1, 1 (grey) or 3 (RGB) channels' % (w, h, c))
    return h, w, c


def stored_bound(length):
    """the most a segment of `length` filtered bytes codes to: stored blocks of at most 65535 bytes, 5 bytes of header each"""
    return length + 5 * -(-length // 65535)


def slot_capacity(length):
    """bytes of a segment's slot: the stored bound and the 4 bytes of an empty stored block, to a multiple of 16"""
    return -(-(stored_bound(length) + 4) // 16) * 16


def segment_plan(h, w, c):
    """THE SEGMENT RULE -> (rows per segment, segments per picture, bytes between segments of the filtered stream, bytes of a slot):
    as many whole rows as fit SEGMENT_TARGET bytes, at least one -- a longer row is a segment of its own"""
    h, w, c = check_size(h, w, c)
    row = 1 + w * c
    rows = min(h, max(1, SEGMENT_TARGET // row))
    return rows, -(-h // rows), -(-rows * row // 16) * 16, slot_capacity(rows * row)


def segment_lengths(h, w, c):
    """the filtered bytes of each segment of a picture"""
    rows, nseg, _, _ = segment_plan(h, w, c)
    row = 1 + w * c
    return [min(rows, h - s * rows) * row for s in range(nseg)]


def adler_partial(data):
    """(len, s1, s2) of a run of bytes: s1 = sum b_i, s2 = sum (len - i) b_i, both mod 65521 (the host statement of what the
    device computes per segment)"""
    n, s1, s2 = len(data), 0, 0
    for i in range(0, n, 4096):
        part = data[i:i + 4096]
        s1 += sum(part)
        s2 += sum((n - i - k) * b for k, b in enumerate(part))
    return n, s1 % ADLER_MOD, s2 % ADLER_MOD


def adler_fold(parts, a=1, b=0):
    """[(len, s1, s2)] of consecutive runs of bytes -> the Adler-32 of their concatenation"""
    for length, s1, s2 in parts:
        b = (b + length * a + s2) % ADLER_MOD
        a = (a + s1) % ADLER_MOD
    return (b << 16) | a


def _chunk(kind, data):
    return struct.pack('>I', len(data)) + kind + data + struct.pack('>I', zlib.crc32(kind + data) & 0xffffffff)


def assemble(w, h, c, zstream):
    """a complete zlib stream of the filtered rows -> the bytes of the file: signature, IHDR (bit depth 8, colour type 0 for
    c = 1 and 2 for c = 3, no interlace), one IDAT, IEND"""
    h, w, c = check_size(h, w, c)
    ihdr = struct.pack('>IIBBBBB', w, h, 8, 0 if c == 1 else 2, 0, 0, 0)
    return SIGNATURE + _chunk(b'IHDR', ihdr) + _chunk(b'IDAT', bytes(zstream)) + _chunk(b'IEND', b'')


def check_coder(coder, out_file=None, is_folder=None):
    """-> coder; a ValueError for an unknown one, or for 'device' where the output (out_file given) is not a picture folder"""
    if coder not in CODERS:
        raise ValueError('png coder %r: expected one of %s' % (coder, ', '.join(CODERS)))
    if coder == 'device' and out_file is not None and not is_folder:
        raise ValueError('--png_coder device codes the pictures of a folder: -o %s is a raw video file (name a folder, or end the '
                         'name with /)' % (out_file,))
    return coder


def write_pictures(pix, paths, filter=5):
    """pix: uint8 CUDA tensor [n, h, w, c] (c = 1 or 3), or [n, h, w] for grey -> the files paths[i], one per picture.  The
    pictures are coded in batches of at most 256 MiB of pixels (ops.png_encode), two host synchronisations per batch."""
    from . import ops
    if pix.dim() == 3:
        pix = pix.unsqueeze(-1)
    n, h, w, c = pix.shape
    paths = list(paths)
    if len(paths) != n:
        raise ValueError('write_pictures: %d pictures, %d paths' % (n, len(paths)))
    for path, z in zip(paths, ops.png_encode(pix, filter)):
        with open(path, 'wb') as f:
            f.write(assemble(w, h, c, z))
