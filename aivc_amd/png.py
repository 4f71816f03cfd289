"""PNG files of 8-bit grey and RGB pictures, coded and read on the device.
Writing (include/aivc_hip_png.h: row filters, and a dynamic-Huffman deflate of independent segments of whole rows;
aivc_amd.ops.png_encode): what stays on the host is what needs every byte of a picture in order and costs next to nothing: the
fold of the segments' Adler-32 sums, the container (signature, IHDR, one IDAT, IEND) and the CRC-32 of each chunk (zlib.crc32
over bytes that are on the host anyway, to be written).
Reading (include/aivc_hip_png_read.h: a zlib inflate and the inverse of the row filters; read_pictures): one PNG is one serial
inflate stream, but a clip is hundreds of independent ones, so every stream of a batch gets a workgroup of its own.  The host
walks the chunks and checks their CRC-32 (parse: the bytes are on the host anyway, to be uploaded).

Out of scope: PNG triplets as decoder output, general LZ77 matching in the writer; on the device, pictures with 16-bit or
sub-byte samples, a palette, alpha or Adam7 interlace (the reader hands those to Pillow), one stream split over several
workgroups -- the sync-flush boundaries of this project's own files included -- and a CRC-32."""
import struct
import zlib

SEGMENT_TARGET = 16384  # filtered bytes per segment, about: whole rows, at least one
ADLER_MOD = 65521
SIGNATURE = b'\x89PNG\r\n\x1a\n'
FILTERS = (0, 1, 2, 3, 4, 5)  # None, Sub, Up, Average, Paeth; 5: per row, the smallest sum of absolute residuals
CODERS = ('pillow', 'device')
READERS = ('pillow', 'device')


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


# ---- reading -----------------------------------------------------------------------------------------------------------------------
class PngError(ValueError):
    """a file that is no PNG, or a broken one; the message names what is wrong"""


class Unsupported(Exception):
    """a valid PNG of a kind the device does not read: palette, alpha, 16-bit or sub-byte samples, Adam7"""


def check_reader(reader, in_path=None, is_folder=None):
    """-> reader; a ValueError for an unknown one, or for 'device' where the input (in_path given) is not a picture folder"""
    if reader not in READERS:
        raise ValueError('png reader %r: expected one of %s' % (reader, ', '.join(READERS)))
    if reader == 'device' and in_path is not None and not is_folder:
        raise ValueError('--png_reader device reads the pictures of a folder: -i %s is not a directory' % (in_path,))
    return reader


def parse(data):
    """the bytes of a PNG file -> (w, h, c, [(offset, length) of every IDAT payload in data, in order]) for an 8-bit grey (c = 1)
    or 8-bit RGB (c = 3) picture without interlace.  The chunk headers are walked, the CRC-32 of IHDR and of every IDAT is
    checked, ancillary chunks are skipped.  Unsupported: a valid PNG of another kind.  PngError: a broken file."""
    data = memoryview(data)
    if bytes(data[:8]) != SIGNATURE:
        raise PngError('not a PNG file: wrong signature')
    at, idats, head, ended = 8, [], None, False
    while at < len(data):
        if at + 8 > len(data):
            raise PngError('truncated chunk header at byte %d' % at)
        n, = struct.unpack('>I', data[at:at + 4])
        kind = bytes(data[at + 4:at + 8])
        if at + 12 + n > len(data):
            raise PngError('truncated %s chunk at byte %d: %d bytes stated, %d left' % (kind.decode('latin-1'), at, n, len(data) - at - 12))
        if head is None and kind != b'IHDR':
            raise PngError('the first chunk is %s, not IHDR' % kind.decode('latin-1'))
        if kind in (b'IHDR', b'IDAT'):
            crc, = struct.unpack('>I', data[at + 8 + n:at + 12 + n])
            if zlib.crc32(data[at + 4:at + 8 + n]) & 0xffffffff != crc:
                raise PngError('CRC-32 mismatch in the %s chunk at byte %d' % (kind.decode('latin-1'), at))
        if kind == b'IHDR':
            if head is not None or n != 13:
                raise PngError('a second IHDR chunk, or one of %d bytes' % n)
            head = struct.unpack('>IIBBBBB', data[at + 8:at + 21])
        elif kind == b'IDAT':
            idats.append((at + 8, n))
        elif kind == b'IEND':
            ended = True
            break
        at += 12 + n
    if head is None:
        raise PngError('no IHDR chunk')
    if not ended:
        raise PngError('no IEND chunk')
    if not idats:
        raise PngError('no IDAT chunk')
    w, h, depth, colour, compression, filter_method, interlace = head
    if w < 1 or h < 1 or colour not in (0, 2, 3, 4, 6) or depth not in (1, 2, 4, 8, 16) or compression or filter_method or interlace > 1:
        raise PngError('IHDR: %d x %d, depth %d, colour type %d, compression %d, filter %d, interlace %d'
                       % (w, h, depth, colour, compression, filter_method, interlace))
    if depth != 8 or colour not in (0, 2) or interlace:
        raise Unsupported('depth %d, colour type %d, interlace %d: the device reads 8-bit grey and RGB without interlace' % (depth, colour, interlace))
    return w, h, 1 if colour == 0 else 3, idats


def _pillow_picture(path, mode, device):
    import numpy as np
    import torch
    from PIL import Image
    img = Image.open(path)
    if img.mode != mode:
        img = img.convert(mode)
    a = np.asarray(img)
    return torch.from_numpy(a.copy()).to(device).view(a.shape[0], a.shape[1], -1)


def read_pictures(paths, device, mode, stats=None):
    """The PNG files `paths` -> a list of uint8 tensors [h, w, c] on `device`, c = 1 for mode 'L' and 3 for 'RGB': the pixels Pillow
    reads.  The 8-bit files of that mode are inflated and unfiltered on the device: their IDAT payloads go through one pinned
    staging buffer in batches of at most rawvideo.BATCH_BYTES (of filtered bytes), each batch one inflate launch, one unfilter
    launch and one copy back of the status words.  Every other file -- Unsupported, or of another colour type -- is read by Pillow
    with the conversion the loaders of func_util.img_processing apply, and takes its place in the list.  A broken file, or a
    stream the device refuses, raises PngError with the file's name.  stats: a dict whose 'device' and 'pillow' counts grow."""
    import numpy as np
    import torch
    from . import abi, ops, rawvideo
    if mode not in ('L', 'RGB'):
        raise ValueError('read_pictures: mode %r, expected L or RGB' % (mode,))
    paths = list(paths)
    out, jobs = [None] * len(paths), []
    for i, path in enumerate(paths):
        with open(path, 'rb') as f:
            data = f.read()
        try:
            w, h, c, idats = parse(data)
        except Unsupported:
            c = None
        except PngError as e:
            raise PngError('%s: %s' % (path, e))
        if c != (1 if mode == 'L' else 3):
            out[i] = _pillow_picture(path, mode, device)
        else:
            view = memoryview(data)
            jobs.append((i, (h, w, c), [view[o:o + n] for o, n in idats]))
    at = 0
    while at < len(jobs):
        end, total = at, 0
        while end < len(jobs) and (end == at or total + _filtered_bytes(jobs[end][1]) <= rawvideo.BATCH_BYTES):
            total += _filtered_bytes(jobs[end][1])
            end += 1
        batch = jobs[at:end]
        shapes = [s for _, s, _ in batch]
        filt, info, _ = ops.inflate_launch([p for _, _, p in batch], [_filtered_bytes(s) for s in shapes], device)
        pics, status = ops.png_unfilter_launch(filt, shapes)
        words = torch.cat([info[:, 0], status]).cpu().numpy().view(np.uint32)  # (synchronises: the one copy back)
        for k, (i, _, _) in enumerate(batch):
            if words[k]:
                raise PngError('%s: inflate: %s' % (paths[i], abi.INFLATE_STATUS.get(int(words[k]), 'status %d' % words[k])))
            if words[len(batch) + k]:
                raise PngError('%s: %s' % (paths[i], abi.PNG_UNFILTER_STATUS.get(int(words[len(batch) + k]), 'status %d' % words[len(batch) + k])))
            out[i] = pics[k]
        at = end
    if stats is not None:
        stats['device'] = stats.get('device', 0) + len(jobs)
        stats['pillow'] = stats.get('pillow', 0) + len(paths) - len(jobs)
    return out


def _filtered_bytes(shape):
    h, w, c = shape
    return h * (1 + w * c)
