"""Raw video files: what a layout is (PixFmt, under ffmpeg's names), the one reader of the codec's planes (open_raw: .y4m and
headerless files, planar 8-bit 4:2:0 as every other layout) and the one writer (write_raw).

The host does no sample arithmetic.  A file's bytes travel to the device as they are -- a stretch of the file per batch, `FRAME`
lines and all, through the pinned pool of aivc_amd.ops._stage -- and one launch per batch converts them to 8-bit 4:2:0 planes
(ops.raw_to_yuv420u8; the arithmetic is stated in include/aivc_hip_rawvideo.h).  Writing is the mirror: one launch per batch
(ops.yuv420u8_to_raw), one copy back.  Out of scope: big-endian layouts, nv16, packed layouts (yuyv422, ...), RGB, interlaced
.y4m, and writing 4:2:2 / 4:4:4 (which would need a choice of upsampling filter)."""
import mmap
import os
import re

import numpy as np

from . import abi

# name -> (bytes per sample, significant bits, bits at the top of the word, shift_x, shift_y, chroma arrangement)
_TABLE = {}
for _c, (_sx, _sy) in (('420', (1, 1)), ('422', (1, 0)), ('444', (0, 0))):
    _TABLE['yuv%sp' % _c] = (1, 8, 0, _sx, _sy, abi.CHROMA_PLANAR)
    for _d in (10, 12, 16):
        _TABLE['yuv%sp%dle' % (_c, _d)] = (2, _d, 0, _sx, _sy, abi.CHROMA_PLANAR)
_TABLE['gray'] = (1, 8, 0, 1, 1, abi.CHROMA_NONE)
for _d in (10, 12, 16):
    _TABLE['gray%dle' % _d] = (2, _d, 0, 1, 1, abi.CHROMA_NONE)
_TABLE.update(nv12=(1, 8, 0, 1, 1, abi.CHROMA_UV), nv21=(1, 8, 0, 1, 1, abi.CHROMA_VU),
              p010le=(2, 10, 1, 1, 1, abi.CHROMA_UV), p016le=(2, 16, 1, 1, 1, abi.CHROMA_UV))
PIX_FMTS = tuple(_TABLE)

BATCH_BYTES = 256 << 20  # raw bytes per pinned buffer, copy and launch: a convention that bounds pinned memory, not measured


class RawVideoError(ValueError):
    """a file that is not what it is taken for, or a request outside it; the message says what the file holds"""


class PixFmt:
    """A raw layout, by ffmpeg's name: PixFmt('yuv420p10le').  bytes_per_sample (1 or 2, little-endian), depth (8 ... 16),
    msb_aligned (the bits sit at the top of the word), shift_x / shift_y (chroma subsampling), chroma (abi.CHROMA_*)."""

    def __init__(self, name):
        if isinstance(name, PixFmt):
            name = name.name
        if name not in _TABLE:
            raise ValueError('unknown pixel format %r; known: %s' % (name, ', '.join(PIX_FMTS)))
        self.name = name
        self.bytes_per_sample, self.depth, self.msb_aligned, self.shift_x, self.shift_y, self.chroma = _TABLE[name]

    def __repr__(self):
        return 'PixFmt(%r)' % self.name

    def __eq__(self, other):
        return isinstance(other, PixFmt) and other.name == self.name

    def __hash__(self):
        return hash(self.name)

    @property
    def writable(self):
        """whether yuv420u8_to_raw / write_raw produce it: 4:2:0 and grey layouts"""
        return self.chroma == abi.CHROMA_NONE or (self.shift_x, self.shift_y) == (1, 1)

    def chroma_size(self, w, h):
        """(columns, rows) of a source chroma plane in samples, ffmpeg's ceil convention; (0, 0) without chroma"""
        if self.chroma == abi.CHROMA_NONE:
            return 0, 0
        return -(-w >> self.shift_x), -(-h >> self.shift_y)

    def layout(self, w, h, pad=0):
        """-> ([byte offset of each plane], [row pitch of each plane], bytes per frame) of a w x h frame whose rows are the tight
        ones plus `pad` bytes (0: what a file holds); planes the layout does not have: offset and pitch 0"""
        cw, ch = self.chroma_size(w, h)
        b = self.bytes_per_sample
        rows = [(w * b, h)]
        if self.chroma == abi.CHROMA_PLANAR:
            rows += [(cw * b, ch)] * 2
        elif self.chroma != abi.CHROMA_NONE:
            rows += [(2 * cw * b, ch)]
        offsets, pitches, at = [0, 0, 0], [0, 0, 0], 0
        for p, (tight, n_rows) in enumerate(rows):
            offsets[p], pitches[p] = at, tight + pad
            at += (tight + pad) * n_rows
        return offsets, pitches, at - pad  # (the last row ends with its tight part)

    def frame_bytes(self, w, h):
        return self.layout(w, h)[2]

    def struct(self, w, h, offsets=None, pitches=None):
        """the aivc_rawvideo_fmt of a w x h frame (include/aivc_hip_rawvideo.h)"""
        if offsets is None or pitches is None:
            offsets, pitches, _ = self.layout(w, h)
        return abi.RawVideoFmt(w, h, self.bytes_per_sample, self.depth, self.msb_aligned, self.shift_x, self.shift_y, self.chroma,
                               (abi.C.c_int64 * 3)(*offsets), (abi.C.c_int64 * 3)(*pitches))

    @property
    def y4m_tag(self):
        """the C tag of a .y4m header, None for a layout the container has no tag for"""
        if self.msb_aligned or self.chroma in (abi.CHROMA_UV, abi.CHROMA_VU):
            return None
        if self.chroma == abi.CHROMA_NONE:
            return 'mono' if self.depth == 8 else 'mono%d' % self.depth
        sub = {(1, 1): '420', (1, 0): '422', (0, 0): '444'}[(self.shift_x, self.shift_y)]
        return sub if self.depth == 8 else '%sp%d' % (sub, self.depth)


# ---- names and headers ---------------------------------------------------------------------------------------------------------
def parse_size_name(path):
    """'<Name>_<W>x<H>_<fps>_420.yuv' -> (w, h)  (src/format_conversion/utils.py:45-72)"""
    for tok in os.path.basename(path).split('_'):
        m = re.fullmatch(r'(\d+)x(\d+)', tok)
        if m:
            return int(m.group(1)), int(m.group(2))
    raise RawVideoError('cannot parse WxH from %s' % path)


def pix_fmt_from_name(path):
    """the layout a headerless file's name states: a _420 / _422 / _444 token and an optional _10b / _12b / _16b / _<n>bit token
    (any of them may carry the extension); the default is yuv420p"""
    sub, depth = '420', 8
    for tok in os.path.basename(path).split('_'):
        tok = tok.split('.')[0]
        if tok in ('420', '422', '444'):
            sub = tok
        m = re.fullmatch(r'(\d+)(b|bit)', tok)
        if m and int(m.group(1)) in (8, 10, 12, 16):
            depth = int(m.group(1))
    return PixFmt('yuv%sp' % sub if depth == 8 else 'yuv%sp%dle' % (sub, depth))


_Y4M_SUB = {'420': '420', '420jpeg': '420', '420mpeg2': '420', '420paldv': '420', '422': '422', '444': '444', 'mono': 'mono'}


def y4m_pix_fmt(tag):
    """the C tag of a .y4m header -> PixFmt; the 4:2:0 sitings all read as 4:2:0 (chroma siting is ignored)"""
    m = re.fullmatch(r'(420|422|444|mono)p(10|12|16)', tag) or re.fullmatch(r'(mono)(10|12|16)', tag)
    if tag in _Y4M_SUB:
        sub, depth = _Y4M_SUB[tag], 8
    elif m:
        sub, depth = m.group(1), int(m.group(2))
    else:
        raise RawVideoError('.y4m colour space C%s is not supported; known: 420, 420jpeg, 420mpeg2, 420paldv, 422, 444, mono and '
                            'the p10 / p12 / p16 forms of 420, 422, 444 and mono' % tag)
    if sub == 'mono':
        return PixFmt('gray' if depth == 8 else 'gray%dle' % depth)
    return PixFmt('yuv%sp' % sub if depth == 8 else 'yuv%sp%dle' % (sub, depth))


def parse_y4m_header(line):
    """b'YUV4MPEG2 W.. H.. F..:.. I. A..:.. C... X...' (without the newline) -> (w, h, (fps numerator, denominator), PixFmt)"""
    toks = line.decode('ascii', 'replace').split(' ')
    if toks[0] != 'YUV4MPEG2':
        raise RawVideoError('not a .y4m stream: it starts with %r' % line[:16])
    w = h = None
    fps, tag = (25, 1), '420'
    for t in toks[1:]:
        if not t:
            continue
        key, val = t[0], t[1:]
        if key == 'W':
            w = int(val)
        elif key == 'H':
            h = int(val)
        elif key == 'F':
            a, _, b = val.partition(':')
            fps = (int(a), int(b or 1))
        elif key == 'I':
            if val not in ('p', '?'):
                raise RawVideoError('.y4m interlacing I%s is not supported: only progressive streams (Ip, I? or no I)' % val)
        elif key == 'C':
            tag = val
    if not w or not h or w < 1 or h < 1:
        raise RawVideoError('.y4m header without a frame size: %r' % line)
    return w, h, fps, y4m_pix_fmt(tag)


# ---- reading ---------------------------------------------------------------------------------------------------------------------
class RawReader:
    """A raw video file: w, h, fps ((numerator, denominator), or None where the file does not say), pix_fmt, n_frames, and
    read(first, last, device).  offsets[i]: where frame i's samples start in the file."""

    def __init__(self, path, pix_fmt=None, size=None):
        self.path = path
        size_bytes = os.path.getsize(path)
        self._file = open(path, 'rb')
        self._map = mmap.mmap(self._file.fileno(), 0, access=mmap.ACCESS_READ) if size_bytes else b''
        self.is_y4m = path.endswith('.y4m')
        if self.is_y4m:
            end = self._map.find(b'\n', 0, 4096)
            if end < 0:
                raise RawVideoError('%s: no .y4m header line in its first 4096 bytes' % path)
            self.w, self.h, self.fps, self.pix_fmt = parse_y4m_header(self._map[:end])
            self.frame_bytes = self.pix_fmt.frame_bytes(self.w, self.h)
            self.offsets, at = [], end + 1
            while True:  # a FRAME line may carry parameters: walk, do not assume 6 bytes; a truncated last frame is not counted
                nl = self._map.find(b'\n', at, at + 4096)
                if nl < 0 or nl + 1 + self.frame_bytes > size_bytes:
                    break
                self.offsets.append(nl + 1)
                at = nl + 1 + self.frame_bytes
            self._starts = [end + 1] + [o + self.frame_bytes for o in self.offsets[:-1]]  # where each FRAME line begins
        else:
            self.w, self.h = parse_size_name(path) if size is None else (int(size[0]), int(size[1]))
            self.fps = None
            self.pix_fmt = pix_fmt_from_name(path) if pix_fmt is None else PixFmt(pix_fmt)
            self.frame_bytes = self.pix_fmt.frame_bytes(self.w, self.h)
            self.offsets = [i * self.frame_bytes for i in range(size_bytes // self.frame_bytes)]
        self.n_frames = len(self.offsets)

    def close(self):
        if self._map:
            self._map.close()
        self._file.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def is_plain(self):
        """a headerless file of planar 8-bit 4:2:0: the planes are the file's bytes, nothing is converted (and read_yuv prints no
        `[INFO] input:` line)"""
        return not self.is_y4m and self.pix_fmt.name == 'yuv420p'

    def frame_range(self, first=0, last=-1):
        """(first, last) with last < 0 the file's last frame; a RawVideoError that states the file's range for a request outside"""
        last = self.n_frames - 1 if last < 0 else last
        if not (0 <= first <= last < self.n_frames):
            raise RawVideoError('frames %d:%d are not in %s; it holds the frames 0 ... %d (%s %dx%d)'
                                % (first, last, self.path, self.n_frames - 1, self.pix_fmt.name, self.w, self.h))
        return first, last

    def _check_frame_line(self, i):
        line = self._map[self._starts[i]:self.offsets[i]]
        if not (line.startswith(b'FRAME') and line[5:6] in (b' ', b'\n')):
            raise RawVideoError('%s: frame %d does not start with a FRAME line at byte %d but with %r'
                                % (self.path, i, self._starts[i], line[:16]))

    def batches(self, first, last):
        """the frames first ... last in runs of at most BATCH_BYTES raw bytes (at least one frame): [(i0, i1 inclusive)]"""
        per = max(1, BATCH_BYTES // self.frame_bytes)
        return [(i, min(i + per - 1, last)) for i in range(first, last + 1, per)]

    def read_stacks(self, first=0, last=-1, device=None):
        """-> [(y [k, h, w], u, v [k, ceil(h/2), ceil(w/2)])] uint8 device tensors, one triple per batch: the stretch of the file
        that holds the batch's frames is one pinned buffer and one asynchronous copy (ops._stage), then one launch"""
        import torch
        from . import ops
        first, last = self.frame_range(first, last)
        device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
        out = []
        for i0, i1 in self.batches(first, last):
            if self.is_y4m:
                for i in range(i0, i1 + 1):
                    self._check_frame_line(i)
            lo, hi = self.offsets[i0], self.offsets[i1] + self.frame_bytes
            blob, _ = ops._stage(device, [np.frombuffer(self._map, np.uint8, hi - lo, lo)])
            out.append(ops.raw_to_yuv420u8(blob, [self.offsets[i] - lo for i in range(i0, i1 + 1)], self.pix_fmt, self.w, self.h))
        return out

    def read(self, first=0, last=-1, device=None):
        """-> the list real_life.encode.read_yuv returns: one {'y','u','v'} dict of uint8 [1, h', w'] device tensors per frame,
        views into the batches' stacks"""
        frames = []
        for y, u, v in self.read_stacks(first, last, device):
            frames += [{'y': y[i:i + 1], 'u': u[i:i + 1], 'v': v[i:i + 1]} for i in range(y.shape[0])]
        return frames


def open_raw(path, pix_fmt=None, size=None):
    """A .y4m file (layout, size and frame rate from its header) or a headerless one (size from `size` or the name's _<W>x<H>_
    token, layout from pix_fmt or the name's tokens, default yuv420p) -> RawReader"""
    return RawReader(path, pix_fmt, size)


# ---- writing ---------------------------------------------------------------------------------------------------------------------
def parse_fps(text):
    """'N' or 'N:D' -> (N, D)"""
    a, _, b = str(text).partition(':')
    try:
        fps = (int(a), int(b or 1))
    except ValueError:
        raise ValueError('frame rate %r: expected N or N:D' % (text,))
    if fps[0] < 1 or fps[1] < 1:
        raise ValueError('frame rate %r: both numbers must be positive' % (text,))
    return fps


def check_writable(pix_fmt, path=''):
    """-> PixFmt; a ValueError for a layout that is not written, or that a .y4m path has no tag for"""
    fmt = PixFmt(pix_fmt)
    if not fmt.writable:
        raise ValueError('%s is not written: only 4:2:0 and grey layouts are (4:2:2 and 4:4:4 need an upsampling filter); writable: %s'
                         % (fmt.name, ', '.join(n for n in PIX_FMTS if PixFmt(n).writable)))
    if path.endswith('.y4m') and fmt.y4m_tag is None:
        raise ValueError('%s has no .y4m colour space tag: write it to a headerless file, or choose a planar layout' % fmt.name)
    return fmt


def _on(t, device):
    return t if device is None else t.to(device)


def write_raw(frames, path, pix_fmt='yuv420p', fps=(25, 1), device=None):
    """frames: a list of {'y','u','v'} dicts of uint8 planes [1, h, w] / [1, ceil(h/2), ceil(w/2)] (device tensors, or host ones:
    those are copied over) -> the file `path` in the layout pix_fmt; a .y4m path gets the header (C tag from the layout, F from
    fps) and a `FRAME` line per frame.  One export launch and one device-to-host copy per batch of at most BATCH_BYTES -- but for
    headerless yuv420p, THE ONE DECISION of the writer: there the file is the planes as they are, and copying them back one by one
    measured twice as fast as the export's one large copy back (experiments/one_raw_io.md)."""
    import torch
    from . import ops
    fmt = check_writable(pix_fmt, path)
    y4m = path.endswith('.y4m')
    lead = b'FRAME\n' if y4m else b''
    with open(path, 'wb') as f:
        if not frames:
            if y4m:
                raise ValueError('write_raw: a .y4m file needs a frame size, and there is no frame')
            return
        if not y4m and fmt.name == 'yuv420p':
            for fr in frames:
                for k in 'yuv':
                    f.write(np.ascontiguousarray(torch.as_tensor(fr[k]).cpu().numpy()).tobytes())
            return
        h, w = frames[0]['y'].shape[-2:]
        if y4m:
            f.write(b'YUV4MPEG2 W%d H%d F%d:%d Ip A1:1 C%s\n' % (w, h, fps[0], fps[1], fmt.y4m_tag.encode()))
        per = max(1, BATCH_BYTES // fmt.frame_bytes(w, h))
        for i0 in range(0, len(frames), per):
            part = frames[i0:i0 + per]
            y, u, v = (torch.cat([_on(torch.as_tensor(fr[k]), device).reshape((1,) + tuple(fr[k].shape[-2:])) for fr in part])
                       for k in 'yuv')
            f.write(ops.yuv420u8_to_raw(y, u, v, fmt, lead).cpu().numpy().tobytes())
