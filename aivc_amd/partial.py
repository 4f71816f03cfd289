"""Partial decode, the host side: which frames of which intra-period units a request names, and what has to be decoded
for them.  No device work and no torch: FrameCodec.decode_video, parallel.decode_video_sharded and the drivers of
real_life/decode.py all take their selection from here, as one Plan (plan()) that is made once per decode.  A whole decode is
the plan of the request for everything.

A request is a set of ABSOLUTE display indices (the numbering of the video header, idx_first ... idx_last, which the
manifest and the PNG names use) and / or a temporal level: the dependency depth of a frame inside its unit
(func_util.GOP_structure.frame_depths).  Units are independent, so a request falls apart into one set of frame names per
unit; the reference closure of that set is what the unit's decode costs."""
import collections

from .func_util.GOP_structure import frame_depths, generate_gop_struct, reference_closure

# One video as the decoder takes it when it has not read the whole file: the header's fields, the coding structure of every
# unit that was walked (in order, from unit 0) and the GOP records -- None for a unit whose bytes were not read.
IndexedVideo = collections.namedtuple('IndexedVideo', 'data_dim first last names gops')

# One decode, stated once.  video: the IndexedVideo; wanted: per unit the set of frame names that are RETURNED (select());
# need: per unit the set that is DECODED; indices: the absolute display indices returned, ascending; whole: nothing was
# selected, the decode is that of the whole stream.
Plan = collections.namedtuple('Plan', 'video wanted need indices whole')


class FrameSelectionError(ValueError):
    """the request names no frame of the stream, or one outside it; the message says what the stream holds"""


def frame_name(i):
    return 'frame_%d' % i


def indexed_from_blob(blob):
    """a whole container held in memory as an IndexedVideo"""
    from .real_life import cat_binary_files as container
    from .real_life import header as hdr
    data_dim, first, last, gops = container.unpack_video(blob)
    for u, g in enumerate(gops):
        if len(g) < hdr.GOP_HEADER_SIZE_BYTES:
            raise container.ContainerError('GOP record %d: %d bytes, a GOP header has %d' % (u, len(g), hdr.GOP_HEADER_SIZE_BYTES))
    return IndexedVideo(data_dim, first, last, [hdr.parse_gop_header(g[:hdr.GOP_HEADER_SIZE_BYTES])[0] for g in gops], gops)


def unit_lengths(names):
    """frames per unit, from every unit's OWN coding structure (a container may mix them)"""
    return [len(generate_gop_struct(n)) for n in names]


def _locate(lengths, pos):
    for u, n in enumerate(lengths):
        if pos < n:
            return u, pos
        pos -= n
    return None


def locate(names, first, idx):
    """absolute display index -> (unit, frame of the unit); None behind the units listed"""
    return _locate(unit_lengths(names), idx - first)


def _range_text(first, last):
    return 'the stream holds the frames %d ... %d' % (first, last)


def frame_range(span, first, last):
    """(a, b), either end None for the stream's -> the indices a ... b, inclusive"""
    a, b = span
    a, b = first if a is None else a, last if b is None else b
    if b < a:
        raise FrameSelectionError('frames %d:%d select nothing; %s' % (a, b, _range_text(first, last)))
    return range(a, b + 1)


def select(names, first, last, frames=None, max_level=None):
    """-> one set of frame names per unit listed in `names` (empty: nothing of that unit).
    frames: absolute display indices, or None for every frame idx_first ... idx_last; max_level: keep frames whose depth in
    their unit is at most that; both: a frame must pass both.  The padded repeats behind idx_last can never be selected.
    FrameSelectionError naming the stream's range for an index outside it, a negative level, or a selection left empty."""
    if max_level is not None and max_level < 0:
        raise FrameSelectionError('max_level %d: temporal levels count from 0; %s' % (max_level, _range_text(first, last)))
    if frames is None:
        idxs = range(first, last + 1)
    else:
        idxs = sorted({int(i) for i in frames})
        off = [i for i in idxs if not first <= i <= last]
        if off:
            raise FrameSelectionError('frame %d is not in the stream; %s' % (off[0], _range_text(first, last)))
    wanted = [set() for _ in names]
    depths, lengths = {}, unit_lengths(names)
    for idx in idxs:
        at = _locate(lengths, idx - first)
        if at is None:  # (a driver that indexed a file only as far as its request reaches never asks behind that)
            if frames is None:
                break
            raise FrameSelectionError('frame %d lies behind the %d units that were indexed' % (idx, len(names)))
        u, k = at
        if max_level is not None:
            if names[u] not in depths:
                depths[names[u]] = frame_depths(generate_gop_struct(names[u]))
            if depths[names[u]][frame_name(k)] > max_level:
                continue
        wanted[u].add(frame_name(k))
    if not any(wanted):
        raise FrameSelectionError('the request selects no frame; %s' % _range_text(first, last))
    return wanted


def closures(names, wanted):
    """per unit: the frames that have to be decoded for wanted[u] (reference_closure; empty where nothing is wanted, and the
    name of such a unit is not looked at).  ValueError for a frame name the unit's coding structure does not have."""
    out = []
    for u, (n, w) in enumerate(zip(names, wanted)):
        gop = generate_gop_struct(n) if w else {}
        unknown = sorted(set(w or ()) - set(gop))
        if unknown:
            raise ValueError('unit %d: coding structure %s has no %s' % (u, n, ', '.join(unknown)))
        out.append(reference_closure(gop, w or ()))
    return out


def plan(video, frames=None, max_level=None):
    """video: an IndexedVideo, or the bytes of a whole container; frames / max_level: as in select() -> Plan.
    A request is decoded as far as its reference closure reaches.  A whole decode (neither frames nor max_level) decodes every
    frame of every unit's coding structure, the padded repeats behind idx_last included -- they are part of its launches
    and of what the bit-count check looks at -- and returns what select() returns for it: idx_first ... idx_last."""
    if not isinstance(video, IndexedVideo):
        video = indexed_from_blob(video)
    whole = frames is None and max_level is None
    wanted = select(video.names, video.first, video.last, frames, max_level)
    need = [set(generate_gop_struct(n)) for n in video.names] if whole else closures(video.names, wanted)
    return Plan(video, wanted, need, selected_indices(video.names, video.first, wanted), whole)


def selected_indices(names, first, wanted):
    """the absolute display indices of a selection, ascending"""
    out, base = [], first
    for n, w in zip(unit_lengths(names), wanted):
        out += sorted(base + int(f.split('_')[-1]) for f in (w or ()))
        base += n
    return out


def coded_frames(names, first, last):
    """coded frames of the stream, padded ones included.  Units behind the ones listed (a file indexed only as far as the request
    reaches) are counted with the coding structure of the last unit listed."""
    lens = unit_lengths(names)
    rest = (last - first + 1) - sum(lens)
    if rest > 0 and lens:
        lens += [lens[-1]] * (-(-rest // lens[-1]))
    return sum(lens)


def parse_frames_arg(text):
    """'A:B' (inclusive), 'A:', ':B' or 'A' -> (a, b) with None for an open end; ValueError for anything else or B < A"""
    parts = text.split(':')
    if len(parts) > 2 or not all(p == '' or p.isdigit() for p in parts) or not any(parts):
        raise ValueError('%r: expected A:B, A:, :B or A (non-negative frame indices)' % text)
    a = int(parts[0]) if parts[0] else None
    b = a if len(parts) == 1 else (int(parts[1]) if parts[1] else None)
    if a is not None and b is not None and b < a:
        raise ValueError('%r: the last frame lies in front of the first' % text)
    return a, b
