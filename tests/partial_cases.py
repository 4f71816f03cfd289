"""What tests/test_partial_decode.py and tests/test_gpu_partial_decode.py share, each stated once.  Not a test module.

Selections are stated as (absolute display indices or None, max_level or None).  The spies only record: which frames went
into FrameCodec.entropy_decode and FrameCodec.synthesise_batch, and which frame records codec.split_sections was handed."""
import io

import numpy as np

import schedule_cases as sc

STRUCTURES = ['1_GOP_0', 'LDP_8', '1_GOP_8', '2_GOP_4', '1_GOP_32']

PADDED = ('1_GOP_8', 64, 48, 12, 3)  # two 9-frame units for 12 frames: unit 1 holds frames 9, 10, 11 and six repeats of 11

# selections on the `ra` clip of schedule_cases (18 frames, two units of 1_GOP_8): id -> (frames, max_level, indices returned,
# frames in the decoded closures)
RA_SELECTIONS = {
    'frame3': ([3], None, [3], 5),
    'frames7to11': (list(range(7, 12)), None, [7, 8, 9, 10, 11], 10),
    'level3': (None, 3, [0, 2, 4, 6, 8, 9, 11, 13, 15, 17], 10),
    'frames7to11_level3': (list(range(7, 12)), 3, [8, 9, 11], 6),
}
# ... and on `chained` (two units of 2_GOP_4, 9 frames each, levels that mix P and B frames)
CHAINED_SELECTIONS = {
    'frames5and12': ([5, 12], None, [5, 12]),
    'level1': (None, 1, [0, 4, 9, 13]),
}
# the default, chunk boundaries inside levels (3, 8, None, 16), one-frame launches (1, 2, None, 1), the entropy stage level by level (64, 8, 1, 16)
PARTIAL_KNOBS = [sc.DEFAULT_KNOBS, sc.CROSSING_KNOBS[0], sc.ONE_FRAME_KNOBS, sc.LOOKAHEAD_KNOBS[0]]
assert PARTIAL_KNOBS[1:] == [(3, 8, None, 16), (1, 2, None, 1), (64, 8, 1, 16)]


def name(i):
    return 'frame_%d' % i


def brute_closure(gop, names):
    """the fixed point of `add the references of everything in the set`, the slow way"""
    out = set(names)
    while True:
        more = {gop[f][k] for f in out for k in ('prev_ref', 'next_ref') if gop[f][k] is not None} | out
        if more == out:
            return out
        out = more


def dummy_video(unit_names, first, n_frames, payload=lambda u, k: b'u%df%d' % (u, k) * (u + 2)):
    """a container of the given units with made-up frame records (host only: nothing decodes them)
    -> (bytes, [GOP record per unit])"""
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    from aivc_amd.real_life import cat_binary_files as container
    from aivc_amd.real_life import header as hdr
    gops = [container.pack_gop(hdr.gop_header_bytes(g, u / 16), [payload(u, k) for k in range(len(generate_gop_struct(g)))])
            for u, g in enumerate(unit_names)]
    dd = {'x': (48, 64), 'y': (3, 4), 'z': (1, 1)}
    return container.pack_video(hdr.video_header_bytes(dd, len(gops), first, first + n_frames - 1), gops), gops


class CountingFile(io.BytesIO):
    """a file that knows how many bytes were read from it"""
    nread = 0

    def read(self, *a):
        b = super().read(*a)
        self.nread += len(b)
        return b


def padded_reference(spec):
    """schedule_cases.reference for the PADDED clip (which its table does not list)"""
    from aivc_amd import synth
    from aivc_amd.real_life import cat_binary_files as container
    from oracle import codec as ocodec
    gop, w, h, n, seed = PADDED
    frames = synth.synthetic_video(w, h, n, seed=seed)
    blob, recs = ocodec.encode_video(spec, frames, gop)
    data_dim, first, last, gops = container.unpack_video(blob)
    return {'name': 'padded', 'gop': gop, 'frames': frames, 'blob': blob, 'recs': recs, 'dec': ocodec.decode_video(spec, blob),
            'gops': gops, 'data_dim': data_dim, 'unit': len(container.unpack_gop(gops[0])[2])}


def assert_selection(got, ref, indices, first=0):
    """a partial decode's list against the oracle's whole decode: the frames of `indices` bit for bit, None everywhere else"""
    assert len(got) == len(ref['dec'])
    assert [first + i for i, f in enumerate(got) if f is not None] == list(indices)
    sc.assert_frames([got[i - first] for i in indices], [ref['dec'][i - first] for i in indices])


def read_planes(path, w, h):
    """a planar I420 file -> the list of host plane dicts schedule_cases.assert_frames compares with"""
    hc, wc = (h + 1) // 2, (w + 1) // 2
    raw = np.fromfile(path, np.uint8).reshape(-1, h * w + 2 * hc * wc)
    return [{'y': r[:h * w].reshape(h, w), 'u': r[h * w:h * w + hc * wc].reshape(hc, wc), 'v': r[h * w + hc * wc:].reshape(hc, wc)}
            for r in raw]


class WorkSpies:
    """What a decode worked on, in order: ('e' | 's', frame type, number of frames) per entropy launch and synthesis batch
    of FrameCodec class-wide, and every frame record codec.split_sections was handed (by the section check, the byte
    estimate and the entropy stage alike)."""

    def __init__(self, monkeypatch):
        from aivc_amd import codec
        self.calls, self.parsed = [], []
        split, ent, syn = codec.split_sections, codec.FrameCodec.entropy_decode, codec.FrameCodec.synthesise_batch
        spies = self

        def spy_split(b):
            spies.parsed.append(bytes(b))
            return split(b)

        def spy_entropy(self, frames_bytes, frame_type, *a, **kw):
            spies.calls.append(('e', frame_type, len(frames_bytes)))
            return ent(self, frames_bytes, frame_type, *a, **kw)

        def spy_synthesis(self, y_hats, prev, nxt, frame_type, data_dim):
            spies.calls.append(('s', frame_type, int(y_hats['cod'].shape[0])))
            return syn(self, y_hats, prev, nxt, frame_type, data_dim)
        monkeypatch.setattr(codec, 'split_sections', spy_split)
        monkeypatch.setattr(codec.FrameCodec, 'entropy_decode', spy_entropy)
        monkeypatch.setattr(codec.FrameCodec, 'synthesise_batch', spy_synthesis)

    def clear(self):
        del self.calls[:], self.parsed[:]

    def frames(self, stage):
        return sum(n for s, _, n in self.calls if s == stage)

    def batches(self, stage):
        return sum(1 for s, _, _ in self.calls if s == stage)
