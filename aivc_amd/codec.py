"""In-memory frame / GOP / video codec on device-resident tensors: the orchestration the
reference spreads over FullNet.GOP_forward (missing from the snapshot), Decoder.decode
(src/real_life/decode.py:455-580), decode_one_GOP (:193-327) and infer_one_sequence
(src/model_mngt/model_management.py:31-244) -- without PNG round trips, temp files or per-latent
device->host CDF copies.  Frames are dicts {'y','u','v'} of uint8 CUDA planes [1,h,w] (8-bit
references are exact: the reference casts every reconstruction to 8-bit levels, decode.py:575).
"""
import contextlib
import os as _os

import torch

from . import abi, ops, partial, rate_control, scene
from .func_util.GOP_structure import FRAME_B, FRAME_I, FRAME_P, coding_levels, generate_gop_struct
from .real_life import cat_binary_files as container
from .real_life import header as hdr
from .real_life.bitstream import finalize_frames, launch_finalize, prepare_finalize, split_sections


def frame_index(name):
    return int(name.split('_')[-1])


def _stack(planes_list):
    return {k: torch.cat([p[k] for p in planes_list], dim=0) for k in 'yuv'}


def _rows_of(entries):
    """[(batch tensor, row), ...] -> the rows as one batch: a VIEW when they are consecutive rows of one tensor (the
    frames of a dependency level sit together in the entropy stage's level-major launches), else a copy"""
    t0, j0 = entries[0]
    if all(t is t0 and j == j0 + i for i, (t, j) in enumerate(entries)):
        return t0[j0:j0 + len(entries)]
    return torch.cat([t[j:j + 1] for t, j in entries], dim=0)


def _unstack(planes, n):
    return [{k: planes[k][i:i + 1] for k in 'yuv'} for i in range(n)]


def make_data_dim(h, w, dim_y, dim_z):
    return {'x': (h, w), 'y': dim_y, 'z': dim_z, 'x_uv': ((h + 1) // 2, (w + 1) // 2)}


def _refs444(prev, nxt, frame_type):
    """the references of P / B frames (planar 4:2:0) as NHWC [n,h,w,4] (y,u,v,0); zeros where there is no next one"""
    prev444 = ops.yuv420_to_444(prev['y'], prev['u'], prev['v'], c_store=4)
    if frame_type != FRAME_B:
        return prev444, torch.zeros_like(prev444)
    return prev444, ops.yuv420_to_444(nxt['y'], nxt['u'], nxt['v'], c_store=4)


def _pend_sections(net, a, sections, k):
    """queue the z and y streams of one network's analyse result as sections k, k + 1 of every frame of the batch"""
    for i, (sz, sy) in enumerate(zip(net.ac.pend_z(a['q_z']), net.ac.pend_y(a['q_y'], a['sigma']))):
        sections[i][k], sections[i][k + 1] = sz, sy


# ---- the plan of one dependency level: which frames, in which batches, on which rank, and what the ranks of a group
# exchange afterwards.  FrameCodec.encode_units / decode_units and the generic drivers of aivc_amd.parallel (which the
# CPU tests run over gloo) all walk it through these functions: every rank of a group sees the same levels, frame types
# (sorted) and frames in the same order, which is what keeps their collectives paired.
def frame_types(gop, frames):
    return sorted({gop[f]['type'] for f in frames})


def level_items(gop, level, unit_ids, ftype, need=None):
    """[(unit, frame name), ...] of one frame type in a level: unit-major, then the level's order.
    need (a partial decode): {unit: the frames of it that are decoded}; None: all of every unit"""
    return [(u, f) for u in unit_ids for f in level if gop[f]['type'] == ftype and (need is None or f in need[u])]


def level_batches(gop, level, unit_ids, max_batch, shard=None, need=None):
    """(frame type, [(unit, frame name), ...]) batches of at most max_batch same-type frames of one
    dependency level (a level of a chained GOP mixes P and B frames); with a shard, this rank's share."""
    for ftype in frame_types(gop, level):
        items = level_items(gop, level, unit_ids, ftype, need)
        if shard is not None:
            items = shard.mine(items)
        for s in range(0, len(items), max_batch):
            yield ftype, items[s:s + max_batch]


def share_level(shard, rec, gop, level, unit_ids, h, w, device):
    """Every rank of the group has written the reconstructions of ITS frames of the level into rec[unit][frame]; one
    exchange per frame type fills in those of its peers (they are the references of the next levels).  A collective:
    all ranks of the group call it for a level, or none does."""
    if shard is None or shard.R == 1:
        return
    for ftype in frame_types(gop, level):
        every = level_items(gop, level, unit_ids, ftype)
        got = shard.exchange_frames(every, [rec[u][f] for u, f in shard.mine(every)], h, w, device)
        for (u, f), r in zip(every, got):
            rec[u][f] = r


class FrameCodec:
    """max_batch bounds how many frames of one dependency level are pushed through the transforms
    together (activations of a 1080p frame at 1/2 resolution are 133 MB per 64-channel tensor; 16 frames
    measured 2.3 % faster than 8 at 1080p -- fewer, larger launches: less drain / ramp time between the
    ~12 k stream-ordered kernels of a step -- 32 adds 0.4 %)."""

    def __init__(self, full_net, max_batch=16, entropy_chunk=64, entropy_streams=8, entropy_lookahead=None,
                 flag_md5sum=False):
        self.net = full_net
        self.entropy_chunk = entropy_chunk
        self.entropy_streams = max(2, entropy_streams)  # decoder: concurrent range-coder chains
        # ... issued this many dependency levels ahead of the synthesis; None / 0: the whole video up front (when its
        # CDF windows fit in memory, _entropy_budget)
        self.entropy_lookahead = max(1, entropy_lookahead) if entropy_lookahead else None
        self.mof = full_net.mode_net.mode_net
        self.cod = full_net.codec_net.codec_net
        self.max_batch = max_batch
        # debug (src/real_life/bitstream.py:209-211): a feature-wise md5 in front of every section, checked by
        # the decoder; both ends must agree on the flag (it is not signalled in the bitstream)
        for net in (self.mof, self.cod):
            if getattr(net, 'ac', None) is not None:
                net.ac.flag_md5sum = bool(flag_md5sum)

    def encode_batch(self, cur, prev, nxt, frame_type, idx_rate=0., want_aux=False, on_sections=None, want_rec=True):
        """Encode n frames of the same type together.  cur/prev/nxt: lists of uint8 plane dicts
        (prev/nxt ignored where the frame type has no such reference).
        idx_rate: a scalar, or one rate per frame of the batch (frames of units coded at different rates: the latent stages
        then use one gain row per image, include/aivc_hip_rates.h; the same rate n times is the scalar path).
        -> list of {'bytes', 'rec', 'data_dim'[, 'aux']}
        on_sections(sections): called once every latent of the batch is quantised -- BEFORE the CodecNet synthesis is
        queued -- so that the caller can send the non-zero-map flags on their way to the host (prepare_finalize)
        half a batch earlier than the reconstructions exist.
        want_rec=False: the frames are no other frame's reference and the caller only wants their bitstream -- the
        CodecNet synthesis (g_a_ref of the prediction, g_s, the 8-bit cast) is not run, 'rec' is [None] * n; the
        sections are the same bytes either way (nothing the entropy coder reads depends on the reconstruction)."""
        n = len(cur)
        h, w = cur[0]['y'].shape[-2:]
        dev = cur[0]['y'].device
        cur_p = _stack(cur)
        sections = [[None] * 4 for _ in range(n)]
        pred = skip = None
        aux = {}
        if frame_type != FRAME_I:
            prev_p = _stack(prev)
            next_p = _stack(nxt) if frame_type == FRAME_B else None
            # lazy stacks of 3-channel images: the first conv reads the sources itself (aivc_conv_images); they are packed
            # only if a layer cannot
            a = self.mof.analyse(ops.ImageStack((cur_p, prev_p, next_p), h, w, dev), frame_type, idx_rate)
            _pend_sections(self.mof, a, sections, 0)
            pred, skip, wb = self._predict(a['y_hat'], prev_p, next_p, frame_type, h, w, want_aux)
            if want_aux:
                aux.update(alpha=wb['alpha'], beta=wb['beta'], warping=wb['x_warp'][..., :3])
        c = self.cod.analyse(ops.ImageStack((cur_p, pred), h, w, dev), frame_type, idx_rate)
        _pend_sections(self.cod, c, sections, 2)
        if on_sections is not None:
            on_sections(sections)
        rec_p = self._reconstruct_planes(self.cod.synthesise(c['y_hat'], pred), skip, h, w) if want_rec else None
        recs = _unstack(rec_p, n) if want_rec else [None] * n
        if want_aux:
            aux['code'] = ops.yuv420_to_444(cur_p['y'], cur_p['u'], cur_p['v'], c_store=3)
            # the batch's planes as the kernels hold them, stacked per plane (the quality log scores them in place)
            aux['cur_planes'], aux['rec_planes'] = cur_p, rec_p
        return {'sections': sections, 'rec': recs, 'data_dim': make_data_dim(h, w, c['dim_y'], c['dim_z']), 'aux': aux}

    def _predict(self, y_hat_mof, prev_p, next_p, frame_type, h, w, want_aux=False):
        """MOFNet synthesis + motion compensation of a batch of P / B frames (prev_p / next_p: their stacked references)
        -> (prediction, skip part, everything warp_blend returned)"""
        short_in = ops.ImageStack((prev_p, next_p), h, w, prev_p['y'].device) if frame_type == FRAME_B else None
        mof_out = self.mof.synthesise(y_hat_mof, short_in)
        prev444, next444 = _refs444(prev_p, next_p, frame_type)
        wb = ops.warp_blend(mof_out, prev444, next444, h, w, frame_type, co=4, want_aux=want_aux)
        wb['pred']._aivc_cmap = (0, 1, 2)  # 3 real channels + a zero pad channel
        return wb['pred'], wb['skip'], wb

    @staticmethod
    def _reconstruct_planes(cod_out, skip, h, w):
        """CodecNet's output (+ the skip part) -> the batch's 8-bit reconstructions, stacked per plane"""
        _, rec8 = ops.frame_to_yuv420(cod_out, h, w, skip=skip, want_float=False)
        return dict(zip('yuv', rec8))

    @classmethod
    def _reconstruct(cls, cod_out, skip, h, w, n):
        """... as the n frames' plane dicts"""
        return _unstack(cls._reconstruct_planes(cod_out, skip, h, w), n)

    # ---- one frame in row bands over the ranks of a unit group (aivc_amd/bands.py) --------------------------------
    def _band_frame(self, bands, h):
        """fix the row partition for a frame of h rows: the y grid's rows are split evenly over the ranks"""
        from .bands import count_down
        k = count_down(self.cod.g_a)
        h_y = h
        for _ in range(k):
            h_y = (h_y + 1) // 2
        bands.set_frame(h_y, k)
        return k

    def _band_motion(self, bands, y_hat_mof, prev, nxt, frame_type, h, w, kf):
        """MOFNet synthesis + motion compensation in bands -> (pred band, skip band) of this rank's frame rows"""
        from .bands import Band, BandImages
        prev444, next444 = _refs444(prev, nxt, frame_type)
        short_in = BandImages(bands, (prev, nxt), h, w, kf) if frame_type == FRAME_B else None
        mof_out = self.mof.synthesise(y_hat_mof, short_in, bands=bands)
        b0, b1 = bands.own(kf, h)
        if b1 > b0:
            wb = ops.warp_blend(mof_out.t[:, b0 - mof_out.g0:], prev444, next444, h, w, frame_type, co=4, rows=(b0, b1 - b0))
            pred, skip = wb['pred'], wb['skip']
        else:
            pred = skip = torch.empty((1, 0, w, 4), dtype=torch.float32, device=prev444.device)
        return Band(bands, pred, b0, h, kf, b0, b1), Band(bands, skip, b0, h, kf, b0, b1)

    def _band_reconstruct(self, bands, cod_out, skip, h, w, kf):
        """this rank's rows of the 8-bit reconstruction, then the whole planes on every rank (they are references)"""
        b0, b1 = bands.own(kf, h)
        dev = cod_out.t.device
        planes = None
        if b1 > b0:
            _, rec8 = ops.frame_to_yuv420(cod_out.rows(b0, b1), b1 - b0, w, skip=None if skip is None else skip.rows(b0, b1),
                                          want_float=False)
            planes = dict(zip('yuv', rec8))
        return bands.gather_planes(planes, h, w)

    def encode_banded(self, cur, prev, nxt, frame_type, idx_rate, bands, on_sections=None):
        """encode_batch for ONE frame whose transforms are spread in row bands over the ranks of `bands`
        (every rank passes the same frames).  The latents (all-gathered) and hence the sections are identical on all
        ranks; the caller lets one of them range-code.  -> like encode_batch (one frame)."""
        from .bands import BandImages
        h, w = cur['y'].shape[-2:]
        kf = self._band_frame(bands, h)
        sections = [[None] * 4]
        pred = skip = None
        if frame_type != FRAME_I:
            nx = nxt if frame_type == FRAME_B else None
            a = self.mof.analyse(BandImages(bands, (cur, prev, nx), h, w, kf), frame_type, idx_rate, bands=bands)
            _pend_sections(self.mof, a, sections, 0)
            pred, skip = self._band_motion(bands, a['y_hat'], prev, nxt, frame_type, h, w, kf)
        c = self.cod.analyse(BandImages(bands, (cur, pred), h, w, kf), frame_type, idx_rate, bands=bands)
        _pend_sections(self.cod, c, sections, 2)
        if on_sections is not None:
            on_sections(sections)
        cod_out = self.cod.synthesise(c['y_hat'], None if pred is None else BandImages(bands, (pred,), h, w, kf), bands=bands)
        rec = self._band_reconstruct(bands, cod_out, skip, h, w, kf)
        return {'sections': sections, 'rec': [rec], 'data_dim': make_data_dim(h, w, c['dim_y'], c['dim_z']), 'aux': {}}

    def synthesise_banded(self, y_hats, prev, nxt, frame_type, data_dim, bands):
        """synthesise_batch for ONE frame in row bands (y_hats: the frame's decoded latents, on every rank)"""
        from .bands import BandImages
        h, w = data_dim['x']
        kf = self._band_frame(bands, h)
        pred = skip = None
        if frame_type != FRAME_I:
            pred, skip = self._band_motion(bands, y_hats['mof'], prev, nxt, frame_type, h, w, kf)
        cod_out = self.cod.synthesise(y_hats['cod'], None if pred is None else BandImages(bands, (pred,), h, w, kf), bands=bands)
        return self._band_reconstruct(bands, cod_out, skip, h, w, kf)

    @staticmethod
    def _banded(shard, n_frames, h, w):
        """A dependency level with fewer frames than the group has ranks can be coded frame by frame in row bands over
        all of them (configs[4]: the 1-, 1-, 1-, 2-, 4-frame levels of a single 4K unit on 8 GPUs).  It pays when a
        band's kernels plus ~70 halo exchanges per frame beat one rank doing the frame alone
        (profiles/r04_band_stats_*.json: per-rank kernel time 8.0 vs 29.0 ms for a 4K B frame on 8 ranks, 5.8 vs 9.0 ms at
        1080p on 4, but 7.7 vs 9.1 ms at 1080p on 2): by default from 4 ranks per group on, or from 2 for frames of >= 6 Mpixel.
        AIVC_BAND_LEVELS=1 / 0 forces it on / off (every rank must see the same value).  Under version 2 of the contract
        (the default) bands are opt-in: AIVC_BAND_LEVELS=1 or shard.band_levels = True."""
        if shard is None or shard.R <= 1 or n_frames >= shard.R:
            return False
        # Row bands are bit exact because every output element of version 1 of the contract is one chain over its own window
        # whatever tensor the window is cut from.  Version 2 (Winograd chains, ops.set_precision('fp32w')) computes an output
        # in the 2 x 2 tile of the tensor it is given and decides by that tensor's size (aivc_winograd_covers); bands keep its
        # bits too (aivc_amd/bands.py): every slab starts on the frame's tile grid, an output row of a tile reads only its own
        # 3-row window (zero-coefficient terms are skipped), and a slab launch is routed by the size of the map it was cut
        # from (ops.slab_contract).  Whether bands pay there is unmeasured (Winograd launches on slabs of ~17 latent rows),
        # so the automatic rule below stays off in that version.
        force = _os.environ.get('AIVC_BAND_LEVELS')
        if force is not None:
            return force not in ('0', '')
        mode = getattr(shard, 'band_levels', None)
        if ops.PRECISION == abi.PREC_FP32_WINO:
            return mode is True
        # shard.band_levels: True / False set by the caller (bench.py turns it on once its warm-up clip came out
        # byte-identical to a single-process encode over the same transport), None = automatic.  The automatic rule
        # applies over gloo / threads, where the byte identity is tested; over RCCL the point-to-point halo exchange on
        # a split sub-group has never run on hardware available to the build (one GPU per lease), so there it stays
        # opt-in until a caller has verified it (tools/rccl_preflight.py --codec, bench.py).
        if mode is not None:
            return bool(mode)
        if getattr(shard, 'backend', None) == 'nccl':
            return False
        return shard.R >= 4 or h * w >= 6000000

    def encode_frame(self, cur, prev, nxt, frame_type, idx_rate=0., want_aux=False):
        out = self.encode_batch([cur], [prev], [nxt], frame_type, idx_rate, want_aux)
        res = {'bytes': finalize_frames(out['sections'])[0], 'rec': out['rec'][0], 'data_dim': out['data_dim']}
        if want_aux:
            res['aux'] = out['aux']
        return res

    def entropy_decode(self, frames_bytes, frame_type, data_dim, idx_rate=0., device=None, streams=None):
        """Entropy stage of the decoder for n frames of one type: z streams -> h_s -> (mu, sigma) ->
        y streams -> y_hat.  It depends on the bitstream only (never on reconstructed frames), so the
        caller may run it for every frame of a video up front, all streams concurrently.
        -> {'mof': y_hat [n,h_y,w_y,C] or None, 'cod': y_hat}
        idx_rate: a scalar, or one rate per frame (as in encode_batch).
        streams: optional list of HIP streams; the two networks' chains (z streams -> h_s -> y streams) are
        independent and go to streams[0] / streams[1]; then -> (dict, [event per chain])."""
        device = device or torch.device('cuda')
        secs = [split_sections(b) for b in frames_bytes]
        h_y, w_y = data_dim['y']
        h_z, w_z = data_dim['z']
        out = {'mof': None}
        events = []
        for k, (name, net, iz, iy) in enumerate((('mof', self.mof, 0, 1), ('cod', self.cod, 2, 3))):
            if name == 'mof' and frame_type == FRAME_I:
                continue
            ctx = torch.cuda.stream(streams[k % len(streams)]) if streams else contextlib.nullcontext()
            with ctx:
                q_z = net.ac.decode_z([s[iz] for s in secs], h_z, w_z, net.nb_ft_z, device)
                pay_y = [s[iy] for s in secs]
                out[name] = net.latents_from_symbols(q_z, lambda sigma: net.ac.decode_y(pay_y, sigma), frame_type,
                                                     (h_y, w_y), idx_rate)
                if streams:
                    ev = torch.cuda.Event()
                    ev.record()
                    events.append(ev)
        return (out, events) if streams else out

    def synthesise_batch(self, y_hats, prev, nxt, frame_type, data_dim):
        """Reconstruction stage (mirror of Decoder.decode, src/real_life/decode.py:455-580) for n frames
        of one type whose latents are already decoded.  -> list of uint8 plane dicts."""
        h, w = data_dim['x']
        n = y_hats['cod'].shape[0]
        pred = skip = None
        if frame_type != FRAME_I:
            prev_p = _stack(prev)
            next_p = _stack(nxt) if frame_type == FRAME_B else None
            pred, skip, _ = self._predict(y_hats['mof'], prev_p, next_p, frame_type, h, w)
        return self._reconstruct(self.cod.synthesise(y_hats['cod'], pred), skip, h, w, n)

    def decode_batch(self, frames_bytes, prev, nxt, frame_type, data_dim, idx_rate=0., device=None):
        y_hats = self.entropy_decode(frames_bytes, frame_type, data_dim, idx_rate, device)
        return self.synthesise_batch(y_hats, prev, nxt, frame_type, data_dim)

    def decode_frame(self, frame_bytes, prev, nxt, frame_type, data_dim, idx_rate=0., device=None):
        return self.decode_batch([frame_bytes], [prev], [nxt], frame_type, data_dim, idx_rate, device)[0]

    # ------------------------------------------------------------------------------------------
    # Level-synchronous scheduling: frames of one dependency level (of ALL units handed in) only
    # depend on earlier levels, so they are pushed through the networks as one batch and their
    # entropy streams are coded concurrently.  Frames are stored in display order in the container,
    # so this yields the same bytes as the reference's depth-first order.
    def _side_streams(self, k):
        """k high-priority streams for the entropy coder (few waves each, latency critical)"""
        pool = getattr(self, '_sides', None)
        if pool is None:
            pool = self._sides = []
        while len(pool) < k:
            pool.append(torch.cuda.Stream(priority=-1))
        return pool[:k]

    def stream_errors(self):
        """Sections decoded since the last call whose range decoder did not end where their payload ends (see
        ArithmeticCoder.stream_errors), plus failed md5 sections under flag_md5sum -- [(network, what, ...)].
        Waits for the decodes concerned; call it after the frames have been fetched."""
        out = []
        for name, net in (('mofnet', self.mof), ('codecnet', self.cod)):
            ac = getattr(net, 'ac', None)
            if ac is None:
                continue
            out += [(name,) + e for e in ac.stream_errors()]
            out += [(name, what + ' md5', i, 0, 0) for what, i in ac.md5_errors]
            ac.md5_errors = []
        return out

    def check_sections(self, parsed, need=None):
        """The section framing and the y map lists of EVERY frame of every unit, on the host, before any kernel or
        collective: a malformed file is then a ContainerError on every rank alike (each holds the whole bitstream) --
        with the check left to decode_y only the rank that owns the bad frame raised while its peers went on into
        the level's exchange and waited for the collective timeout.
        need (a partial decode): {unit: the frames of it that are decoded}; only those are looked at, and an entry of `parsed`
        may be None for a unit that is not decoded at all."""
        for u, rec in enumerate(parsed):
            if rec is None:
                continue
            gop_name, _, frames = rec
            gop = generate_gop_struct(gop_name)
            names = sorted(gop, key=frame_index)
            if len(names) != len(frames):
                raise container.ContainerError('unit %d: %d frames in the record, coding structure %s has %d'
                                               % (u, len(frames), gop_name, len(names)))
            for k, fb in enumerate(frames):
                if need is not None and names[k] not in need[u]:
                    continue
                secs = split_sections(fb)
                for net, sy in ((self.mof, secs[1]), (self.cod, secs[3])):
                    if net is self.mof and gop[names[k]]['type'] == FRAME_I:
                        continue
                    ac = getattr(net, 'ac', None)
                    if ac is not None:
                        ac._parse_maps(sy[32:] if ac.flag_md5sum else sy, net.nb_ft_y, k)

    def _entropy_bytes(self, parsed, members, data_dim, need=None):
        """device bytes the entropy stage of these units holds when all of it is issued at once: per coded y symbol the
        64-entry CDF window + sigma (132 B, real_life/bitstream.py _rows_workspace) + the symbol, per frame the
        hyperprior's activations and latents (bounded by 64 floats per y position per network).  The coded map counts
        are in the sections' first byte -- behind the 32-character md5 text under flag_md5sum
        (ArithmeticCoder._strip_md5) -- and never more than the format's map limit.  need (a partial decode): {unit: the frames
        of it that are decoded}; only those are counted."""
        h_y, w_y = data_dim['y']
        npix = h_y * w_y
        total = 0
        for i in members:
            for k, fb in enumerate(parsed[i][2]):
                if need is not None and 'frame_%d' % k not in need[i]:
                    continue
                secs = split_sections(fb)
                for net, sy in ((self.mof, secs[1]), (self.cod, secs[3])):
                    ac = getattr(net, 'ac', None)
                    skip = 32 if ac is not None and ac.flag_md5sum else 0
                    if len(sy) > skip:
                        total += min(sy[skip], abi.MAX_MAPS) * npix * 134 + npix * 4 * 640
        return total

    @staticmethod
    def _entropy_budget(device):
        """a quarter of the free device memory (AIVC_ENTROPY_BUDGET_GB overrides)"""
        gb = _os.environ.get('AIVC_ENTROPY_BUDGET_GB')
        if gb:
            return int(float(gb) * 2 ** 30)
        free, _ = torch.cuda.mem_get_info(device)
        return free // 4

    def _param_stamp(self):
        """changes whenever a parameter / buffer of the model is modified in place, replaced or moved"""
        ts = getattr(self, '_param_list', None)
        if ts is None:  # (walking the module tree costs 1.3 ms; the Parameter objects themselves survive .to() / load_state_dict)
            ts = self._param_list = list(self.net.parameters()) + list(self.net.buffers())
        return hash(tuple((t.data_ptr(), t._version) for t in ts))

    def _level_work(self, shard, gop, level, unit_ids, h, w, need=None):
        """-> (row-band context or None, this rank's batches of the level).  A banded level (_banded) is the same plan with
        one-frame batches of EVERY frame: every rank of the group works on each of them, a band of rows each.
        need: as in level_items (a partial decode; never with a shard)."""
        if self._banded(shard, len(unit_ids) * len(level), h, w):
            return shard.bands(), level_batches(gop, level, unit_ids, 1)
        return None, level_batches(gop, level, unit_ids, self.max_batch, shard, need)

    def encode_units(self, units, gop_name, idx_rate=0., shard=None, recon='all', stats=None, stats_units=None):
        """units: list of frame lists (display order, each len == len(GOP struct)).
        -> ([gop bytes per unit], [reconstructions per unit], data_dim)
        idx_rate: a scalar for all units, or one rate per unit: frame (u, f) of a level batch is then coded at idx_rate[u]
        (one batch may mix rates) and unit u's GOP header carries idx_rate[u].  A list is checked
        (rate_control.check_unit_rates: multiples of 1/16 inside the gain matrix, ValueError naming the unit); a scalar is
        taken as it is.  Each unit comes out with the bytes it has when coded alone at its rate.
        recon: 'all' -- every frame is reconstructed, as the reference's encoder does (its forward pass returns x_hat
        for every frame and the command line prints a PSNR from them); 'refs' -- a bitstream-only encoder: frames that
        no other frame of the GOP structure references (the last dependency level of a random-access GOP: 16 of the 33
        frames of 1_GOP_32; the last P of a low-delay chain) skip their CodecNet synthesis and come back as None.
        Same bytes (tests/test_gpu_codec.py); single-process coding only.
        stats (aivc_amd.quality.QualityStats, optional): the encoder's quality log.  Every level batch is then encoded
        with want_aux and scored on the device right after its reconstruction (squared error, alpha / beta / warping
        sums, MS-SSIM: a few launches per batch, no host synchronisation; the auxiliary tensors do not outlive the
        batch), and the four section sizes of every frame are recorded, all under (stats_units[unit], display index) --
        stats_units: the units' numbers in the video, default 0, 1, ...  Same bytes as without it.  Every frame must be
        reconstructed to be scored (not with recon='refs'), by this process (not with a shard).
        shard (aivc_amd.parallel.ClipShard, optional): the frames of every dependency level are spread over the
        ranks of this process' group; each rank codes `shard.mine(items)` and the new 8-bit reconstructions are
        exchanged once per level (they are the references of the next levels).  Stream scheduling is the
        single-GPU one; the frame bitstreams are gathered once, at the end.  Every rank of the group returns
        the same blobs -- identical to a single-process run.
        gop_name: one structure for all units, or a list with one name per unit (aivc_amd.scene.plan_units: the units around
        a scene cut): the units are grouped by structure as _decode_units_gen groups them, each group runs the level loop
        below on its own (levels of different groups are not merged), and every unit has the bytes it has when coded alone
        under its structure.  Unit-wise coding only: ValueError with a shard."""
        if not isinstance(gop_name, str):
            return self._encode_units_by_structure(units, list(gop_name), idx_rate, shard, recon, stats, stats_units)
        gop = generate_gop_struct(gop_name)
        names = sorted(gop, key=frame_index)
        rec = [dict() for _ in units]
        fbytes = [dict() for _ in units]
        data_dim = None
        sides = self._side_streams(self.entropy_streams)
        jobs = []
        waiting = None  # [(items, sections, flags on their way to the host) per batch] of the previous level
        split = shard is not None and shard.R > 1
        if recon not in ('all', 'refs'):
            raise ValueError("recon must be 'all' or 'refs'")
        if recon == 'refs' and shard is not None:
            raise ValueError("recon='refs' is a single-process option (the sharded paths exchange every reconstruction)")
        if stats is not None and recon != 'all':
            raise ValueError("a quality log scores every frame's reconstruction: stats= needs recon='all'")
        if stats is not None and shard is not None:
            raise ValueError('stats= is an option of unit-wise coding (the level-sharded paths spread a unit over ranks)')
        stats_units = list(range(len(units))) if stats_units is None else list(stats_units)
        unit_rates = None  # one rate per unit, or None: idx_rate serves them all
        if rate_control.is_rate_list(idx_rate):
            if len(idx_rate) != len(units):
                raise ValueError('%d rate indices for %d units' % (len(idx_rate), len(units)))
            unit_rates = rate_control.check_unit_rates(idx_rate, rate_control.nb_rates_of(self))

        def rate_of(chunk):
            return idx_rate if unit_rates is None else [unit_rates[u] for u, _ in chunk]
        referenced = {gop[f][k] for f in gop for k in ('prev_ref', 'next_ref') if gop[f].get(k) is not None}

        def flush(li):
            # the levels' coder launches are independent of each other: rotate the stream so that a level with
            # long streams (few frames, big latents) does not queue the following ones behind it
            k = li % len(sides)
            for items, secs, prep in waiting:
                jobs.append((items, launch_finalize(secs, sides[k], prepared=prep,
                                                    fork_streams=sides[k + 1:] + sides[:k])))

        uids = range(len(units))
        h, w = units[0][0]['y'].shape[-2:]
        n_levels = 0
        for li, level in enumerate(coding_levels(gop)):
            n_levels = li + 1
            pending = []
            bands, batches = self._level_work(shard, gop, level, uids, h, w)
            # in bands the sections are identical on every rank: the group's first rank codes them
            keep = bands is None or shard.local == 0
            for ftype, chunk in batches:
                # the flags of the batch start their trip to the host as soon as its latents are quantised, i.e.
                # before its CodecNet synthesis is queued: the LAST level's range coding then runs under that level's
                # own synthesis instead of after it (it was the exposed tail of the encoder)
                preps = []
                cur, prev, nxt = ([units[u][frame_index(f)] for u, f in chunk],
                                  [rec[u].get(gop[f]['prev_ref']) for u, f in chunk],
                                  [rec[u].get(gop[f]['next_ref']) for u, f in chunk])
                on_secs = (lambda secs: preps.append(prepare_finalize(secs))) if keep else None
                if bands is None:
                    out = self.encode_batch(cur, prev, nxt, ftype, rate_of(chunk), want_aux=stats is not None, on_sections=on_secs,
                                            want_rec=recon == 'all' or any(f in referenced for _, f in chunk))
                    if stats is not None:
                        stats.score_batch([(stats_units[u], frame_index(f)) for u, f in chunk], out.pop('aux'))
                else:
                    out = self.encode_banded(cur[0], prev[0], nxt[0], ftype, rate_of(chunk), bands, on_sections=on_secs)
                data_dim = out['data_dim']
                for (u, f), r in zip(chunk, out['rec']):
                    rec[u][f] = r
                if keep:
                    pending.append((chunk, out['sections'], preps[0]))
            # entropy coding runs on the side streams one level behind the transforms: the host picks the flags
            # up (and launches the range coder) only after the next level's transforms are queued, so the main
            # stream never drains on that wait
            if bands is None:  # every rank of the group needs this level's reconstructions before the next level
                share_level(shard, rec, gop, level, uids, h, w, units[0][0]['y'].device)
            if waiting is not None:
                flush(li - 1)
            waiting = pending if pending else None
        if waiting is not None:
            flush(n_levels - 1)
        for items, job in jobs:
            for (u, f), b in zip(items, job.collect()):
                fbytes[u][f] = b
                if stats is not None:
                    stats.add_sections((stats_units[u], frame_index(f)), [len(sec) for sec in split_sections(b)])
            # (logging, real_life.bitstream.ESTIMATE_RATE: what the CDF bounds price this rank's streams at, and what the
            # range coder wrote for them)
            self.estimated_bits = getattr(self, 'estimated_bits', 0.0) + job.est_bits
            self.coded_payload_bytes = getattr(self, 'coded_payload_bytes', 0) + job.real_bytes
        if split:
            keys = [(u, f) for u in range(len(units)) for f in names]
            allb = shard.gather_bytes({k: fbytes[k[0]][k[1]] for k in keys if k[1] in fbytes[k[0]]}, keys)
            for (u, f), b in allb.items():
                fbytes[u][f] = b
            data_dim = shard.agree(data_dim)
        heads = [hdr.gop_header_bytes(gop_name, idx_rate if unit_rates is None else unit_rates[u]) for u in range(len(units))]
        blobs = [container.pack_gop(heads[u], [fbytes[u][f] for f in names]) for u in range(len(units))]
        return blobs, [[rec[u][f] for f in names] for u in range(len(units))], data_dim

    def _encode_units_by_structure(self, units, names, idx_rate, shard, recon, stats, stats_units):
        """encode_units with one structure name per unit: one call of the single-structure path per name, in order of first use"""
        if shard is not None:
            raise ValueError('one structure per unit is an option of unit-wise coding (the level-sharded paths spread a unit '
                             'over ranks)')
        if len(names) != len(units):
            raise ValueError('%d structure names for %d units' % (len(names), len(units)))
        per_unit = rate_control.is_rate_list(idx_rate)
        if per_unit:
            if len(idx_rate) != len(units):
                raise ValueError('%d rate indices for %d units' % (len(idx_rate), len(units)))
            idx_rate = rate_control.check_unit_rates(idx_rate, rate_control.nb_rates_of(self))
        stats_units = list(range(len(units))) if stats_units is None else list(stats_units)
        groups = {}
        for u, name in enumerate(names):
            groups.setdefault(name, []).append(u)
        blobs, recs, data_dim = [None] * len(units), [None] * len(units), None
        for name, members in groups.items():
            b, r, data_dim = self.encode_units([units[u] for u in members], name,
                                               [idx_rate[u] for u in members] if per_unit else idx_rate, recon=recon,
                                               stats=stats, stats_units=[stats_units[u] for u in members])
            for u, bu, ru in zip(members, b, r):
                blobs[u], recs[u] = bu, ru
        return blobs, recs, data_dim

    def decode_units(self, gop_blobs, data_dim, device=None, shard=None, wanted=None):
        """-> [reconstructions (display order) per unit]; see _decode_units_gen."""
        return self.decode_units_finish(self.decode_units_begin(gop_blobs, data_dim, device, shard, wanted))

    def decode_units_begin(self, gop_blobs, data_dim, device=None, shard=None, wanted=None):
        """First half of decode_units: parse the records and issue the entropy stage of the WHOLE video on the side
        streams (when its CDF windows fit, _entropy_budget); nothing is queued on the main stream.  A caller with other
        main-stream work -- the next clip's encode (src/real_life/encode.py and decode.py are two processes on two
        machines in a deployment: the decoder of clip i runs while the encoder works on clip i + 1) -- issues it between
        _begin and _finish: the serial range-coder streams (the I frame's y stream at the head, 0.5 / 2.1 M symbols at
        1080p / 4K high rate) then decode under that work instead of in front of the first synthesis.
        -> a handle for decode_units_finish."""
        g = self._decode_units_gen(gop_blobs, data_dim, device, shard, wanted)
        try:
            next(g)
        except StopIteration as e:
            return ('done', e.value)
        return ('running', g)

    @staticmethod
    def decode_units_finish(handle):
        state, g = handle
        if state == 'done':
            return g
        while True:
            try:
                next(g)
            except StopIteration as e:
                return e.value

    def _decode_units_gen(self, gop_blobs, data_dim, device=None, shard=None, wanted=None):
        """-> [reconstructions (display order) per unit] (a generator: yields once per coding-structure group, right
        after that group's entropy stage has been issued up front; decode_units runs it through).  Units are grouped by
        their coding structure; each carries the rate index of its own GOP header, so a video whose units were coded at
        different rates decodes in the same level batches as a single-rate one.  shard: as in encode_units (the entropy stage only runs
        for this rank's frames; one exchange of the new reconstructions per level).
        Stage 1 entropy-decodes EVERY frame of every unit (entropy_chunk frames at a time: that many
        range-coder streams run concurrently, one wavefront each; the serial coder is off the
        frame-to-frame critical path).  Stage 2 reconstructs level by level in batches.
        wanted (a partial decode; None: everything, as above): one collection of frame names per unit, empty or None for
        a unit nothing is asked of -- that unit is not looked at (its record may be None) and comes back as None.  Of the
        others both stages run for the reference closure of the wanted frames only (`need` below restricts every list
        of frames the stages are fed from); frames of one level from different units still share a batch.  The unit's
        list keeps display order and full length, None where a frame was not asked for: an ancestor that is decoded
        but not wanted is dropped with the generator's state.  Same bits as the whole decode; not with a shard."""
        if wanted is not None and shard is not None:
            raise ValueError('wanted= is an option of unit-wise decoding (the level-sharded paths spread a unit over ranks)')
        if wanted is not None and len(wanted) != len(gop_blobs):
            raise ValueError('%d selections for %d units' % (len(wanted), len(gop_blobs)))
        parsed = [container.unpack_gop(g) if wanted is None or wanted[i] else None for i, g in enumerate(gop_blobs)]
        need = None if wanted is None else partial.closures([rec and rec[0] for rec in parsed], wanted)
        self.check_sections(parsed, need)
        out = [None] * len(gop_blobs)
        groups = {}  # by coding structure alone: the members keep their own rate index, a level batch may mix them
        for i, rec in enumerate(parsed):
            if rec is not None:
                groups.setdefault(rec[0], []).append(i)
        for gop_name, members in groups.items():
            gop = generate_gop_struct(gop_name)
            names = sorted(gop, key=frame_index)
            # entropy stage on the (high priority) side stream, one dependency level ahead of the
            # synthesis stage on the main stream; the host alternates between the two so that both
            # queues stay fed
            main, sides = torch.cuda.current_stream(), self._side_streams(self.entropy_streams)
            # The entropy stage depends on the bitstream (host memory) and on the model only -- never on what the main
            # stream is still doing (in encode -> decode sequences: the last level's synthesis of the encoder), so the
            # side streams do NOT wait for it: the first levels' serial y streams decode under that work.  (Kernel-
            # ready parameters are synchronised when they are built, layers/_cache.py.)
            # Parameters the entropy stage reads DIRECTLY (gain vectors, the hyperprior's inputs) are not behind that
            # cache (a conv bias is read in place too, but it is part of its layer's cache stamp: changing it rebuilds
            # the entry behind the cache's device-wide wait): if any parameter was modified in place or moved since the
            # last decode (an asynchronous gain.add_ of a calibration, load_state_dict, .to() -- on the main stream),
            # the side streams wait for the main stream once, here (tests/test_gpu_schedules.py).
            stamp = self._param_stamp()
            if _os.environ.get('AIVC_DEC_WAIT_MAIN') or stamp != getattr(self, '_dec_param_stamp', None):
                for sd in sides:
                    sd.wait_stream(main)
                self._dec_param_stamp = stamp
            levels = coding_levels(gop)
            if need is not None:  # a closure holds the references of its frames: the levels left empty are the deepest ones
                levels = [level for level in levels if any(f in need[i] for i in members for f in level)]
            lat, ready = {}, {}
            rr = [0]

            h, w = data_dim['x']

            def my_items(level, ftype):
                items = level_items(gop, level, members, ftype, need)
                if shard is not None and not self._banded(shard, len(members) * len(level), h, w):
                    items = shard.mine(items)  # (a banded level's latents are decoded by every rank: no exchange)
                return items

            def issue_items(ftype, items):
                for s0 in range(0, len(items), self.entropy_chunk):
                    chunk = items[s0:s0 + self.entropy_chunk]
                    pair = [sides[(rr[0] + k) % len(sides)] for k in range(2)]
                    rr[0] += 2
                    yh, evs = self.entropy_decode([parsed[i][2][frame_index(f)] for i, f in chunk], ftype,
                                                  data_dim, [parsed[i][1] for i, _ in chunk], device, streams=pair)
                    for v in yh.values():
                        if v is not None:
                            v.record_stream(main)
                    for j, it in enumerate(chunk):
                        lat[it] = {k: (None if v is None else (v, j)) for k, v in yh.items()}  # (batch tensor, row)
                        ready[it] = evs

            def issue_entropy(level):
                for ftype in frame_types(gop, level):
                    issue_items(ftype, my_items(level, ftype))

            rec = {i: {} for i in members}
            ahead = self.entropy_lookahead
            if ahead is None and self._entropy_bytes(parsed, members, data_dim, need) > self._entropy_budget(device):
                ahead = 2  # the windows of the whole group do not fit beside the activations: level by level
            if ahead is None:
                # the WHOLE group's entropy stage up front, frames of one type from all dependency levels in the same
                # launches (level-major order, so the first chunk holds the frames the synthesis needs first): every
                # serial stream of the video is then in flight at once -- what bounds the entropy stage is its longest
                # stream, not the number of levels times it (at high rate a 4K y stream decodes for > 0.3 s, and level
                # by level the synthesis of every level waited for that again)
                for ftype in frame_types(gop, names):
                    issue_items(ftype, [it for level in levels for it in my_items(level, ftype)])
                ahead = len(levels)
                yield 'entropy stage issued'  # (decode_units_begin returns here)
            else:
                for li in range(min(ahead, len(levels))):
                    issue_entropy(levels[li])
            for li, level in enumerate(levels):
                if li + ahead < len(levels):
                    issue_entropy(levels[li + ahead])
                bands, batches = self._level_work(shard, gop, level, members, h, w, need)
                for ftype, chunk in batches:
                    for ev in {id(e): e for it in chunk for e in ready[it]}.values():
                        main.wait_event(ev)
                    yh = {k: (None if lat[chunk[0]][k] is None else _rows_of([lat[it][k] for it in chunk]))
                          for k in ('mof', 'cod')}
                    prev, nxt = ([rec[i].get(gop[f]['prev_ref']) for i, f in chunk],
                                 [rec[i].get(gop[f]['next_ref']) for i, f in chunk])
                    if bands is None:
                        dec = self.synthesise_batch(yh, prev, nxt, ftype, data_dim)
                    else:
                        dec = [self.synthesise_banded(yh, prev[0], nxt[0], ftype, data_dim, bands)]
                    for (i, f), r in zip(chunk, dec):
                        rec[i][f] = r
                        del lat[(i, f)]
                if bands is None:
                    share_level(shard, rec, gop, level, members, h, w, device or torch.device('cuda'))
            for i in members:
                out[i] = [rec[i][f] if wanted is None or f in wanted[i] else None for f in names]
        return out

    def encode_gop(self, frames, gop_name, idx_rate=0.):
        blobs, recs, data_dim = self.encode_units([frames], gop_name, idx_rate)
        return blobs[0], recs[0], data_dim

    def decode_gop(self, gop_bytes, data_dim, device=None):
        return self.decode_units([gop_bytes], data_dim, device)[0]

    # ------------------------------------------------------------------------------------------
    def encode_video(self, frames, gop_name, idx_starting_frame=0, idx_end_frame=None, idx_rate=0.,
                     unit_filter=None, recon='all', stats=None, layout=None):
        """frames[i] is the frame with absolute index idx_starting_frame + i.  The last intra-period
        unit is padded by repeating the last frame (src/model_mngt/model_management.py:142-153).
        unit_filter(u) -> bool selects the units this process codes (multi-GPU sharding); skipped
        units come back as None in the returned list of GOP blobs.
        stats: see encode_units; the rows are recorded under (unit number in the video, display index in the unit).
        idx_rate: a scalar, or one rate per unit of the VIDEO (indexed by the unit's number whatever unit_filter selects;
        the entries of units filtered out are not looked at).
        layout (aivc_amd.scene.UnitLayout, optional): the units of the video, each with its own structure (scene cuts);
        default: ceil(n / unit) units of gop_name.  unit_filter, idx_rate lists and the stats rows index ITS units; the layout
        in use comes back as 'layout'."""
        n = len(frames)
        idx_end_frame = idx_starting_frame + n - 1 if idx_end_frame is None else idx_end_frame
        uniform = layout is None
        if uniform:
            layout = scene.plan_units(n, (), gop_name)
        elif layout.n_frames != n:
            raise ValueError('a layout of %d frames for a video of %d' % (layout.n_frames, n))
        nb_gop = len(layout.names)
        mine = [u for u in range(nb_gop) if unit_filter is None or unit_filter(u)]
        gops, recs, data_dim = [None] * nb_gop, [None] * nb_gop, None
        if mine:
            every = layout.units(frames)
            units = [every[u] for u in mine]
            if rate_control.is_rate_list(idx_rate):
                if len(idx_rate) != nb_gop:
                    raise ValueError('%d rate indices for the %d units of the video' % (len(idx_rate), nb_gop))
                idx_rate = rate_control.check_unit_rates([idx_rate[u] for u in mine], rate_control.nb_rates_of(self), mine)
            blobs, rr, data_dim = self.encode_units(units, gop_name if uniform else [layout.names[u] for u in mine], idx_rate,
                                                    recon=recon, stats=stats, stats_units=mine)
            for u, b, r in zip(mine, blobs, rr):
                gops[u], recs[u] = b, r
        return {'gops': gops, 'recs': recs, 'data_dim': data_dim, 'nb_gop': nb_gop,
                'idx_starting_frame': idx_starting_frame, 'idx_end_frame': idx_end_frame, 'layout': layout}

    @staticmethod
    def assemble_video(enc):
        vh = hdr.video_header_bytes(enc['data_dim'], enc['nb_gop'], enc['idx_starting_frame'],
                                    enc['idx_end_frame'])
        return container.pack_video(vh, enc['gops'])

    def decode_video(self, video, device=None, unit_filter=None, frames=None, max_level=None, plan=None):
        """video: the bytes of a container, or an aivc_amd.partial.IndexedVideo (a file read through
        real_life.cat_binary_files.index_video: records of units the request does not touch may be None).
        -> (list of uint8 plane dicts for frames idx_first..idx_last (padded frames removed), data_dim, idx_first, idx_last);
        frames of units filtered out are None, and so are frames that were not asked for.
        frames: absolute display indices (the video header's numbering, as in the manifest and the PNG names); max_level:
        only frames whose dependency depth in their unit is at most that (a level deeper than the structure selects
        everything); both: a frame must pass both; neither: the whole video.  Every unit counts with the length of its own
        coding structure.  The padded repeats behind idx_last cannot be asked for; a request decodes them where a wanted
        frame references them, the whole decode decodes all of them.  partial.FrameSelectionError (a ValueError) naming the
        stream's range for an empty selection, an index outside idx_first ... idx_last or a negative level.  What is decoded
        is the reference closure of the selection, unit by unit (decode_units, wanted=): the frames are bit-identical to
        those of a whole decode.  plan: the aivc_amd.partial.Plan of this decode where the caller has made it already
        (video, frames and max_level are then its own)."""
        plan = plan or partial.plan(video, frames, max_level)
        video = plan.video
        if unit_filter is not None:  # (every rank: the units of its peers as well, before any kernel or collective)
            self.check_sections([container.unpack_gop(g) if n else None for g, n in zip(video.gops, plan.need)], plan.need)
        mine = [u for u, n in enumerate(plan.need) if n and (unit_filter is None or unit_filter(u))]
        dec = {}
        if mine:
            dec = dict(zip(mine, self.decode_units([video.gops[u] for u in mine], video.data_dim, device,
                                                   wanted=None if plan.whole else [plan.wanted[u] for u in mine])))
        out = []
        for u, n in enumerate(partial.unit_lengths(video.names)):
            out.extend(dec.get(u) or [None] * n)
        n_real = video.last - video.first + 1
        return (out + [None] * n_real)[:n_real], video.data_dim, video.first, video.last
