"""encode(param) with the reference's signature and RESULT lines (src/real_life/encode.py), reading a raw video
file (aivc_amd.rawvideo, the one reader), or -- when sequence_path is a directory -- the reference's folders of PNG pictures."""
import os
import time

import numpy as np
import torch

from ..codec import FrameCodec
from ..func_util.console_display import print_log_msg
from ..func_util.nn_util import get_value
from ..options import SOURCE, Source


def read_yuv(path, first=0, last=-1, device=None, pix_fmt=None):
    """A raw video file -> (the frames first ... last as dicts of uint8 planes {'y','u','v'} [1, h', w'] on `device`, first, last).
    Every file goes through the one reader, aivc_amd.rawvideo.open_raw: the file's bytes to the device in batches, one ingest launch
    per batch, the frames views into the batches' stacks.  A headerless planar 8-bit 4:2:0 file's planes are its bytes; anything else
    (a .y4m file, a named pix_fmt, a name with a _422 / _444 / _10b ... token) prints one `[INFO] input:` line.  A request outside
    the file is an aivc_amd.rawvideo.RawVideoError that names the file's range."""
    from .. import parallel, rawvideo
    with rawvideo.open_raw(path, pix_fmt) as reader:
        first, last = reader.frame_range(first, last)
        frames = reader.read(first, last, device)
    if not reader.is_plain and parallel.rank_world()[0] == 0:
        print('[INFO] input: %s %dx%d, %d frames (converted to 8-bit 4:2:0 on the device)'
              % (reader.pix_fmt.name, reader.w, reader.h, len(frames)))
    return frames, first, last


def read_png_folder(path, first=0, last=-1, device=None, reader=SOURCE.png_reader, colour=SOURCE.colour, chroma_down=SOURCE.chroma_down):
    """A folder of the reference's pictures (func_util.img_processing.load_frames: PNG triplets in the old or the clic
    layout, or one RGB PNG per frame; detected from the file names) -> the same list of uint8 plane dicts as read_yuv.
    Frame indices are the ones in the file names; the frame size is the first picture's.  RGB pictures are converted on
    the device and have the reference's floor-sized chroma planes, the codec stores ceil-sized ones: an odd frame size is
    refused for them.  reader: 'pillow' (the default), or 'device' for pictures inflated and unfiltered on the device
    (aivc_amd.png.read_pictures: the same planes); rank 0 then prints one `[INFO] input:` line.
    colour: None (the default) -- RGB pictures become planes by Pillow's arithmetic (BT.601, full range); an
    aivc_amd.color.ColourSpec -- by that matrix and range, chroma_down 'point' (the default) or 'box' (aivc_amd/color.py); rank 0
    then prints one `[INFO] colour:` line.  With a folder of PNG triplets either is a ValueError (load_frames): nothing is converted
    there."""
    from .. import color, parallel, png
    from ..func_util import img_processing as ip
    png.check_reader(reader)
    mode, rgb, present = ip.detect_folder_layout(path)
    last = present[-1] if last < 0 else last
    stats = {'device': 0, 'pillow': 0}
    loaded = ip.load_frames({'sequence_path': path, 'idx_starting_frame': first, 'nb_frame_to_load': last - first + 1,
                             'rgb': rgb, 'loading_mode': mode, 'device': device, 'png_reader': reader, 'png_stats': stats,
                             'colour': colour, 'chroma_down': chroma_down})
    if colour is not None and parallel.rank_world()[0] == 0:
        print(color.info_line(colour, chroma_down))
    if reader == 'device' and parallel.rank_world()[0] == 0:
        print('[INFO] input: %d pictures inflated on the device, %d read by Pillow' % (stats['device'], stats['pillow']))
    frames = [ip.u8_planes(loaded['frame_%d' % i]) for i in range(last - first + 1)]
    h, w = frames[0]['y'].shape[-2:]
    for fr in frames:
        if tuple(fr['y'].shape[-2:]) != (h, w) or tuple(fr['u'].shape[-2:]) != ((h + 1) // 2, (w + 1) // 2):
            raise ValueError('%s: luma %s with chroma %s: every frame must have the size of the first (%d x %d) and 4:2:0 '
                             'chroma of the ceil size (RGB pictures: even sides)'
                             % (path, tuple(fr['y'].shape[-2:]), tuple(fr['u'].shape[-2:]), w, h))
    return frames, first, last


def encode(param):
    """working_dir: '' (the default) -- no log; a directory -- the reference's per-frame table <working_dir>/detailed.txt
    (func_util/result_logging.py) is written from statistics scored on the device while the frames are coded
    (aivc_amd/quality.py), the PSNR line comes from the exact integer squared error, an `Estimated MS-SSIM` line follows it
    and the returned dictionary gains ms_ssim_db, h, w and nb_coded_frames.  The bitstream is the same either way.
    idx_rate: the rate index of the whole clip, or a list with one per intra-period unit.  target_bpp > 0 (instead of an
    idx_rate): every unit gets the richest rate index of the grid 0, rate_step, ..., nb_rates - 1 whose GOP record fits
    target_bpp x w x h x (frames of the unit) / 8 bytes (aivc_amd/rate_control.py: a few bitstream-only encodes, then the
    final one); one `[RATE]` line per unit, a `[WARN]` line for a unit that does not fit at any rate; the returned dictionary
    gains 'rates'.  Under torch.distributed.run every rank searches the units it codes.
    digests: True -- the sidecar manifest '<final_file>.md5' (aivc_amd/digests.py): the arithmetic contract the encode ran in
    and one MD5 per reconstructed plane, computed on the device where the planes lie (aivc_amd.ops.md5_planes); every rank
    digests the frames of its units, rank 0 writes the file.  The bitstream is the same with and without it.
    scene_cut: None (the default) -- the clip is cut into units by counting, and nothing below runs; a threshold in grey levels
    -- the sums of absolute differences between consecutive luma planes come from the device (aivc_amd.ops.pair_sad_u8), the
    frames that stand out over both neighbours by at least the threshold open a new intra-period unit (aivc_amd/scene.py: the
    units in front of a cut take a shorter structure, which their GOP headers state; any decoder of the format reads the
    stream), one `[SCENE]` line per cut and an `[INFO] units` line are printed, and the returned dictionary gains 'cuts' and
    'unit_names'.  Under torch.distributed.run every rank computes the same sums and the same layout.
    size: None (the default) -- the clip is coded at the size it arrives in, and nothing below runs; (w, h) -- every plane is
    resized on the device right after it has been read (func_util.img_processing.resize_frames: Pillow's Image.resize byte for
    byte, filter `resample`, one of aivc_amd.resize.FILTERS, default bicubic; y to h x w, u and v to the ceil half size, each plane
    on its own, chroma siting ignored; RGB pictures are converted to 4:2:0 first).  Everything from there on sees the coded
    size: the header, the scene cuts, the digests, the w x h of the byte budget, the sharding -- and the quality log, whose
    PSNR and MS-SSIM score the reconstruction against the RESIZED source.  The stream has no display-size field: the decoder
    is told the size to write (decode_one_video: out_size).  Every rank resizes the clip it read.
    pix_fmt: None (the default) -- a .y4m file says what it holds, a headerless file's name does (read_yuv); a name of
    aivc_amd.rawvideo.PIX_FMTS -- the layout of a headerless file.  The conversion to the 8-bit 4:2:0 planes that are coded runs
    on the device before everything else, the resize included: header, scene cuts, digests, budgets and the quality log see the
    converted planes, and the log scores against the CONVERTED source.
    png_reader: 'pillow' (the default) or 'device', who reads the pictures of a folder (read_png_folder); 'device' with a
    sequence_path that is no directory is a ValueError.  The bitstream is the same either way.
    colour: None (the default) -- the RGB pictures of a folder become planes by Pillow's arithmetic (BT.601, full range), and
    nothing below runs; an aivc_amd.color.ColourSpec (BT.601 / 709 / 2020, full or limited range) -- by that matrix and range, in
    integers on the device (aivc_amd/color.py), chroma_down 'point' (the default: the chroma of pixel (2i, 2j)) or 'box' (of the
    2 x 2 block, rounded once).  The conversion runs before the resize, like pix_fmt: header, scene cuts, digests, budgets and
    the quality log see the converted planes.  One `[INFO] colour:` line is printed.  A sequence_path that holds planes already
    (a raw video file, a folder of PNG triplets) is a ValueError.  The stream stores no colour description, as it stores no
    frame rate and no display size: the decoder is told too (decode_one_video: colour).
    The stages: _source (file or folder -> frames), _code (frames -> bitstream), the gathers of what every rank found,
    _write_outputs (manifest, debug digests, bitstream), _report (RESULT lines and the returned dictionary)."""
    default = {'model': None, 'sequence_path': '', 'GOP_struct_name': '', 'GOP_struct': None, 'idx_rate': 0.,
               'final_file': '', 'flag_bitstream_debug': False, 'idx_starting_frame': 0, 'idx_end_frame': -1,
               'working_dir': '', 'target_bpp': 0., 'rate_step': 1 / 16, 'digests': False, 'scene_cut': None, **SOURCE._asdict()}
    model = get_value('model', param, default)
    seq = get_value('sequence_path', param, default)
    gop_name = get_value('GOP_struct_name', param, default)
    final_file = get_value('final_file', param, default)
    first = get_value('idx_starting_frame', param, default)
    last = get_value('idx_end_frame', param, default)
    working_dir = get_value('working_dir', param, default)
    idx_rate = get_value('idx_rate', param, default)
    target_bpp = get_value('target_bpp', param, default)
    scene_cut = get_value('scene_cut', param, default)
    want_digests = get_value('digests', param, default)
    dev = next(model.parameters()).device
    if first > last and last != -1:
        print('ERROR: First frame index bigger than last frame index')
        return
    frames, first, last = _source(seq, first, last, dev, Source.from_param(param))
    print_log_msg('INFO', 'Start encoding', '', '')
    t0 = time.time()
    fc = FrameCodec(model)
    from . import bitstream
    from .. import parallel
    fc.estimated_bits, fc.coded_payload_bytes = 0.0, 0
    rank, world = parallel.rank_world()
    stats = None
    if working_dir:
        from ..quality import QualityStats
        stats = QualityStats()
    layout, cuts = None, None
    if scene_cut is not None:
        layout, cuts = _scene_layout(frames, gop_name, float(scene_cut), first, rank)
    n = last - first + 1
    with torch.no_grad(), bitstream.estimating_rate():  # the reference's in-band rate check (RESULT lines)
        blob, enc, rates = _code(fc, frames, gop_name, first, last, idx_rate, target_bpp, get_value('rate_step', param, default),
                                 stats, layout, rank, world, dev)
        # this rank's frames that are not padding (all of the clip's on one GPU): (position in the clip, reconstruction)
        own = [(idx, r) for idx, r in _own_frames(enc) if idx < n]
        digested = None
        if want_digests:  # (queued behind the encode, before the device is waited for)
            from .. import ops
            from .decode import digest_frames
            contract = ops.precision_name()
            digested = digest_frames([r for _, r in own], dev) if own else None
        torch.cuda.synchronize()
    dt = time.time() - t0
    est_bits, payload = fc.estimated_bits, float(fc.coded_payload_bytes)
    se = cnt = 0.0  # squared error of the frames THIS process reconstructed, summed over the ranks
    if stats is None:  # (else scored on the device already)
        for idx, r in own:
            se += sum(float(((r[k].float() - frames[idx][k].float()) ** 2).sum()) for k in 'yuv')
            cnt += sum(frames[idx][k].numel() for k in 'yuv')
    if world > 1:
        import torch.distributed as dist
        t = torch.tensor([se, cnt, est_bits, payload], dtype=torch.float64, device=parallel._comm_device(None, dev))
        dist.all_reduce(t)
        se, cnt, est_bits, payload = (float(v) for v in t)
    seq_res = None
    if stats is not None:  # every rank scored the frames of its units: the rows travel to rank 0 (to all, in fact)
        from ..model_mngt.model_management import lambda_tradeoff_of, sequence_result_from_rows, write_detailed_log
        rows = parallel.gather_quality_rows(stats.rows(), enc['layout'].keys(), dev)
        if rank == 0:
            lambdas = [lambda_tradeoff_of(model, r) for r in rates] if isinstance(rates, (list, tuple)) \
                else lambda_tradeoff_of(model, rates)
            seq_res = sequence_result_from_rows(rows, enc['nb_gop'], enc['layout'], first, n, lambdas)
            write_detailed_log(working_dir, seq_res, _sequence_name(seq))
    manifest = None
    if want_digests:  # 48 bytes per frame travel to rank 0 (to all, in fact), like the quality rows
        host = [] if digested is None else [t.cpu().numpy() for t in digested]  # y, u, v: [frames of this rank, 16] each
        rows = {first + idx: b''.join(d[k].tobytes() for d in host) for k, (idx, _) in enumerate(own)}
        if world > 1:
            rows = parallel.gather_bytes_all(rows, list(range(first, first + n)), None, world, dev)
        manifest = (contract, {i: (b[:16].hex(), b[16:32].hex(), b[32:].hex()) for i, b in rows.items()})
    debug = [(first + idx, r) for idx, r in own] if get_value('flag_bitstream_debug', param, default) else []
    _write_outputs(final_file, blob, manifest, debug, rank)
    if world > 1:
        dist.barrier()  # the file exists before any rank goes on (to decode it)
    if rank != 0:
        return None
    psnr = 10 * np.log10(255.0 ** 2 / max(se / cnt, 1e-12)) if seq_res is None else seq_res['sequence']['psnr']
    extra = {'rates': list(rates)} if target_bpp and target_bpp > 0 else {}
    if layout is not None:
        extra.update(cuts=[first + t for t in cuts], unit_names=list(layout.names))
    return _report(final_file, len(blob), n, dt, psnr, seq_res, est_bits, payload, extra)


def _source(seq, first, last, dev, source):
    """sequence_path -> (frames, first, last): a folder of pictures or a raw video file, then the optional resize.  THE ONE PLACE
    that looks at what sequence_path is; source, an aivc_amd.options.Source, is checked against it before anything is read."""
    source.check(seq)
    if os.path.isdir(seq):
        frames, first, last = read_png_folder(seq, first, last, dev, source.png_reader, source.colour, source.chroma_down)
    else:
        frames, first, last = read_yuv(seq, first, last, dev, source.pix_fmt)
    if source.size is not None:
        from ..func_util.img_processing import resize_frames
        frames = resize_frames(frames, int(source.size[0]), int(source.size[1]), source.resample, dev)
    return frames, first, last


def _sequence_name(seq):
    """the name detailed.txt gives the clip: the folder's or the file's, without the file's extension"""
    name = os.path.basename(os.path.normpath(seq))
    return name[:-4] if name.endswith(('.yuv', '.y4m')) else name


def _code(fc, frames, gop_name, first, last, idx_rate, target_bpp, rate_step, stats, layout, rank, world, dev):
    """frames -> (bitstream: None off rank 0, this rank's encode_video record, the rate index: idx_rate as given, or the list
    with one per unit that a byte budget chose).  Under a budget every rank searches its units; else one process per GPU shares
    the intra-period units out, the container on rank 0; else this process codes them all."""
    from .. import parallel
    lay = {} if layout is None else {'layout': layout}
    if target_bpp and target_bpp > 0:
        return _encode_budgeted(fc, frames, gop_name, target_bpp, rate_step, first, stats, rank, world, dev, layout)
    if world > 1:
        blob, enc = parallel.encode_video_sharded(fc, frames, gop_name, first, idx_rate=idx_rate, return_enc=True, stats=stats, **lay)
    else:
        enc = fc.encode_video(frames, gop_name, idx_starting_frame=first, idx_end_frame=last, idx_rate=idx_rate, stats=stats, **lay)
        blob = fc.assemble_video(enc)
    return blob, enc, idx_rate


def _write_outputs(final_file, blob, manifest, debug, rank):
    """the files next to the bitstream and the bitstream: rank 0 writes the manifest ((contract, rows) or None) and the
    bitstream, every rank the debug digests of its own frames ([(absolute index, reconstruction)])"""
    parent = os.path.dirname(final_file)
    if parent:
        os.makedirs(parent, exist_ok=True)
    if manifest is not None and rank == 0:
        from .. import digests
        digests.write_manifest(digests.manifest_path(final_file), manifest[0], manifest[1])
    if debug:
        from .decode import debug_dir, write_debug_md5
        for idx, r in debug:
            write_debug_md5([r], idx, debug_dir(final_file))
    if rank == 0:
        with open(final_file, 'wb') as f:
            f.write(blob)


def _report(final_file, real_byte, n, dt, psnr, seq_res, est_bits, payload, extra):
    """rank 0: the RESULT lines -> the dictionary encode() returns; extra: the entries a byte budget and scene cuts add"""
    print_log_msg('INFO', 'Encoding done', '', '')
    print_log_msg('INFO', 'Bitstream path', '', final_file)
    print_log_msg('RESULT', 'Number of frames', '[frame]', int(n))
    print_log_msg('RESULT', 'Encoding/decoding time', '[s]', '%.1f' % dt)
    print_log_msg('RESULT', 'Encoding/decoding FPS', '[frame/s]', '%.1f' % (n / dt))
    print_log_msg('RESULT', 'Estimated PSNR', '[dB]', '%.4f' % psnr)
    if seq_res is not None:
        print_log_msg('RESULT', 'Estimated MS-SSIM', '[dB]', '%.4f' % seq_res['sequence']['ms_ssim_db'])
    # The reference's in-band rate check (src/real_life/encode.py:140-170): the rate its entropy model ESTIMATES against
    # the bytes written.  Here the estimate is what the 16-bit CDF bounds price the coded symbols at (aivc_bounds_rate:
    # sum of -log2((c_hi - c_lo) / 2^16), what an ideal arithmetic coder would write for the same CDFs); the real rate
    # is the file, whose overhead over the estimate is the range coder's flush (< 2 bytes per stream), the map lists
    # and the container's length prefixes and headers.
    est_byte = est_bits / 8
    overhead = (real_byte / est_byte - 1) * 100 if est_byte > 0 else float('nan')
    print_log_msg('RESULT', 'Estimated rate', '[byte]', '%.1f' % est_byte)
    print_log_msg('RESULT', 'Real rate', '[byte]', real_byte)
    print_log_msg('RESULT', 'Estimated rate overhead', '[%]', '%.2f' % overhead)
    out = {'real_rate_byte': real_byte, 'psnr': psnr, 'nb_frames_to_code': n, 'estimated_rate_byte': est_byte,
           'rate_overhead_percent': overhead, 'range_coder_payload_byte': int(payload)}
    if seq_res is not None:
        avg = seq_res['sequence']
        out.update(ms_ssim_db=avg['ms_ssim_db'], h=avg['h'], w=avg['w'], nb_coded_frames=len(seq_res) - 1)
    out.update(extra)
    return out


def _own_frames(enc):
    """(display index in the video, reconstruction) of the frames of the units THIS process coded, padded repeats included"""
    for u, g in enumerate(enc['recs']):
        if g is not None:
            for i, r in enumerate(g):
                yield enc['layout'].position(u, i), r


def _scene_layout(frames, gop_name, threshold, first, rank):
    """The clip's scene cuts and the unit layout they give (aivc_amd/scene.py).  One launch pair over the luma planes and one
    synchronisation -- the copy of n - 1 sums to the host -- before the encode starts; with 1_GOP_0 every frame is a unit
    already and nothing is launched.  Rank 0 prints the [SCENE] and [INFO] units lines.  -> (UnitLayout, [cut positions])"""
    from .. import ops, scene
    from ..func_util.GOP_structure import generate_gop_struct
    cuts, sad, npix = [], [], frames[0]['y'].numel()
    if len(generate_gop_struct(gop_name)) > 1:
        sad = [int(v) for v in ops.pair_sad_u8([fr['y'] for fr in frames]).cpu()]
        cuts = scene.scene_cuts(sad, npix, threshold)
    layout = scene.plan_units(len(frames), cuts, gop_name)
    if rank == 0:
        for t, score in zip(cuts, scene.cut_scores(sad, npix, cuts)):
            print('[SCENE] cut at frame %d: +%.2f over its neighbours' % (first + t, score))
        print('[INFO] units: %s' % layout.summary())
    return layout, cuts


def _encode_budgeted(fc, frames, gop_name, target_bpp, rate_step, first, stats, rank, world, dev, layout=None):
    """encode() under a byte budget per unit: every rank searches and codes the units it owns (a unit's choice depends on
    that unit alone), rank 0 gets the container; the [RATE] / [WARN] lines come from rank 0, for all units.
    -> (bitstream or None, this rank's encode_video record, [rate per unit of the video])"""
    from .. import parallel, rate_control
    mine = (lambda u: parallel.unit_owner(u, world) == rank) if world > 1 else None
    enc = rate_control.encode_video_budgeted(fc, frames, gop_name, target_bpp, step=rate_step, idx_starting_frame=first,
                                             stats=stats, unit_filter=mine, **({} if layout is None else {'layout': layout}))
    report = {u: (ch.rate, ch.nbytes, int(ch.over_budget)) for u, ch in enumerate(enc['choices']) if ch is not None}
    if world > 1:
        import struct
        keys = list(range(enc['nb_gop']))
        got = parallel.gather_bytes_all({u: struct.pack('>dqq', *v) for u, v in report.items()}, keys, None, world, dev)
        report = {u: struct.unpack('>dqq', b) for u, b in got.items()}
    blob = parallel.assemble_video_sharded(fc, enc, dev)
    rates = [report[u][0] for u in range(enc['nb_gop'])]
    if rank == 0:
        for u in range(enc['nb_gop']):
            r, nbytes, over = report[u]
            print('[RATE] unit %d: idx_rate %s %d B / %d B' % (u, ('%.4f' % r).rstrip('0').rstrip('.'), nbytes, enc['budgets'][u]))
            if over:
                print('[WARN] unit %d: %d B at its leanest rate index, over its budget of %d B' % (u, nbytes, enc['budgets'][u]))
    return blob, enc, rates
