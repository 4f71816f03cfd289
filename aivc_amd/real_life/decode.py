"""Frame / GOP / video decoder with the reference's class and function names
(src/real_life/decode.py).  Decoder.decode keeps the reference's dictionary contract (float YUV
dicts, one bitstream file per frame); decode_one_video reads the container and writes a raw video
file (aivc_amd.rawvideo.write_raw, the one writer), or on request a folder of RGB pictures (the reference's per-frame `dd` forks are out of scope)."""
import os
import time

import numpy as np
import torch
from torch.nn import Module

from ..codec import FrameCodec
from ..func_util.console_display import print_log_msg
from ..func_util.nn_util import get_value
from ..models.full_net import _to_float_dic, _to_u8_planes
from ..options import SINK, Sink, is_png_folder
from .utils import BITSTREAM_SUFFIX


class ConditionalDecoder(Module):
    """Decoder half of a ConditionalNet (src/real_life/decode.py:752-898): shares the sub-modules."""

    def __init__(self, param):
        super().__init__()
        net = get_value('conditional_net', param, {'conditional_net': None})
        self.net = net
        self.g_s, self.h_s = net.g_s, net.h_s
        self.g_a_ref = getattr(net, 'g_a_ref', None)
        self.pdf_y, self.pdf_z, self.pdf_parameterizer = net.pdf_y, net.pdf_z, net.pdf_parameterizer
        self.nb_ft_shortcut_out, self.nb_ft_y, self.nb_ft_z = net.out_c_shortcut_y, net.nb_ft_y, net.nb_ft_z
        self.gain_I, self.flag_gain_p_b = net.gain_I, net.flag_gain_p_b
        if self.flag_gain_p_b:
            self.gain_P, self.gain_B = net.gain_P, net.gain_B
        self.ac = net.ac


class CodecNetDecoder(Module):
    def __init__(self, param):
        super().__init__()
        self.codec_dec = ConditionalDecoder({'conditional_net': get_value('codec_net', param, {'codec_net': None}).codec_net})


class MOFNetDecoder(Module):
    def __init__(self, param):
        super().__init__()
        self.mofnet_dec = ConditionalDecoder({'conditional_net': get_value('mofnet', param, {'mofnet': None}).mode_net})


class Decoder(Module):
    """Entire decoder, built from a complete FullNet (src/real_life/decode.py:429-580)."""

    def __init__(self, param):
        super().__init__()
        full_net = get_value('full_net', param, {'full_net': None})
        self.full_net = full_net
        self.codec_net_dec = CodecNetDecoder({'codec_net': full_net.codec_net})
        self.mofnet_dec = MOFNetDecoder({'mofnet': full_net.mode_net})
        self.motion_compensation = full_net.motion_compensation
        self.in_layer, self.out_layer = full_net.in_layer, full_net.out_layer

    def decode(self, param):
        """{'prev_dic','next_dic','frame_type','bitstream_path','data_dim','idx_rate','device'} ->
        decoded frame as a float YUV dict holding 8-bit levels."""
        default = {'prev_dic': None, 'next_dic': None, 'frame_type': None, 'bitstream_path': None, 'data_dim': None,
                   'flag_bitstream_debug': False, 'idx_rate': 0., 'device': 'cuda:0'}
        dev = torch.device(get_value('device', param, default))
        path = get_value('bitstream_path', param, default)
        if not path.endswith(BITSTREAM_SUFFIX):
            path += BITSTREAM_SUFFIX
        with open(path, 'rb') as f:
            frame_bytes = f.read()

        def planes(d):
            return None if d is None else _to_u8_planes(d, dev)
        fc = FrameCodec(self.full_net)
        rec = fc.decode_frame(frame_bytes, planes(get_value('prev_dic', param, default)),
                              planes(get_value('next_dic', param, default)), get_value('frame_type', param, default),
                              get_value('data_dim', param, default), get_value('idx_rate', param, default), dev)
        return _to_float_dic(rec)


def write_png_folder(frames, directory, device, indices, coder=SINK.png_coder, colour=SINK.colour):
    """decoded frames -> <directory>/<idx>.png, RGB pictures (func_util.img_processing.save_tensor_as_img, mode 'yuv420':
    the colour conversion runs on the device, straight from the decoder's 8-bit planes).  indices: the absolute index of
    every frame handed in.  coder: 'pillow' (one Image.save per frame on the host) or 'device': the planes of a batch of at
    most 256 MiB of pixels take one colour launch and are coded on the device (aivc_amd.png.write_pictures) -- the same names,
    the same pixels, other bytes.  colour: None -- Pillow's YCbCr -> RGB (BT.601, full range); an aivc_amd.color.ColourSpec --
    the planes carry that matrix and range (aivc_amd/color.py), with either coder"""
    from .. import png
    png.check_coder(coder)
    os.makedirs(directory, exist_ok=True)
    if coder == 'device' and frames:
        from .. import rawvideo
        from ..func_util.img_processing import _planes_to_rgb
        h, w = frames[0]['y'].shape[-2:]
        per = max(1, rawvideo.BATCH_BYTES // (3 * h * w))
        for i0 in range(0, len(frames), per):
            part = frames[i0:i0 + per]
            y, u, v = (torch.cat([torch.as_tensor(fr[k]).to(device).reshape((1,) + tuple(fr[k].shape[-2:])) for fr in part]) for k in 'yuv')
            png.write_pictures(_planes_to_rgb(y, u, v, 1, colour), [os.path.join(directory, '%d.png' % idx) for idx in indices[i0:i0 + per]])
        return
    from ..func_util.img_processing import save_tensor_as_img
    for idx, fr in zip(indices, frames):
        save_tensor_as_img({k: torch.as_tensor(fr[k]).to(device) for k in 'yuv'}, os.path.join(directory, '%d.png' % idx), mode='yuv420',
                           colour=colour)


def digest_frames(frames, device):
    """frames: a list of dicts of uint8 planes [1, h, w] (device tensors, or host tensors / arrays: those are copied over)
    -> three uint8 device tensors [n, 16], the MD5 of every y, u and v plane (aivc_amd.ops.md5_planes: one launch per kind of
    plane, so that the equal-sized planes of a kind share wavefronts; no synchronisation)"""
    from .. import ops
    return tuple(ops.md5_planes([torch.as_tensor(fr[c]).to(device).contiguous() for fr in frames]) for c in 'yuv')


def probe_unit0(frame_codec, path, plan, device, contract):
    """decode the first intra-period unit, as a video of that one unit, under `contract` -> how many of its sections did not
    decode to where their payload ends (the trial decode of `--contract auto`, aivc_amd/digests.py: choose_contract); the
    precision is put back.  The unit's record is the plan's, or read through the index where the request does not touch it."""
    from .. import ops
    from . import cat_binary_files as container
    video = plan.video
    unit0 = video.gops[0]
    if unit0 is None:
        with open(path, 'rb') as f:
            unit0 = container.read_units(f, container.index_video(f, upto=0)[3], [0])[0]
    prev = ops.set_precision(contract)
    try:
        with torch.no_grad():
            frame_codec.decode_video(video._replace(names=video.names[:1], gops=[unit0]), device)
        torch.cuda.synchronize()
        return len(frame_codec.stream_errors())
    finally:
        ops.set_precision(prev)


def decode_one_video(param):
    """verify: '' (off), the path of a manifest (aivc_amd/digests.py), or True for '<bitstream>.md5': the decoded planes are
    digested on the device and compared with the manifest's; one `[VERIFY] <n> frames, <k> planes differ` line and the first
    eight differing '<idx>_<c>' names are printed, the frames are written regardless, verify_mismatch_count() says how many.
    contract: '' (whatever the process runs in), a name of aivc_amd.ops.set_precision, or 'auto': the manifest's when there is
    one (verification is then implied), else a trial decode of unit 0 (aivc_amd/digests.py: choose_contract).  The
    precision of the process is put back before this returns.
    frames: (a, b), absolute display indices, either end None for the stream's; max_level: a temporal level (the dependency
    depth of a frame in its unit).  With either, this is a partial decode: the index of the file is walked only as far as the
    request reaches and only the units it touches are read (what lies behind the last of them may be missing), only the
    reference closure of the request is decoded, and the frames asked for are written in ascending order (pictures
    under their absolute index), counted by `Number of frames` and compared with their rows of the manifest.  One line more
    is printed: `[INFO] partial decode: <K> frames written, <D> of <C> coded frames decoded`.  A request outside the stream
    is an aivc_amd.partial.FrameSelectionError.  Without either it is the same decode with the request for everything.
    out_size: None (the default), or (w, h): the frames that are returned and written -- the .yuv file or the pictures -- are
    resized to it on the device just before (func_util.img_processing.resize_frames: Pillow's Image.resize byte for byte,
    filter `resample`, default bicubic; each plane on its own, chroma to the ceil half size, chroma siting ignored).  The
    stream has no display-size field, so the size is the caller's to give, and so is a .yuv file name that states it.
    Verification and flag_bitstream_debug look at the planes at CODED size, before the resize; a partial decode resizes only
    the frames it returns.
    out_pix_fmt: the layout of the file that is written, a 4:2:0 or grey name of aivc_amd.rawvideo.PIX_FMTS (default yuv420p);
    an out_file that ends in .y4m gets a header and `FRAME` lines, fps: its frame rate (numerator, denominator) -- the stream
    stores none, default (25, 1).  The export runs on the device after the resize (aivc_amd.rawvideo.write_raw, for every file:
    yuv420p into a headerless file is the planes one after the other); the frames that are returned, verified and digested stay
    the 8-bit planes.
    png_coder: 'pillow' (the default) or 'device', who codes the pictures of a folder (write_png_folder); 'device' with an
    out_file that names a raw video file is a ValueError.
    colour: None (the default) -- the pictures of a folder are Pillow's YCbCr -> RGB of the planes (BT.601, full range); an
    aivc_amd.color.ColourSpec -- the planes carry that matrix and range and the pictures are converted by it, in integers on the
    device (aivc_amd/color.py), after the resize; one `[INFO] colour:` line is printed.  The stream stores no colour description,
    so this is the caller's to say, as the encoder was told.  Verification keeps digesting the coded planes.  An out_file that
    names a raw video file is a ValueError: nothing is converted there."""
    default = {'decoder': None, 'bitstream_path': '', 'device': 'cuda:0', 'out_file': '', 'flag_bitstream_debug': False,
               'verify': '', 'contract': '', 'frames': None, 'max_level': None, **SINK._asdict()}
    decoder = get_value('decoder', param, default).eval()
    path = get_value('bitstream_path', param, default)
    dev = torch.device(get_value('device', param, default))
    out_file = get_value('out_file', param, default)
    verify = get_value('verify', param, default)
    contract = get_value('contract', param, default)
    print_log_msg('INFO', 'Bitstream path', '', path)
    plan = read_plan(path, get_value('frames', param, default), get_value('max_level', param, default))
    from .. import digests, ops, parallel
    _VERIFY_BAD[0] = 0
    sink = Sink.from_param(param)
    sink.check(out_file, odd_pictures=True)
    manifest = None
    manifest_file = verify if isinstance(verify, str) and verify else digests.manifest_path(path)
    if verify or (contract == 'auto' and os.path.exists(manifest_file)):
        manifest = digests.read_manifest(manifest_file)
    prev_precision = ops.precision_name()
    try:
        if contract == 'auto':
            fc0 = FrameCodec(decoder.full_net)
            choice, _, note = digests.choose_contract(None if manifest is None else manifest.contract, prev_precision,
                                                      lambda name: probe_unit0(fc0, path, plan, dev, name), parallel.rank_world()[1])
            if note and parallel.rank_world()[0] == 0:
                print(note)
            ops.set_precision(choice)
        elif contract:
            ops.set_precision(contract)
        return _decode_one_video(decoder, path, plan, dev, out_file, manifest, get_value('flag_bitstream_debug', param, default), sink)
    finally:
        ops.set_precision(prev_precision)


def read_plan(path, span, max_level):
    """the file of a decode -> its aivc_amd.partial.Plan, the video holding the records of the units that are decoded: the
    index is walked as far as the request reaches (span: (a, b) or None; all of it for a whole decode), and of the payload
    only those units are read"""
    from .. import partial
    from . import cat_binary_files as container
    with open(path, 'rb') as f:
        data_dim, first, last, units = container.index_video(f, upto_frame=None if span is None else span[1])
        video = partial.IndexedVideo(data_dim, first, last, [u[2] for u in units], [None] * len(units))
        plan = partial.plan(video, None if span is None else partial.frame_range(span, first, last), max_level)
        gops = container.read_units(f, units, [u for u, need in enumerate(plan.need) if need])
    return plan._replace(video=video._replace(gops=gops))


def _decode_one_video(decoder, path, plan, dev, out_file, manifest, flag_bitstream_debug, sink):
    print_log_msg('INFO', 'Start decoding', '', '')
    t0 = time.time()
    from .. import parallel, partial
    rank, world = parallel.rank_world()
    fc = FrameCodec(decoder.full_net)
    video, first = plan.video, plan.video.first
    with torch.no_grad():
        if world > 1:  # one process per GPU: every rank decodes its intra-period units, rank 0 collects the planes
            frames = parallel.decode_video_sharded(fc, video, dev, plan=plan)
        else:
            frames = fc.decode_video(video, dev, plan=plan)[0]
    torch.cuda.synchronize()
    dt = time.time() - t0
    errs = report_stream_errors(fc, path)  # (every rank reports the sections IT decoded)
    _JOB_ERRORS[0] = len(errs)
    if world > 1:  # ... and the job's total reaches every rank: the exit status of rank 0 speaks for all of them
        import torch.distributed as dist
        cnt = torch.tensor([len(errs)], dtype=torch.int64, device=dev if dist.get_backend() == 'nccl' else 'cpu')
        dist.all_reduce(cnt)
        _JOB_ERRORS[0] = int(cnt.item())
    if rank != 0:
        dist_barrier_after_write(world)
        return None
    shown = plan.indices  # the absolute indices of the frames asked for, ascending; `frames` becomes those frames
    frames = [frames[i - first] for i in shown]
    n = len(shown)
    print_log_msg('INFO', 'Decoding done', '', '')
    if not plan.whole:
        print('[INFO] partial decode: %d frames written, %d of %d coded frames decoded'
              % (n, sum(len(c) for c in plan.need), partial.coded_frames(video.names, first, video.last)))
    print_log_msg('RESULT', 'Number of frames', '[frame]', int(n))
    print_log_msg('RESULT', 'Decoding time', '[s]', '%.1f' % dt)
    print_log_msg('RESULT', 'Decoding FPS', '[frame/s]', '%.1f' % (n / dt))
    found = None
    if manifest is not None:  # (queued now, read after the frames have been written)
        found = digest_frames(frames, dev)
    coded = frames
    if sink.out_size is not None:  # (after the digests: they are the coded planes')
        from ..func_util.img_processing import resize_frames
        frames = resize_frames(frames, int(sink.out_size[0]), int(sink.out_size[1]), sink.resample, dev)
    if is_png_folder(out_file):
        if sink.colour is not None:
            from .. import color
            print(color.info_line(sink.colour))
        write_png_folder(frames, out_file, dev, shown, sink.png_coder, sink.colour)
    elif out_file:  # (after the resize: the export sees the size that is written)
        from .. import rawvideo
        rawvideo.write_raw(frames, out_file, sink.out_pix_fmt, tuple(sink.fps), dev)
    dist_barrier_after_write(world)
    if manifest is not None:  # the frames returned against their rows of the manifest; a whole decode against all of it
        from .. import digests
        rows = dict(zip(shown, digests.hex_rows(0, [d.cpu().numpy() for d in found]).values()))
        differing = digests.compare(manifest.rows if plan.whole else digests.manifest_subset(manifest.rows, shown), rows)
        _VERIFY_BAD[0] = len(differing)
        for line in digests.verify_lines(len(rows), differing):
            print(line)
    if flag_bitstream_debug:
        for idx, fr in zip(shown, coded):
            check_debug_md5([fr], idx, debug_dir(path))
    return frames


_VERIFY_BAD = [0]  # planes of the last decode_one_video whose digest is not the manifest's (rank 0)


def verify_mismatch_count():
    return _VERIFY_BAD[0]


STREAM_ERRORS = []  # what the last decode_one_video found on THIS rank
_JOB_ERRORS = [0]   # ... and how many sections failed over all ranks of the job (the CLI's exit status)


def stream_error_count():
    return max(_JOB_ERRORS[0], len(STREAM_ERRORS))


def report_stream_errors(frame_codec, path=''):
    """A bitstream written on another implementation of the transforms (the reference on torch: its sigma differs
    from this build's in the last bits), a damaged file or the wrong model decodes WITHOUT any error from the range
    coder -- it just yields other symbols from the first differing CDF bound on.  Two detectors say so: the md5
    sections of flag_md5sum (src/real_life/bitstream.py:488-499) and, always on, the decoder's bit count against the
    section length.  Printed in the reference's style, not raised; the CLI exits non-zero."""
    errs = frame_codec.stream_errors()
    del STREAM_ERRORS[:]
    STREAM_ERRORS.extend(errs)
    if errs:
        print('-' * 80)
        print('[WARN] %d section(s) of %s did not decode to where their payload ends: the stream was NOT written with the '
              'CDFs this decoder builds (other implementation of the transforms / other model / damaged file); the '
              'frames from the first such section on are unreliable' % (len(errs), path or 'the bitstream'))
        for net, what, i, have, need in errs[:8]:
            print('\t%s %s, stream %d of its launch: payload %d bytes, decode accounts for %d' % (net, what, i, have, need))
        print('-' * 80)
    return errs


def dist_barrier_after_write(world):
    """multi-rank CLI: nobody goes on (to evaluate the output file) before rank 0 has written it"""
    if world > 1:
        import torch.distributed as dist
        dist.barrier()


def debug_dir(bitstream_path):
    """where flag_bitstream_debug keeps the encoder's per-plane digests: '<bitstream>.debug/' (the reference uses
    '<root>/debug/<sequence>/' next to its PNG folders, src/model_mngt/model_management.py:132-135)"""
    return bitstream_path + '.debug'


def plane_md5(plane, kind=None):
    """Digest flag_bitstream_debug compares per plane.  The reference hashes the PNG FILE it saved for the plane
    (save_yuv_separately -> to_pil_image(mode='L').save, src/func_util/img_processing.py:290-302; compare at
    src/real_life/decode.py:304-326): the same file is produced here in memory with PIL, so the .md5 files
    interoperate with a reference decoder / encoder running the same Pillow + zlib (the PNG byte stream depends
    on them; pinned by tests/golden/decoder_*.npz `pngmd5_*`).  kind='raw': digest of the raw 8-bit plane,
    independent of Pillow / zlib; kind=None picks 'png' when Pillow is importable."""
    import hashlib
    a = plane.cpu().numpy() if isinstance(plane, torch.Tensor) else np.asarray(plane)
    a = np.ascontiguousarray(a.reshape(a.shape[-2], a.shape[-1]))
    if kind is None:
        kind = digest_kind()
    if kind == 'raw':
        return hashlib.md5(a.tobytes()).hexdigest()
    import io
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(a, 'L').save(buf, format='PNG')
    return hashlib.md5(buf.getvalue()).hexdigest()


def digest_kind():
    try:
        import PIL  # noqa: F401
        return 'png'
    except ImportError:
        return 'raw'


def write_debug_md5(frames, first, directory):
    """encoder side of flag_bitstream_debug: '<idx>_<c>.md5' per reconstructed plane (see plane_md5).  A bare
    32-digit digest is the md5 of the PNG file, as in the reference; where Pillow is missing the file says
    'raw:<digest>' so that the decoder compares like with like whatever ITS environment."""
    os.makedirs(directory, exist_ok=True)
    kind = digest_kind()
    for i, fr in enumerate(frames):
        for c in 'yuv':
            with open(os.path.join(directory, '%d_%s.md5' % (first + i, c)), 'w') as f:
                f.write(('raw:' if kind == 'raw' else '') + plane_md5(fr[c], kind))


def check_debug_md5(frames, first, directory):
    """decoder side: same messages as src/real_life/decode.py:318-326; -> number of mismatching planes"""
    bad = 0
    for i, fr in enumerate(frames):
        for c in 'yuv':
            name = '%d_%s' % (first + i, c)
            with open(os.path.join(directory, name + '.md5')) as f:
                encoder_md5 = f.read().strip()
            msg = name + ': '
            kind = 'png'
            if encoder_md5.startswith('raw:'):
                kind, encoder_md5 = 'raw', encoder_md5[4:]
            if encoder_md5 != plane_md5(fr[c], kind):  # (a 'png' digest without Pillow here raises: no silent fallback)
                bad += 1
                msg += '\n' + '-' * 80 + '\n' + 'Incorrect reconstruction!\n' + '-' * 80 + '\n'
            else:
                msg += 'Identical reconstruction!'
            print(msg)
        print('')
    return bad
