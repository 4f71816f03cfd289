#!/usr/bin/env python3
"""encode.py CLI (flags of src/encode.py:27-66).  python -m aivc_amd.encode -i clip_WxH_fps_420.yuv ...
-i may also name a .y4m file, a headerless file in another layout (--pix_fmt, or _422 / _444 / _10b ... tokens in its name), or a folder of the reference's pictures: PNG triplets (<idx>_{y,u,v}.png, or the CLIC layout) or <idx>.png RGB.
RGB pictures become planes by Pillow's arithmetic (BT.601, full range) unless --matrix / --range say what the planes are to carry."""
import argparse

from aivc_amd.cli_common import add_contract_flag, contract_scope, get_model, resolve_device
from aivc_amd.func_util.GOP_structure import generate_gop_struct
from aivc_amd.real_life.encode import encode


def add_rate_flags(p):
    """--idx_rate / --target_bpp / --rate_step (shared with aivc.py)"""
    p.add_argument('--idx_rate', default=None, type=float,
                   help='rate index of the whole clip: a multiple of 1/16 in [0, rate indices of the model - 1]; default 0')
    p.add_argument('--target_bpp', default=0., type=float,
                   help='bit per pixel: every intra-period unit is coded at the richest rate index whose GOP record fits '
                        'target_bpp x w x h x frames / 8 bytes (a few bitstream-only encodes per unit); 0: off')
    p.add_argument('--rate_step', default=0.0625, type=float, help='grid step of the --target_bpp search (a multiple of 1/16)')


def check_rate_flags(p, a):
    """-> the idx_rate to encode with; an argparse error for --idx_rate together with --target_bpp or off the 1/16 grid"""
    from aivc_amd import rate_control
    if a.target_bpp < 0:
        p.error('--target_bpp must be positive (0: off)')
    if a.idx_rate is not None and a.target_bpp > 0:
        p.error('--idx_rate and --target_bpp are mutually exclusive: a byte budget chooses the rate index itself')
    if a.idx_rate is not None and (a.idx_rate < 0 or not rate_control.on_sixteenths(a.idx_rate)):
        p.error('--idx_rate %r: expected a non-negative multiple of 1/16 (the GOP header stores sixteenths)' % a.idx_rate)
    if a.rate_step <= 0 or not rate_control.on_sixteenths(a.rate_step):
        p.error('--rate_step %r: expected a positive multiple of 1/16' % a.rate_step)
    return 0 if a.idx_rate is None else a.idx_rate


def add_scene_flag(p):
    """--scene_cut [T] (shared with aivc.py)"""
    p.add_argument('--scene_cut', nargs='?', const=10.0, default=None, type=float, metavar='T',
                   help='detect scene cuts on the device and open a new intra-period unit at each: a frame whose mean absolute '
                        'luma difference to its predecessor stands out over both neighbouring differences by at least T grey '
                        'levels (default 10, a convention that has not been measured on real material); the units in front of a '
                        'cut take a shorter coding structure, any decoder of the format reads the stream; off by default')


def check_scene_flag(p, a):
    if a.scene_cut is not None and not a.scene_cut >= 0:
        p.error('--scene_cut %r: the threshold is a non-negative number of grey levels' % a.scene_cut)


SIZE_HELP = ('code the clip at this size: every plane is resized on the device right after it has been read (y to H x W, u and v to '
             'the ceil half size, each on its own; RGB pictures are converted to 4:2:0 first); header, scene cuts, digests, the '
             'byte budget of --target_bpp and the --log_dir table (which scores against the RESIZED source) see the coded size.  '
             'The stream has no display-size field: decode.py --out_size writes another size')


def add_size_flag(p):
    """--size WxH and --resample (aivc.py adds --out_size to the same call)"""
    from aivc_amd.resize import add_resize_flags
    add_resize_flags(p, {'--size': SIZE_HELP})


def add_pix_fmt_flag(p):
    """--pix_fmt NAME (shared with aivc.py)"""
    from aivc_amd.rawvideo import PIX_FMTS
    p.add_argument('--pix_fmt', default=None, choices=PIX_FMTS, metavar='NAME',
                   help='layout of a headerless -i file, under ffmpeg\'s names (%s); unset: the _420 / _422 / _444 and _10b / _12b / '
                        '_16b / _<n>bit tokens of its name, default yuv420p.  A .y4m file says what it holds.  Anything but planar '
                        '8-bit 4:2:0 is converted to it on the device before everything else (--size included): what is coded, '
                        'digested and scored by --log_dir are the converted planes' % ', '.join(PIX_FMTS))


def add_png_reader_flag(p):
    """--png_reader {pillow,device} (shared with aivc.py)"""
    from aivc_amd.png import READERS
    p.add_argument('--png_reader', default='pillow', choices=READERS,
                   help='who reads the pictures of a folder given as -i: pillow (one Image.open per picture on the host, the default) or '
                        'device (8-bit grey and RGB pictures are inflated and unfiltered on the device, all pictures of the clip at '
                        'once; any other PNG still goes through Pillow); the same planes and the same bitstream either way')


def check_png_reader(p, a):
    """an argparse error for --png_reader device where -i is not a picture folder"""
    import os
    from aivc_amd import png
    try:
        png.check_reader(a.png_reader, a.i, os.path.isdir(a.i))
    except ValueError as e:
        p.error(str(e))


def check_input_range(a):
    """a raw video file as -i: exit status 2 with the file's range for --start_frame / --end_frame outside it, before a device is
    looked for (like a partial decode's request outside the stream)"""
    import os
    from aivc_amd import rawvideo
    if not os.path.isfile(a.i):
        return
    try:
        with rawvideo.open_raw(a.i, a.pix_fmt) as reader:
            reader.frame_range(a.start_frame, a.end_frame)
    except rawvideo.RawVideoError as e:
        print('[ERROR] %s: %s' % (a.i, e))
        raise SystemExit(2)


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--gop', default='1_GOP_32', type=str)
    p.add_argument('--model', default='ms_ssim-2021cc-6', type=str)
    p.add_argument('-i', default='../raw_videos/BQMall_832x480_60_420.yuv', type=str)
    p.add_argument('-o', default='../bitstream.bin', type=str)
    p.add_argument('--start_frame', default=0, type=int)
    p.add_argument('--end_frame', default=-1, type=int)
    p.add_argument('--rng_seed', default=666, type=int)
    p.add_argument('--cpu', action='store_true')
    p.add_argument('--log_dir', default='', type=str,
                   help='write the per-frame table <log_dir>/detailed.txt (PSNR, rates, alpha, beta, loss, MS-SSIM) and print '
                        'the Estimated MS-SSIM line; off by default.  With --size the scores are against the resized source')
    p.add_argument('--digests', action='store_true',
                   help='write the sidecar manifest <bitstream>.md5: the arithmetic contract and one MD5 per reconstructed plane, '
                        'computed on the device (decode.py --verify checks a decode against it); the bitstream does not change')
    add_pix_fmt_flag(p)
    add_png_reader_flag(p)
    from aivc_amd.color import add_colour_flags, check_colour_flags
    add_colour_flags(p, decoder=False)
    add_contract_flag(p, ('fp32', 'fp32w'))
    add_rate_flags(p)
    add_scene_flag(p)
    add_size_flag(p)
    a = p.parse_args(argv)
    a.idx_rate = check_rate_flags(p, a)
    check_scene_flag(p, a)
    check_png_reader(p, a)
    check_colour_flags(p, a, in_path=a.i)
    from aivc_amd.resize import check_resize_flags
    a.resample = check_resize_flags(p, a, ('--size',))
    return a


def main(argv=None):
    a = parse_args(argv)
    check_input_range(a)
    dev = resolve_device(a.cpu)
    model = get_model(a.model, dev)
    nb_rates = len(model.codec_net.codec_net.gain_I.enc_gain_list) if a.idx_rate else 1
    if a.idx_rate > nb_rates - 1:
        raise SystemExit('[ERROR] --idx_rate %s: model %s has %d rate indices (0 ... %d)' % (a.idx_rate, a.model, nb_rates, nb_rates - 1))
    with contract_scope(a.contract):
        return encode({'model': model, 'sequence_path': a.i, 'GOP_struct': generate_gop_struct(a.gop),
                       'GOP_struct_name': a.gop, 'idx_rate': a.idx_rate, 'final_file': a.o, 'idx_starting_frame': a.start_frame,
                       'idx_end_frame': a.end_frame, 'working_dir': a.log_dir, 'target_bpp': a.target_bpp,
                       'rate_step': a.rate_step, 'digests': a.digests, 'scene_cut': a.scene_cut, 'size': a.size,
                       'resample': a.resample, 'pix_fmt': a.pix_fmt, 'png_reader': a.png_reader, 'colour': a.colour,
                       'chroma_down': a.chroma_down})


if __name__ == '__main__':
    main()
