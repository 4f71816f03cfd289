#!/usr/bin/env python3
"""encode.py CLI (flags of src/encode.py:27-66).  python -m aivc_amd.encode -i clip_WxH_fps_420.yuv ...
-i may also name a .y4m file, a headerless file in another layout (--pix_fmt, or _422 / _444 / _10b ... tokens in its name), or a folder of the reference's pictures: PNG triplets (<idx>_{y,u,v}.png, or the CLIC layout) or <idx>.png RGB.
RGB pictures become planes by Pillow's arithmetic (BT.601, full range) unless --matrix / --range say what the planes are to carry."""
import argparse

from aivc_amd import options
from aivc_amd.cli_common import contract_scope, get_model, resolve_device
from aivc_amd.func_util.GOP_structure import generate_gop_struct
from aivc_amd.real_life.encode import encode


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
    return options.parse(p, argv, 'source', 'rate', 'scene', contract=('fp32', 'fp32w'))


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
                       'rate_step': a.rate_step, 'digests': a.digests, 'scene_cut': a.scene_cut, **a.source._asdict()})


if __name__ == '__main__':
    main()
