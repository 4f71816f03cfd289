#!/usr/bin/env python3
"""aivc.py CLI (flags of src/aivc.py:16-76): encode, decode, evaluate (PSNR, MS-SSIM, size) -- in one process
(the reference forks three python processes and goes through PNG triplets)."""
import argparse
import os
import sys

from aivc_amd import decode as dec_cli
from aivc_amd import encode as enc_cli
from aivc_amd import evaluate as eval_cli


def gop_name(cfg, gop_size, intra_period):
    """src/aivc.py:80-107"""
    if cfg == 'AI':
        return '1_GOP_0'
    if cfg == 'LDP':
        if intra_period not in range(2, 65535):
            sys.exit('[ERROR]: Intra period should be in [2, 65535] for LDP.')
        return 'LDP_%d' % intra_period
    if cfg == 'RA':
        if intra_period % gop_size:
            sys.exit('[ERROR]: Intra period must be equal a multiple of GOP size')
        return '%d_GOP_%d' % (intra_period // gop_size, gop_size)
    sys.exit('[ERROR]: unknown coding configuration. Should be either RA, AI or LDP.')


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--coding_config', default='RA', type=str)
    p.add_argument('--gop_size', default=32, type=int)
    p.add_argument('--intra_period', default=32, type=int)
    p.add_argument('--model', default='ms_ssim-2021cc-3', type=str)
    p.add_argument('-i', default='../raw_videos/BlowingBubbles_416x240_50_420.yuv', type=str)
    p.add_argument('--start_frame', default=0, type=int)
    p.add_argument('--end_frame', default=90, type=int)
    p.add_argument('--bitstream_out', default='../bitstream.bin', type=str)
    p.add_argument('-o', default='../compressed.yuv', type=str)
    p.add_argument('--rng_seed', default=666, type=int)
    p.add_argument('--cpu', action='store_true')
    p.add_argument('--log_dir', default='', type=str, help="the encoder's per-frame table goes to <log_dir>/detailed.txt (encode.py)")
    p.add_argument('--digests', action='store_true',
                   help='the encoder writes the manifest <bitstream_out>.md5 (encode.py --digests) and the decode is verified against it')
    dec_cli.add_verify_flag(p)
    from aivc_amd.cli_common import add_contract_flag
    add_contract_flag(p, ('fp32', 'fp32w', 'auto'))
    enc_cli.add_rate_flags(p)
    enc_cli.add_scene_flag(p)
    enc_cli.add_pix_fmt_flag(p)
    enc_cli.add_png_reader_flag(p)
    dec_cli.add_out_format_flags(p)
    dec_cli.add_png_coder_flag(p)
    from aivc_amd.color import add_colour_flags, check_colour_flags
    add_colour_flags(p)
    from aivc_amd.resize import add_resize_flags, check_resize_flags
    add_resize_flags(p, {'--size': enc_cli.SIZE_HELP, '--out_size': dec_cli.OUT_SIZE_HELP})
    a = p.parse_args(argv)
    enc_cli.check_rate_flags(p, a)
    enc_cli.check_scene_flag(p, a)
    enc_cli.check_png_reader(p, a)
    a.resample = check_resize_flags(p, a, ('--size', '--out_size'))
    dec_cli.check_out_size(p, a, a.o)
    dec_cli.check_out_format(p, a, a.o)
    dec_cli.check_png_coder(p, a, a.o)
    check_colour_flags(p, a, in_path=a.i, out_path=a.o, out_is_folder=dec_cli.is_png_folder(a.o))  # (both halves are told)
    return a


def input_size(path, pix_fmt=None):
    """(w, h) of the frames in -i: a .y4m header's, else the name's"""
    from aivc_amd import rawvideo
    with rawvideo.open_raw(path, pix_fmt) as reader:
        return reader.w, reader.h


def size_text(size):
    return '%dx%d' % size


def main(argv=None):
    a = parse_args(argv)
    gop = gop_name(a.coding_config, a.gop_size, a.intra_period)
    common = ['--model', a.model] + (['--cpu'] if a.cpu else [])
    colour = ['--matrix', a.colour.matrix, '--range', a.colour.range] if a.colour is not None else []
    import os
    banner = print if int(os.environ.get('RANK', '0')) == 0 else (lambda *x: None)  # one voice in a multi-rank job
    banner(('*' * 80).center(120))
    banner('Starting encoding'.center(120))
    enc_cli.main(['-i', a.i, '--gop', gop, '--start_frame', str(a.start_frame), '--end_frame', str(a.end_frame),
                  '-o', a.bitstream_out, '--rate_step', str(a.rate_step)] + common
                 + (['--log_dir', a.log_dir] if a.log_dir else [])
                 + (['--idx_rate', str(a.idx_rate)] if a.idx_rate is not None else [])
                 + (['--target_bpp', str(a.target_bpp)] if a.target_bpp > 0 else [])
                 + (['--digests'] if a.digests else [])
                 + (['--scene_cut', repr(a.scene_cut)] if a.scene_cut is not None else [])
                 + (['--pix_fmt', a.pix_fmt] if a.pix_fmt is not None else [])
                 + (['--png_reader', a.png_reader] if a.png_reader != 'pillow' else [])
                 + colour + (['--chroma_down', a.chroma_down] if a.chroma_down != 'point' else [])
                 + (['--size', size_text(a.size), '--resample', a.resample] if a.size is not None else [])
                 + (['--contract', a.contract] if a.contract not in (None, 'auto') else []))  # (auto is the decoder's choice)
    banner(('*' * 80).center(120))
    banner('Starting decoding'.center(120))
    verify = a.verify if a.verify else bool(a.digests)  # --digests verifies its own decode
    status = dec_cli.main(['-i', a.bitstream_out, '-o', a.o] + common
                          + ([] if not verify else ['--verify'] if verify is True else ['--verify', verify])
                          + (['--out_size', size_text(a.out_size), '--resample', a.resample] if a.out_size is not None else [])
                          + (['--out_pix_fmt', a.out_pix_fmt] if a.out_pix_fmt != 'yuv420p' else [])
                          + (['--fps', '%d:%d' % a.fps] if a.fps != (25, 1) else [])
                          + (['--png_coder', a.png_coder] if a.png_coder != 'pillow' else []) + colour
                          + (['--contract', a.contract] if a.contract else []))
    from aivc_amd import parallel
    if parallel.rank_world()[0] != 0:  # multi-rank job: rank 0 evaluates
        return status
    if os.path.isdir(a.i) or dec_cli.is_png_folder(a.o):  # (evaluate.py scores planar files)
        print('[INFO] evaluation skipped: it compares two planar .yuv files, -i / -o name picture folders')
        return status
    written = a.out_size if a.out_size is not None else a.size  # the size of the frames in -o, where it was chosen here
    source = written and input_size(a.i, a.pix_fmt)  # (-i is looked at only where a size was chosen)
    if written != source:
        print('[INFO] evaluation skipped: -o holds %dx%d frames, -i %dx%d ones (evaluate.py compares frames of one size; '
              '--out_size with the size of -i brings them back)' % (written + source))
        return status
    print(('*' * 80).center(120))
    print('Starting evaluation'.center(120))
    eval_cli.main(['--raw', a.i, '--compressed', a.o, '--bitstream', a.bitstream_out, '--start_frame', str(a.start_frame)]
                  + (['--pix_fmt', a.pix_fmt] if a.pix_fmt is not None else [])
                  + (['--compressed_pix_fmt', a.out_pix_fmt] if a.out_pix_fmt != 'yuv420p' and not a.o.endswith('.y4m') else []))
    return status  # 3: decoded and evaluated, but the stream did not decode cleanly (real_life/decode.py)


def cli():
    raise SystemExit(main())


if __name__ == '__main__':
    cli()
