#!/usr/bin/env python3
"""decode.py CLI (flags of src/decode.py:24-40).  -o dir/ writes RGB pictures: Pillow's YCbCr -> RGB (BT.601, full range) unless
--matrix / --range say what the planes carry; the stream stores no colour description."""
import argparse

from aivc_amd.cli_common import add_contract_flag, contract_scope, get_model, resolve_device
from aivc_amd.real_life.decode import Decoder, decode_one_video, is_png_folder


OUT_SIZE_HELP = ('write the decoded frames at this size: resized on the device just before they are written, .yuv or pictures (y to '
                 'H x W, u and v to the ceil half size); --verify keeps digesting the planes at coded size, --frames / --max_level '
                 'resize only what they write.  The name of a .yuv output is the caller\'s business')


def check_out_size(p, a, out):
    """an argparse error for an odd --out_size with RGB pictures as output: their chroma would not be the ceil-sized planes the
    encoder takes back (real_life.encode.read_png_folder refuses such a folder)"""
    from aivc_amd.real_life.decode import is_png_folder
    if a.out_size is not None and is_png_folder(out) and (a.out_size[0] % 2 or a.out_size[1] % 2):
        p.error('--out_size %dx%d with RGB pictures as output (-o %s): RGB pictures need even sides' % (a.out_size + (out,)))


def add_out_format_flags(p):
    """--out_pix_fmt NAME and --fps N[:D] (shared with aivc.py)"""
    from aivc_amd.rawvideo import PIX_FMTS, PixFmt
    names = [n for n in PIX_FMTS if PixFmt(n).writable]
    p.add_argument('--out_pix_fmt', default='yuv420p', choices=names, metavar='NAME',
                   help='layout of the file that is written (%s; 4:2:0 and grey layouts only): exported on the device, after '
                        '--out_size.  -o out.y4m writes a .y4m file (planar and grey layouts)' % ', '.join(names))
    p.add_argument('--fps', default='25:1', type=str, metavar='N[:D]',
                   help='frame rate in the header of a .y4m output (default 25:1): the stream stores no frame rate')


def check_out_format(p, a, out):
    """a.fps becomes (N, D); an argparse error for a bad rate or a layout a .y4m -o has no tag for"""
    from aivc_amd import rawvideo
    try:
        a.fps = rawvideo.parse_fps(a.fps)
        rawvideo.check_writable(a.out_pix_fmt, '' if is_png_folder(out) else out)
    except ValueError as e:
        p.error(str(e))


def add_png_coder_flag(p):
    """--png_coder {pillow,device} (shared with aivc.py)"""
    from aivc_amd.png import CODERS
    p.add_argument('--png_coder', default='pillow', choices=CODERS,
                   help='who codes the <idx>.png pictures of a folder given as -o: pillow (one Image.save per frame on the host, the '
                        'default) or device (row filters and a Huffman deflate on the GPU: the same pixels, other bytes)')


def check_png_coder(p, a, out):
    """an argparse error for --png_coder device where -o is not a picture folder"""
    from aivc_amd import png
    try:
        png.check_coder(a.png_coder, out, is_png_folder(out))
    except ValueError as e:
        p.error(str(e))


def parse_args(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument('--cpu', action='store_true')
    p.add_argument('-i', default='../bitstream.bin', type=str)
    p.add_argument('-o', default='../compressed.yuv', type=str)
    p.add_argument('--model', default='ms_ssim-2021cc-6', type=str)
    p.add_argument('--rng_seed', default=666, type=int)
    add_verify_flag(p)
    add_contract_flag(p, ('fp32', 'fp32w', 'auto'))
    p.add_argument('--frames', default=None, type=frames_arg, metavar='A:B',
                   help='partial decode: only the frames A ... B (inclusive, absolute display indices as in the manifest and the '
                        'picture names; also A:, :B or A) are written; only their references are decoded and only their units read')
    p.add_argument('--max_level', default=None, type=int, metavar='L',
                   help='partial decode: only frames of temporal level <= L (the dependency depth inside an intra-period unit: '
                        '0 the I frame, 1 the P frame; 1_GOP_32 has levels 0 ... 6, each one less halves the frame count)')
    add_out_format_flags(p)
    add_png_coder_flag(p)
    from aivc_amd.color import add_colour_flags, check_colour_flags
    add_colour_flags(p, encoder=False)
    from aivc_amd.resize import add_resize_flags, check_resize_flags
    add_resize_flags(p, {'--out_size': OUT_SIZE_HELP})
    a = p.parse_args(argv)
    check_out_format(p, a, a.o)
    check_png_coder(p, a, a.o)
    check_colour_flags(p, a, out_path=a.o, out_is_folder=is_png_folder(a.o))
    if a.max_level is not None and a.max_level < 0:
        p.error('--max_level %d: temporal levels count from 0' % a.max_level)
    a.resample = check_resize_flags(p, a, ('--out_size',))
    check_out_size(p, a, a.o)
    return a


def frames_arg(text):
    from aivc_amd.partial import parse_frames_arg
    try:
        return parse_frames_arg(text)
    except ValueError as e:
        raise argparse.ArgumentTypeError(str(e))


def add_verify_flag(p):
    """--verify [MANIFEST] (shared with aivc.py): '' is off, True the manifest next to the bitstream"""
    p.add_argument('--verify', nargs='?', const=True, default='', metavar='MANIFEST',
                   help='digest the decoded planes on the device and compare them with the manifest the encoder wrote under '
                        '--digests (default: <bitstream>.md5); exit status 4 when planes differ and the stream itself decoded cleanly')


def main(argv=None):
    a = parse_args(argv)
    dev = resolve_device(a.cpu)
    out = a.o if a.o.endswith(('.yuv', '.y4m')) or is_png_folder(a.o) else a.o + '.yuv'  # ('dir/' or an existing directory: <idx>.png)
    dec = Decoder({'full_net': get_model(a.model, dev)}).eval()
    from aivc_amd.partial import FrameSelectionError
    from aivc_amd.real_life.cat_binary_files import ContainerError
    try:
        with contract_scope(a.contract):
            decode_one_video({'decoder': dec, 'bitstream_path': a.i, 'device': str(dev), 'out_file': out, 'verify': a.verify,
                              'contract': 'auto' if a.contract == 'auto' else '', 'frames': a.frames, 'max_level': a.max_level,
                              'out_size': a.out_size, 'resample': a.resample, 'out_pix_fmt': a.out_pix_fmt, 'fps': a.fps,
                              'png_coder': a.png_coder, 'colour': a.colour})
    except ContainerError as e:  # a truncated / damaged file: say so and stop (exit status 2), no frames are written
        print('[ERROR] %s is not a complete bitstream: %s' % (a.i, e))
        raise SystemExit(2)
    except FrameSelectionError as e:  # --frames / --max_level ask for nothing the stream holds: likewise
        print('[ERROR] %s: %s' % (a.i, e))
        raise SystemExit(2)
    return exit_status()


def exit_status():
    """0, or 3 when the frames were written but some section did not decode cleanly ON ANY RANK (every rank records
    the sections it decoded; the counts are summed over the job so that rank 0's status speaks for all of them), or 4 when every
    section decoded cleanly but planes differ from the manifest's digests (--verify; a stream error takes precedence)"""
    from aivc_amd.real_life.decode import stream_error_count, verify_mismatch_count
    if stream_error_count():
        return 3
    return 4 if verify_mismatch_count() else 0


def cli():
    """console-script entry point: the process exit status is main()'s"""
    raise SystemExit(main())


if __name__ == '__main__':
    cli()
