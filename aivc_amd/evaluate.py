#!/usr/bin/env python3
"""evaluate.py CLI (src/evaluate.py): the CLIC-2021 figures of a decoded video and the size of its bitstream --

    PSNR    [dB]: ...      MS-SSIM     : ...      MS-SSIM [dB]: ...      Size [bytes]: ...

The reference walks two folders of <idx>_{y,u,v}.png planes; here --raw / --compressed are raw video files (what encode.py
reads and decode.py writes -- no PNG round trip), read by the one reader, aivc_amd.rawvideo.open_raw: planar 8-bit 4:2:0 .yuv
files, .y4m, other layouts by --pix_fmt / --compressed_pix_fmt or the tokens of the name, which are converted to 8-bit 4:2:0 on
the device first -- a 10-bit source is scored as the encoder saw it.  The three planes of every decoded frame are scored on the
GPU (aivc_amd/clic21/metrics.py)."""
import argparse
import os

from aivc_amd.clic21.metrics import evaluate


def _host_planes(reader, first=0, count=None):
    """an opened aivc_amd.rawvideo reader -> the host planes [{'y', 'u', 'v'}] of its frames from `first` on, at most `count`"""
    n = reader.n_frames - first if count is None else min(reader.n_frames - first, count)
    frames = reader.read(first, first + n - 1) if n > 0 else []
    return [{k: fr[k][0].cpu().numpy() for k in 'yuv'} for fr in frames]


def evaluate_yuv(raw_path, compressed_path, start_frame=0, pix_fmt=None, compressed_pix_fmt=None):
    """frame size from the raw file: its .y4m header, or its name (<Name>_<W>x<H>_..., as encode.py parses it); a headerless
    compressed file has the raw file's size"""
    from aivc_amd import rawvideo
    with rawvideo.open_raw(raw_path, pix_fmt) as src:
        w, h = src.w, src.h
        with rawvideo.open_raw(compressed_path, compressed_pix_fmt, None if compressed_path.endswith('.y4m') else (w, h)) as out:
            if (out.w, out.h) != (w, h):
                raise ValueError('%s holds %dx%d frames, %s %dx%d ones' % (compressed_path, out.w, out.h, raw_path, w, h))
            dec = _host_planes(out)
        raw = _host_planes(src, start_frame, len(dec))
    target, submit = {}, {}
    for idx, (r, d) in enumerate(zip(raw, dec)):
        for c in 'yuv':
            target['%d_%s' % (idx, c)] = r[c]
            submit['%d_%s' % (idx, c)] = d[c]
    return evaluate(submit, target)


def main(argv=None):
    p = argparse.ArgumentParser()
    from aivc_amd.rawvideo import PIX_FMTS
    p.add_argument('--raw', default='', type=str, help='raw video file with the input frames: planar 4:2:0 .yuv, .y4m, or --pix_fmt')
    p.add_argument('--compressed', default='', type=str, help='raw video file written by decode.py (.yuv or .y4m)')
    p.add_argument('--pix_fmt', default=None, choices=PIX_FMTS, metavar='NAME', help='layout of a headerless --raw (encode.py --pix_fmt)')
    p.add_argument('--compressed_pix_fmt', default=None, choices=PIX_FMTS, metavar='NAME',
                   help='layout of a headerless --compressed (decode.py --out_pix_fmt)')
    p.add_argument('--bitstream', default='../bitstream.bin', type=str, help='Path of the bitstream')
    p.add_argument('--start_frame', default=0, type=int, help='index of the first coded frame inside --raw')
    a = p.parse_args(argv)
    comp = a.compressed if a.compressed.endswith(('.yuv', '.y4m')) else a.compressed + '.yuv'
    results = evaluate_yuv(a.raw, comp, a.start_frame, a.pix_fmt, a.compressed_pix_fmt)
    print('PSNR    [dB]: ' + '%.5f' % (results.get('PSNR')))
    print('MS-SSIM     : ' + '%.5f' % (results.get('MSSSIM')))
    print('MS-SSIM [dB]: ' + '%.5f' % (results.get('MSSSIM_dB')))
    try:
        print('Size [bytes]: ' + '%.0f' % os.path.getsize(a.bitstream))
    except FileNotFoundError:
        print('[ERROR]: bitstream not found, can not evaluate its size!')
        print('Bistream path: ' + a.bitstream)
    return results


if __name__ == '__main__':
    main()
