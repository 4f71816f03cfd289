#!/usr/bin/env python3
"""The colour conversion by matrix and range (aivc_amd.color.rgb_to_yuv420 / yuv_to_rgb) on 33 frames of 1080p, each beside the
table kernels of Pillow's arithmetic (ops.rgb8_to_yuv420u8 / ops.yuv8_to_rgb8) on the same frames and beside a device-to-device
copy that moves the same number of bytes (read + written): HIP events around every launch (ops.PROFILE_HBM; the copy between two
events of its own), the paths taken in turn within each of `repeats` runs after one warm-up run, medians.  The outputs are
compared with the numpy statement on the first and the last frame.
Also, on the host: the share of the 2^24 RGB triples on which bt601 full differs from Pillow's arithmetic, per component, in
both directions.  experiments/colour.md.
usage: tools/bench_colour.py [out.json] [frames] [repeats]"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from aivc_amd import color, ops  # noqa: E402

H, W = 1080, 1920


def med(v):
    return sorted(v)[len(v) // 2]


def pillow_differences():
    """bt601 full against Image.convert on every triple -> {direction: {component: share that differs, 'max': largest difference}}"""
    from PIL import Image
    i, j = np.meshgrid(np.arange(4096), np.arange(4096), indexing='ij')
    img = np.stack([i >> 4, ((i & 15) << 4) | (j >> 8), j & 255], axis=-1).astype(np.uint8)
    spec = ('bt601', 'full')
    out = {}
    for name, mode_in, mode_out, fn, comps in (('rgb_to_ycbcr', 'RGB', 'YCbCr', color.forward_pixels, ('Y', 'Cb', 'Cr')),
                                               ('ycbcr_to_rgb', 'YCbCr', 'RGB', color.inverse_pixels, 'RGB')):
        pil = np.asarray(Image.fromarray(img, mode_in).convert(mode_out)).astype(np.int16)
        d = np.abs(fn(img, spec).astype(np.int16) - pil)
        out[name] = dict({c: round(float((d[..., k] != 0).mean()), 6) for k, c in enumerate(comps)},
                         any=round(float((d != 0).any(axis=-1).mean()), 6), max=int(d.max()))
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 33
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device('cuda:0')
    spec = color.ColourSpec('bt709', 'limited')
    rng = np.random.default_rng(0)
    host = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    rgb = torch.from_numpy(host).to(dev)
    y, u, v = ops.rgb8_to_yuv420u8(rgb)
    nbytes = n * (H * W * 4 + 2 * (H // 2) * (W // 2))  # read + written, either direction
    src = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
    dst = torch.empty_like(src)
    paths = {
        'rgb8_to_yuv420u8': lambda: ops.rgb8_to_yuv420u8(rgb),
        'rgb8_to_yuv420u8_matrix': lambda: color.rgb_to_yuv420(rgb, spec, 'point'),
        'rgb8_to_yuv420u8_matrix box': lambda: color.rgb_to_yuv420(rgb, spec, 'box'),
        'yuv8_to_rgb8': lambda: ops.yuv8_to_rgb8(y, u, v),
        'yuv8_to_rgb8_matrix': lambda: color.yuv_to_rgb(y, u, v, spec),
    }
    ms = {k: [] for k in list(paths) + ['copy of the same bytes']}
    for r in range(repeats + 1):
        for name, fn in paths.items():
            ops.PROFILE_HBM = []
            fn()
            torch.cuda.synchronize()
            prof, ops.PROFILE_HBM = ops.PROFILE_HBM, None
            assert len(prof) == 1 and prof[0][1] == nbytes, (name, prof)
            if r:
                ms[name].append(prof[0][2].elapsed_time(prof[0][3]))
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        dst.copy_(src)
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms['copy of the same bytes'].append(e0.elapsed_time(e1))
    res = {'frames': n, 'size': '%dx%d' % (W, H), 'repeats': repeats, 'bytes_moved': nbytes,
           'ms': {k: [round(x, 4) for x in t] for k, t in ms.items()},
           'ms_median': {k: round(med(t), 4) for k, t in ms.items()},
           'TB_per_s_median': {k: round(nbytes / med(t) / 1e9, 3) for k, t in ms.items()}}
    # the outputs at this size against the statement, first and last frame
    pick = [0, n - 1]
    same = {}
    for down in ('point', 'box'):
        got = [t[pick].cpu().numpy() for t in color.rgb_to_yuv420(rgb, spec, down)]
        same['forward ' + down] = all(np.array_equal(a, b) for a, b in zip(got, color.forward_numpy(host[pick], spec, down)))
    planes = [t[pick].cpu().numpy() for t in (y, u, v)]
    same['inverse'] = bool(np.array_equal(color.yuv_to_rgb(y, u, v, spec)[pick].cpu().numpy(), color.inverse_numpy(*planes, spec)))
    res['equals_numpy_statement'] = same
    print(json.dumps(res), flush=True)
    res['bt601_full_against_pillow'] = pillow_differences()
    print(json.dumps(res['bt601_full_against_pillow']), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
