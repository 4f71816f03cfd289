#!/usr/bin/env python3
"""The device PNG coder (ops.png_encode, png.write_pictures) on 33 frames of 1080p against Pillow's Image.save on one host core:
  * device time of a batch: HIP events around the two calls of the C ABI (ops.PROFILE_HBM: png_deflate = filter + segment coder,
    png_gather), and the wall clock of ops.png_encode, which adds the two copies back and the Adler fold;
  * wall clock of real_life.decode.write_png_folder on the same decoded frames with coder='device' and with coder='pillow' (what
    decode.py -o folder/ spends behind the decode itself, which is the same for both);
  * file sizes against Pillow's default for those frames and for the analytic pictures of tests/png_cases.py at sigma = 3 and 1,
    and there against zlib Z_RLE on the same filtered bytes cut into the same segments.
The frames: the analytic picture, shifted by the frame index, plus Gaussian noise of 3 levels per frame, through
ops.rgb8_to_yuv420u8.  The first run of every path warms it up and is dropped.  experiments/png.md.
usage: tools/bench_png.py [out.json] [frames] [repeats]"""
import io
import json
import os
import shutil
import sys
import tempfile
import time
import zlib

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import png_cases as pcs  # noqa: E402
from aivc_amd import ops, png  # noqa: E402
from aivc_amd.real_life.decode import write_png_folder  # noqa: E402

H, W = 1080, 1920


def med(v):
    return sorted(v)[len(v) // 2]


def pillow_bytes(pix):
    from PIL import Image
    buf = io.BytesIO()
    t0 = time.perf_counter()
    Image.fromarray(pix).save(buf, format='PNG')
    return len(buf.getvalue()), time.perf_counter() - t0


def folder_bytes(path):
    return sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 33
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    base = pcs.analytic_picture(H, W, 0).astype(np.float64)
    rgb = np.stack([np.clip(np.rint(np.roll(base, 4 * i, 1) + rng.normal(0, 3, base.shape)), 0, 255).astype(np.uint8) for i in range(n)])
    y, u, v = ops.rgb8_to_yuv420u8(torch.from_numpy(rgb).to(dev))
    frames = [{'y': y[i:i + 1], 'u': u[i:i + 1], 'v': v[i:i + 1]} for i in range(n)]
    pictures = ops.yuv8_to_rgb8(y, u, v)  # what the folder holds
    res = {'frames': n, 'size': '%dx%d' % (W, H), 'repeats': repeats}

    # 1. the coder alone
    dev_ms, wall_ms = {'png_deflate': [], 'png_gather': []}, []
    for r in range(repeats + 1):
        ops.PROFILE_HBM = []
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        streams = ops.png_encode(pictures, 5)
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        prof, ops.PROFILE_HBM = ops.PROFILE_HBM, None
        if r:
            wall_ms.append((t1 - t0) * 1e3)
            for name in dev_ms:
                dev_ms[name].append(sum(e0.elapsed_time(e1) for k, _, e0, e1 in prof if k == name))
    res['png_encode'] = {'device_ms': {k: [round(x, 3) for x in t] for k, t in dev_ms.items()},
                         'device_ms_median_total': round(med([a + b for a, b in zip(*dev_ms.values())]), 3),
                         'wall_ms': [round(x, 1) for x in wall_ms], 'wall_ms_median': round(med(wall_ms), 1),
                         'stream_bytes': sum(len(s) for s in streams), 'raw_bytes': n * H * (1 + 3 * W)}
    print(json.dumps(res['png_encode']), flush=True)

    # 2. the folder
    tmp = tempfile.mkdtemp(prefix='bench_png_')
    try:
        walls = {'device': [], 'pillow': []}
        for coder, runs in (('device', repeats + 1), ('pillow', 1)):
            for r in range(runs):
                folder = os.path.join(tmp, '%s_%d' % (coder, r))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                write_png_folder(frames, folder, dev, list(range(n)), coder)
                walls[coder].append((time.perf_counter() - t0) * 1e3)
            res[coder + '_folder_bytes'] = folder_bytes(folder)
        from PIL import Image
        same = all(np.array_equal(np.asarray(Image.open(os.path.join(tmp, 'device_0', '%d.png' % i))),
                                  np.asarray(Image.open(os.path.join(tmp, 'pillow_0', '%d.png' % i)))) for i in (0, n - 1))
        res['write_png_folder'] = {'device_wall_ms': [round(x, 1) for x in walls['device'][1:]], 'device_wall_ms_median': round(med(walls['device'][1:]), 1),
                                   'pillow_wall_ms': round(walls['pillow'][0], 1), 'same_pixels': bool(same),
                                   'pillow_over_device': round(walls['pillow'][0] / med(walls['device'][1:]), 1),
                                   'device_over_pillow_bytes': round(res['device_folder_bytes'] / res['pillow_folder_bytes'], 4)}
        print(json.dumps(res['write_png_folder']), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)

    # 3. the analytic pictures
    res['analytic'] = []
    lengths = pcs.segment_lengths(H, W, 3)
    for sigma in (3, 1):
        pix = pcs.analytic_picture(H, W, sigma, seed=1 + sigma)
        z = ops.png_encode(torch.from_numpy(pix[None]).to(dev), 5)[0]
        filtered = zlib.decompress(z)
        rle = pcs.stitched_stream(filtered, lengths, zlib.Z_RLE)
        pil, pil_s = pillow_bytes(pix)
        res['analytic'].append({'sigma': sigma, 'device_stream_bytes': len(z), 'zlib_rle_same_segments_bytes': len(rle),
                                'ratio_to_rle': round(len(z) / len(rle), 5), 'device_file_bytes': len(png.assemble(W, H, 3, z)),
                                'pillow_file_bytes': pil, 'device_over_pillow': round(len(png.assemble(W, H, 3, z)) / pil, 4),
                                'pillow_save_ms': round(pil_s * 1e3, 1)})
        print(json.dumps(res['analytic'][-1]), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
