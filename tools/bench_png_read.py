#!/usr/bin/env python3
"""The device PNG reader (png.read_pictures: ops.inflate, ops.png_unfilter) on 33 frames of 1080p against Pillow on one host core,
the sibling of tools/bench_png.py and on the same frames.  Pillow writes them once as a triplet folder (<idx>_{y,u,v}.png) and
once as an RGB folder (<idx>.png), both on local disk.  Per folder:
  * device time of aivc_inflate and of aivc_png_unfilter: HIP events around the calls of the C ABI (ops.PROFILE_HBM);
  * wall clock of real_life.encode.read_png_folder(reader='device'), from the files to planes on the device;
  * wall clock of read_png_folder(reader='pillow') in the same process and run: the path without the reader, the baseline.
The first run of each path warms it up and is dropped; the runs that follow are all shown.  experiments/png_read.md.
usage: tools/bench_png_read.py [out.json] [frames] [repeats]"""
import contextlib
import io
import json
import os
import shutil
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import png_cases as pcs  # noqa: E402
from aivc_amd import ops  # noqa: E402
from aivc_amd.real_life.encode import read_png_folder  # noqa: E402

H, W = 1080, 1920


def timed_read(folder, dev, reader):
    """-> (wall ms, {launch name: device ms}, the frames)"""
    ops.PROFILE_HBM = [] if reader == 'device' else None
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        frames, _, _ = read_png_folder(folder, 0, -1, dev, reader)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    prof, ops.PROFILE_HBM = ops.PROFILE_HBM or [], None
    ms = {}
    for name, _, e0, e1 in prof:
        ms[name] = ms.get(name, 0.0) + e0.elapsed_time(e1)
    return wall, ms, frames


def main():
    from PIL import Image
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 33
    repeats = int(sys.argv[3]) if len(sys.argv) > 3 else 3
    dev = torch.device('cuda:0')
    rng = np.random.default_rng(0)
    base = pcs.analytic_picture(H, W, 0).astype(np.float64)
    rgb = np.stack([np.clip(np.rint(np.roll(base, 4 * i, 1) + rng.normal(0, 3, base.shape)), 0, 255).astype(np.uint8) for i in range(n)])
    y, u, v = ops.rgb8_to_yuv420u8(torch.from_numpy(rgb).to(dev))
    pictures = ops.yuv8_to_rgb8(y, u, v).cpu().numpy()  # what bench_png.py's folder holds
    planes = {k: t.cpu().numpy() for k, t in (('y', y), ('u', u), ('v', v))}
    res = {'frames': n, 'size': '%dx%d' % (W, H), 'repeats': repeats}
    tmp = tempfile.mkdtemp(prefix='bench_png_read_')
    try:
        folders = {'triplets': os.path.join(tmp, 'triplets'), 'rgb': os.path.join(tmp, 'rgb')}
        for d in folders.values():
            os.makedirs(d)
        for i in range(n):
            Image.fromarray(pictures[i]).save(os.path.join(folders['rgb'], '%d.png' % i))
            for k in 'yuv':
                Image.fromarray(planes[k][i]).save(os.path.join(folders['triplets'], '%d_%s.png' % (i, k)))
        for kind, folder in folders.items():
            row = {'files': len(os.listdir(folder)), 'file_bytes': sum(os.path.getsize(os.path.join(folder, f)) for f in os.listdir(folder)),
                   'device_wall_ms': [], 'pillow_wall_ms': [], 'inflate_device_ms': [], 'png_unfilter_device_ms': []}
            same = True
            for r in range(repeats + 1):
                wall_d, ms, got = timed_read(folder, dev, 'device')
                wall_p, _, want = timed_read(folder, dev, 'pillow')
                if r == 0:  # (the dropped run checks that the two readers agree)
                    same = all(torch.equal(a[k], b[k]) for a, b in zip(got, want) for k in 'yuv')
                    continue
                row['device_wall_ms'].append(round(wall_d, 1))
                row['pillow_wall_ms'].append(round(wall_p, 1))
                row['inflate_device_ms'].append(round(ms.get('inflate', 0.0), 2))
                row['png_unfilter_device_ms'].append(round(ms.get('png_unfilter', 0.0), 2))
            row['same_planes'] = bool(same)
            row['device_faster_in_every_run'] = all(d < p for d, p in zip(row['device_wall_ms'], row['pillow_wall_ms']))
            res[kind] = row
            print(json.dumps({kind: row}), flush=True)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
