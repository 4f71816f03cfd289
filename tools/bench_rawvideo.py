#!/usr/bin/env python3
"""ops.raw_to_yuv420u8 / ops.yuv420u8_to_raw on 129-frame clips -- ingest of 1080p yuv444p10le and of 2160p p010le, export of
1080p to yuv420p10le -- against
  * the copy floor: a device-to-device copy of as many bytes as the op reads plus writes (input + output volume), timed in the
    same run -- such a copy reads AND writes that volume, so half its time is the floor of the op's traffic;
  * the numpy statement of tests/rawvideo_cases.py on 16 host threads, over the first `host_frames` frames (a frame takes seconds
    there), scaled to the clip.
experiments/rawvideo.md.

Device time by HIP events around the call (pointer table upload included), the device idle before; the paths alternate, the first
round warms every path up and is dropped; medians and the spread (min ... max).  Frame 0 and the last host frame of every device
result are compared with numpy's by byte.
usage: tools/bench_rawvideo.py [out.json] [repeats] [frames] [host_frames]"""
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rawvideo_cases as rvc  # noqa: E402
from aivc_amd import ops  # noqa: E402

HOST_THREADS = 16
SIZES = {'2160p': (3840, 2160), '1080p': (1920, 1080)}


def med(v):
    return sorted(v)[len(v) // 2]


def stats(v):
    return {'median_ms': round(med(v), 3), 'min_ms': round(min(v), 3), 'max_ms': round(max(v), 3), 'runs': len(v)}


def events(fn):
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def raw_clip(name, w, h, n, dev, seed):
    """n tight frames of random samples in the layout, back to back on the device -> (uint8 blob, bytes per frame)"""
    b, depth, top = rvc.FORMATS[name][:3]
    size = rvc.frame_bytes(name, w, h)
    gen = torch.Generator(device=dev).manual_seed(seed)
    if b == 1:
        return torch.randint(0, 256, (n * size,), device=dev, generator=gen, dtype=torch.uint8), size
    words = torch.randint(0, 1 << depth, (n * size // 2,), device=dev, generator=gen, dtype=torch.int32)
    return (words << (16 - depth if top else 0)).to(torch.int16).view(torch.uint8), size


def case(kind, name, res, n, dev, repeats, pool, host_frames):
    w, h = SIZES[res]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    size = rvc.frame_bytes(name, w, h)
    planes_bytes = n * (h * w + 2 * hc * wc)
    if kind == 'ingest':
        blob, _ = raw_clip(name, w, h, n, dev, 5)
        offsets = [i * size for i in range(n)]
        run = lambda: ops.raw_to_yuv420u8(blob, offsets, name, w, h)  # noqa: E731
        host_in = [blob[i * size:(i + 1) * size].cpu().numpy() for i in range(host_frames)]
        host_one = lambda fr: rvc.ingest(fr, name, w, h)  # noqa: E731
    else:
        gen = torch.Generator(device=dev).manual_seed(6)
        y, u, v = (torch.randint(0, 256, s, device=dev, generator=gen, dtype=torch.uint8) for s in ((n, h, w), (n, hc, wc), (n, hc, wc)))
        run = lambda: ops.yuv420u8_to_raw(y, u, v, name)  # noqa: E731
        host_in = [(y[i].cpu().numpy(), u[i].cpu().numpy(), v[i].cpu().numpy()) for i in range(host_frames)]
        host_one = lambda fr: rvc.export(fr[0], fr[1], fr[2], name)  # noqa: E731
    vol = n * size + planes_bytes
    a = torch.empty(vol, dtype=torch.uint8, device=dev)
    b = torch.empty_like(a)
    paths = {kind: run, 'copy_in_plus_out': lambda: b.copy_(a)}
    times = {k: [] for k in paths}
    got = None
    for r in range(repeats + 1):  # (the first round warms every path up and is dropped)
        for k, fn in paths.items():
            t, out = events(fn)
            if r:
                times[k].append(t)
            if k == kind:
                got = out
            del out
    t0 = time.perf_counter()
    want = list(pool.map(host_one, host_in))
    host_ms = (time.perf_counter() - t0) * 1e3
    equal = True
    for i in (0, host_frames - 1):
        if kind == 'ingest':
            equal = equal and all(np.array_equal(got[k][i].cpu().numpy(), want[i][k]) for k in range(3))
        else:
            equal = equal and np.array_equal(got[i].cpu().numpy(), want[i])
    out = {'op': kind, 'pix_fmt': name, 'size': res, 'frames': n, 'bytes_raw': n * size, 'bytes_planes': planes_bytes,
           'equals_numpy': bool(equal), 'numpy_16_threads': {'frames': host_frames, 'ms': round(host_ms, 1),
                                                             'scaled_to_clip_ms': round(host_ms * n / host_frames, 1)}}
    out.update({k: stats(v) for k, v in times.items()})
    dev_ms, floor_ms = out[kind]['median_ms'], out['copy_in_plus_out']['median_ms'] / 2
    out['traffic_floor_ms'] = round(floor_ms, 3)
    out['device_over_floor'] = round(dev_ms / floor_ms, 2)
    out['numpy_over_device'] = round(out['numpy_16_threads']['scaled_to_clip_ms'] / dev_ms, 1)
    out['tbps_in_plus_out'] = round(vol / (dev_ms * 1e-3) / 1e12, 3)
    return out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    n = int(sys.argv[3]) if len(sys.argv) > 3 else 129
    host_frames = min(n, int(sys.argv[4]) if len(sys.argv) > 4 else 16)
    dev = torch.device('cuda:0')
    res = {'host_threads': HOST_THREADS, 'repeats': repeats, 'cases': []}
    with ThreadPoolExecutor(HOST_THREADS) as pool:
        for kind, name, size in (('ingest', 'yuv444p10le', '1080p'), ('ingest', 'p010le', '2160p'), ('export', 'yuv420p10le', '1080p')):
            res['cases'].append(case(kind, name, size, n, dev, repeats, pool, host_frames))
            print(json.dumps(res['cases'][-1]), flush=True)
            torch.cuda.empty_cache()
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(json.dumps(res) + '\n')


if __name__ == '__main__':
    main()
