#!/usr/bin/env python3
"""ops.md5_planes on stacks of 1080p planes against the host path it replaces (device -> host copy of the same planes, then
hashlib.md5 per plane), in one process, the two alternating (experiments/frame_digests.md).
Device time: HIP events around the three launches (y, u, v) of a batch of frames; host time: a host clock around .cpu() +
hashlib, which ends with the data on the host.  The rate per wavefront is that of the y launch alone: 64 planes are one
wavefront, 64 x plane bytes over its time, in bytes per cycle at the MI355X's peak engine clock of 2400 MHz (a lower bound of
the rate per cycle where the device runs slower than that).
usage: tools/bench_digest.py [out.json] [repeats] [clock MHz]"""
import hashlib
import json
import os
import sys
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from aivc_amd import ops  # noqa: E402


def events(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def host_path(planes):
    t0 = time.perf_counter()
    out = []
    for p in planes:
        a = p.cpu().numpy()
        out.append(b''.join(hashlib.md5(a[i].tobytes()).digest() for i in range(a.shape[0])))
    return (time.perf_counter() - t0) * 1e3, out


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 5
    dev = torch.device('cuda:0')
    h, w = 1080, 1920
    clock_hz = (float(sys.argv[3]) if len(sys.argv) > 3 else 2400.0) * 1e6
    res = {'height': h, 'width': w, 'clock_mhz': clock_hz / 1e6, 'repeats': repeats, 'cases': []}
    gen = torch.Generator(device=dev).manual_seed(5)
    for n in (64, 132):
        planes = [torch.randint(0, 256, s, dtype=torch.uint8, device=dev, generator=gen)
                  for s in ((n, h, w), (n, h // 2, w // 2), (n, h // 2, w // 2))]
        dev_ms, host_ms, y_ms = [], [], []
        for r in range(repeats + 1):  # (the first round warms both paths up and is dropped)
            t, d = events(lambda: [ops.md5_planes(p) for p in planes])
            ty, _ = events(lambda: ops.md5_planes(planes[0]))
            th, hd = host_path(planes)
            assert [x.cpu().numpy().tobytes() for x in d] == hd, 'device digests are not hashlib\'s'
            if r:
                dev_ms.append(t), host_ms.append(th), y_ms.append(ty)
        med = lambda v: sorted(v)[len(v) // 2]
        lanes = min(n, 64)
        case = {'frames': n, 'bytes': sum(p.numel() for p in planes), 'device_ms': [round(x, 3) for x in dev_ms],
                'host_ms': [round(x, 3) for x in host_ms], 'y_launch_ms': [round(x, 3) for x in y_ms],
                'device_ms_median': round(med(dev_ms), 3), 'host_ms_median': round(med(host_ms), 3),
                'host_over_device': round(med(host_ms) / med(dev_ms), 2),
                'y_bytes_per_cycle_per_wavefront': round(lanes * h * w / (med(y_ms) * 1e-3 * clock_hz), 3),
                'y_cycles_per_block_per_wavefront': round(med(y_ms) * 1e-3 * clock_hz / (h * w / 64 + 1), 1)}
        res['cases'].append(case)
        del planes
    line = json.dumps(res)
    print(line)
    if out_path:
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
