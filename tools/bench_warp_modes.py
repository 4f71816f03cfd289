"""The nine instantiations of warp_modes_kernel (csrc/pixel_ops.hip) next to aivc_warp, same process, same inputs.
python tools/bench_warp_modes.py [frames] [h] [w] [c] [--json PATH]

Device events around REPS launches per window (after a warm-up of every mode), ROUNDS windows per mode taken in
alternation (mode A, mode B, ..., then again) so that a drift of the box hits all alike; reported: the median window and
the spread (min ... max).  GB/s is ALGORITHMIC traffic: the frame in, the flow, the frame out, n * h * w * (2 c + 2) * 4
bytes -- gathered taps that hit the same cache lines are not counted twice.  Flows are a few pixels (the codec's range).
(bilinear, border, align_corners) is forwarded to aivc_warp by the entry point: it is the 'aivc_warp' row itself."""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from aivc_amd import ops  # noqa: E402

REPS, ROUNDS = 20, 7


def main():
    argv = list(sys.argv[1:])
    path = None
    if '--json' in argv:
        i = argv.index('--json')
        path = argv[i + 1]
        del argv[i:i + 2]
    n, h, w, c = (int(a) for a in argv + ['64', '1080', '1920', '4'][len(argv):])
    if not torch.cuda.is_available():
        raise SystemExit('bench_warp_modes: needs the GPU (timings on a CPU mean nothing)')
    dev = torch.device('cuda:0')
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((n, h, w, c), device=dev, generator=g)
    flow = torch.randn((n, h, w, 2), device=dev, generator=g) * 3.0
    modes = [('aivc_warp', ('bilinear', 'border', True))]
    modes += [('%s/%s/%d' % (i, p, a), (i, p, a)) for i in ops.WARP_INTERP for p in ops.WARP_PAD for a in (True, False)
              if (i, p, a) != ('bilinear', 'border', True)]
    for _, m in modes:  # warm-up: code objects, allocator
        for _ in range(3):
            ops.warp(x, flow, *m)
    torch.cuda.synchronize()
    times = {name: [] for name, _ in modes}
    for _ in range(ROUNDS):
        for name, m in modes:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(REPS):
                ops.warp(x, flow, *m)
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / REPS)
    nbytes = n * h * w * (2 * c + 2) * 4
    rows = []
    print('%d frames %d x %d x %d, %.1f MB of algorithmic traffic per call, %d windows of %d calls' % (n, w, h, c, nbytes / 1e6, ROUNDS, REPS))
    for name, _ in modes:
        t = times[name]
        med = statistics.median(t)
        rows.append({'mode': name, 'ms_median': med, 'ms_min': min(t), 'ms_max': max(t), 'gb_per_s': nbytes / med / 1e6})
        print('%-28s %7.3f ms (%.3f ... %.3f)  %6.0f GB/s' % (name, med, min(t), max(t), nbytes / med / 1e6))
    if path:
        with open(path, 'w') as f:
            json.dump({'n': n, 'h': h, 'w': w, 'c': c, 'bytes': nbytes, 'reps': REPS, 'rounds': ROUNDS, 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
