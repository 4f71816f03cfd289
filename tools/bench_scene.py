#!/usr/bin/env python3
"""ops.pair_sad_u8 on the luma planes of a 129-frame 1080p clip (separate, aligned tensors, as read_yuv leaves them) against
  * the same sums as a torch expression on the device, (a.int() - b.int()).abs().sum() per pair, and
  * the time the clip's bytes take at the bandwidth of a float4 copy (MI355X_MICROARCH: 6.29 TB/s measured),
and the wall clock of real_life.encode.encode on the 128-frame 1080p clip of tools/cli_wallclock.py with and without
scene_cut (a clip without cuts: the difference is the price of looking).  experiments/scene_cut.md.

Device time by HIP events.  The clip is 267 MB, about the size of the Infinity Cache, and a call lasts tens of microseconds,
so two figures are taken per path: `warm`, the mean of CALLS back-to-back calls on the same planes (what a cache-resident
clip costs), and `cold`, single calls each behind a 1 GiB fill that evicts the clip (what a clip that has just been
uploaded and pushed out by other work costs).  The two paths alternate; the first round warms both up and is dropped; medians.
Every round compares the kernel's sums with torch's.
usage: tools/bench_scene.py [out.json] [repeats] [encode pairs]"""
import contextlib
import io
import json
import os
import sys
import tempfile
import time

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from aivc_amd import ops  # noqa: E402

COPY_TBPS = 6.29  # float4 copy, measured (8.0 spec)
CALLS = 20


def events(fn, calls=1):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / calls, out


def torch_sums(planes):
    return torch.stack([(b.int() - a.int()).abs().sum() for a, b in zip(planes, planes[1:])])


def med(v):
    return sorted(v)[len(v) // 2]


def kernel_part(dev, repeats):
    n, h, w = 129, 1080, 1920
    gen = torch.Generator(device=dev).manual_seed(5)
    planes = [torch.randint(0, 256, (1, h, w), dtype=torch.uint8, device=dev, generator=gen) for _ in range(n)]
    assert all(p.data_ptr() % 16 == 0 for p in planes)
    # the general path: every other plane one byte into a buffer of its own, so every pair goes through the byte funnel
    odd = [torch.empty(h * w + 1, dtype=torch.uint8, device=dev) for _ in range(n)]
    shifted = [(o[1:] if i % 2 else o[:-1]) for i, o in enumerate(odd)]
    for s, p in zip(shifted, planes):
        s.copy_(p.view(-1))
    flush = torch.empty(1 << 30, dtype=torch.uint8, device=dev)
    paths = {'pair_sad_u8': lambda: ops.pair_sad_u8(planes), 'pair_sad_u8_funnel': lambda: ops.pair_sad_u8(shifted),
             'torch': lambda: torch_sums(planes)}
    warm, cold = {k: [] for k in paths}, {k: [] for k in paths}
    for r in range(repeats + 1):  # (the first round warms every path up and is dropped)
        sums = {}
        for k, fn in paths.items():
            t, sums[k] = events(fn, CALLS if k != 'torch' else 2)
            flush.fill_(r & 255)
            c, _ = events(fn)
            if r:
                warm[k].append(t), cold[k].append(c)
        assert torch.equal(sums['pair_sad_u8'], sums['torch']) and torch.equal(sums['pair_sad_u8_funnel'], sums['torch'])
    nbytes = n * h * w
    floor_ms = nbytes / (COPY_TBPS * 1e12) * 1e3
    out = {'planes': n, 'height': h, 'width': w, 'bytes': nbytes, 'copy_tbps': COPY_TBPS, 'floor_ms': round(floor_ms, 4),
           'repeats': repeats, 'calls_per_warm_window': CALLS}
    for k in paths:
        out[k] = {'warm_ms': [round(x, 4) for x in warm[k]], 'cold_ms': [round(x, 4) for x in cold[k]],
                  'warm_ms_median': round(med(warm[k]), 4), 'cold_ms_median': round(med(cold[k]), 4)}
    for k in ('pair_sad_u8', 'pair_sad_u8_funnel'):
        for kind in ('warm', 'cold'):
            t = out[k]['%s_ms_median' % kind]
            out[k]['torch_over_kernel_' + kind] = round(out['torch']['%s_ms_median' % kind] / t, 1)
            out[k]['fraction_of_floor_' + kind] = round(floor_ms / t, 3)
            out[k]['tbps_' + kind] = round(nbytes / (t * 1e-3) / 1e12, 2)
    return out


def encode_part(dev, pairs):
    from aivc_amd import cli_common
    from aivc_amd.real_life import encode as renc
    from bench import gpu_synthetic_unit
    n, w, h = 128, 1920, 1080
    td = tempfile.mkdtemp(prefix='aivc_scene_')
    raw, bits = os.path.join(td, 'clip_%dx%d_30_420.yuv' % (w, h)), os.path.join(td, 'bits.bin')
    with open(raw, 'wb') as f:
        for fr in gpu_synthetic_unit(w, h, n, 0, dev, 666):
            for k in 'yuv':
                f.write(fr[k].cpu().numpy().tobytes())
    model = cli_common.get_model('absent', dev)
    torch.cuda.synchronize()

    def run(scene_cut):
        sink = io.StringIO()
        with contextlib.redirect_stdout(sink):
            t0 = time.time()
            renc.encode({'model': model, 'sequence_path': raw, 'GOP_struct_name': '1_GOP_32', 'final_file': bits,
                         'idx_starting_frame': 0, 'idx_end_frame': n - 1, 'scene_cut': scene_cut})
            torch.cuda.synchronize()
            dt = time.time() - t0
        with open(bits, 'rb') as f:
            return dt, f.read(), sink.getvalue()
    off, on, blobs, text = [], [], set(), ''
    for r in range(pairs + 1):  # (a warm-up pair first)
        a, blob_a, _ = run(None)
        b, blob_b, text = run(10.0)
        blobs |= {blob_a, blob_b}
        if r:
            off.append(a), on.append(b)
    for p in (raw, bits):
        os.remove(p)
    os.rmdir(td)
    return {'frames': n, 'width': w, 'height': h, 'gop': '1_GOP_32', 'pairs': pairs, 'plain_s': [round(x, 4) for x in off],
            'scene_cut_s': [round(x, 4) for x in on], 'plain_s_median': round(med(off), 4), 'scene_cut_s_median': round(med(on), 4),
            'same_bytes': len(blobs) == 1, 'bitstream_bytes': len(next(iter(blobs))),
            'lines': [l for l in text.split('\n') if l.startswith('[SCENE]') or l.startswith('[INFO] units')]}


def main():
    out_path = sys.argv[1] if len(sys.argv) > 1 else None
    repeats = int(sys.argv[2]) if len(sys.argv) > 2 else 7
    pairs = int(sys.argv[3]) if len(sys.argv) > 3 else 4
    dev = torch.device('cuda:0')
    res = {'kernel': kernel_part(dev, repeats)}
    if pairs > 0:
        with torch.no_grad():
            res['encode'] = encode_part(dev, pairs)
    line = json.dumps(res)
    print(line)
    if out_path:
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
