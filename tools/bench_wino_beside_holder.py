"""A Winograd launch beside a workgroup of another kernel that holds 100 KB of LDS (aivc_diag_hold_lds): the two 5x5 launches
of bench_poly.py's LAYERS at n16 under fp32w, each timed alone and with the holder started on a side stream just before it.
The Winograd kernels take nearly all of a CU's LDS per workgroup, so one of their workgroups cannot start on the holder's CU:
what the launch then costs is what the block walk makes of a workgroup that starts late.  HOLD_MS (default 3): how long the
holder stays, calibrated from a timed run of it.  Select the library with AIVC_HIP_LIB for an A/B.
Per shape: 3 warm-up launches, then 10 launches each way, every one between its own events; mean and shortest."""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import torch  # noqa: E402
from aivc_amd import abi, ops  # noqa: E402

LAYERS = [('poly5', 16, 540, 960, 64, 128), ('tconv5', 16, 272, 480, 128, 64)]  # form, frames, h, w, c_in, c_out
LDS = 100 * 1024


def timed(fn, before=None):
    torch.cuda.synchronize()
    if before:
        before()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def main():
    dev = torch.device('cuda:0')
    side = torch.cuda.Stream()
    sink = torch.empty(64, dtype=torch.int32, device=dev)
    hold_ms = float(os.environ.get('HOLD_MS', '3'))
    probe = 1 << 14
    for _ in range(2):
        t = timed(lambda: ops.diag_hold_lds(LDS, probe, sink))
    iterations = max(1, min(1 << 20, int(probe * hold_ms / t)))
    t_hold = min(timed(lambda: ops.diag_hold_lds(LDS, iterations, sink)) for _ in range(3))
    print('holder: %d iterations of %.1f ns, %.3f ms alone' % (iterations, t / probe * 1e6, t_hold), flush=True)

    def hold():
        with torch.cuda.stream(side):
            ops.diag_hold_lds(LDS, iterations, sink)
    prev = ops.set_precision('fp32w')
    try:
        for (form, nb, h, w, ci, co) in LAYERS:
            g = torch.Generator(device=dev).manual_seed(7)
            x = torch.randn(nb, h, w, ci, device=dev, generator=g)
            wt = torch.randn(co, 5, 5, ci, device=dev, generator=g) * 0.02
            b = torch.rand(co, device=dev, generator=g) * 0.1
            if form == 'poly5':
                fn = lambda: ops.conv2d(x, wt, b, stride=2, pad=2)
            else:
                fn = lambda: ops.conv2d(x, wt, b, mode=abi.MODE_TCONV, stride=2)
            for _ in range(3):
                y = fn()
            alone = [timed(fn) for _ in range(10)]
            beside = [timed(fn, before=hold) for _ in range(10)]
            print('%s %d->%d %dx%d n%d: alone %.4f ms (min %.4f) | beside a %.1f ms holder %.4f ms (min %.4f, max %.4f) = x%.3f  sum %.9e'
                  % (form, ci, co, h, w, nb, sum(alone) / 10, min(alone), t_hold, sum(beside) / 10, min(beside), max(beside),
                     sum(beside) / sum(alone), float(y.double().sum())), flush=True)
            del x, y
    finally:
        ops.set_precision(prev)


if __name__ == '__main__':
    main()
