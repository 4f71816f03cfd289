#!/usr/bin/env python3
"""Generate tests/golden/quality_log.npz by IMPORTING the reference's own metric and logging functions
(src/model_mngt/loss_function.py: compute_metrics_one_GOP, average_N_frame; src/func_util/result_logging.py:
generate_header_file, generate_log_metric_one_frame) and running them, torch fp32 on the CPU, on seeded inputs the way
infer_one_GOP / infer_one_sequence call them (src/model_mngt/model_management.py:161-241, 329-334).

Needs the reference tree (AIVC_REFERENCE_SRC, default /root/reference/src); the test suite uses the committed fixture.  The
fixture holds the seed, the reference's numbers and its text lines -- neither the random tensors (make_inputs(seed) rebuilds
them, here and in the tests) nor anything of the reference's source.

    python tools/gen_golden_quality_log.py [--out FILE.npz]

The case: two intra-period units of three frames (an I frame and two inter frames each), luma 80 x 48 so that the chroma
planes are 40 x 24 and the five-scale pyramid meets odd sizes (5 x 3 -> 3 x 2), the last frame padding.  The reconstruction
is distorted strongly enough that every MS-SSIM is <= 0.95: the dB figure -10 log10(1 - ms_ssim) then amplifies an error of
the score by at most 10 / ln 10 / 0.05 = 87, which keeps a dB tolerance derived from the score's meaningful.
"""
import os
import sys

sys.dont_write_bytecode = True
import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gen_golden import install_stubs  # noqa: E402

REF = os.environ.get('AIVC_REFERENCE_SRC', '/root/reference/src')
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'quality_log.npz')

SEED = 20211
H, W = 48, 80
UNIT, NB_GOP, NB_PAD = 3, 2, 1
LAMBDA = 0.0125
FIRST_FRAME = 7
SEQUENCE_NAME = 'synthetic_80x48'
MAX_MS_SSIM = 0.95
KEYS = ('loss', 'mse', 'mse_warping', 'psnr', 'psnr_warping', 'codec_rate_bpp', 'mode_rate_bpp', 'total_rate_bpp', 'mean_alpha',
        'mean_beta', 'ms_ssim', 'ms_ssim_db', 'h', 'w')


def _plane_pair(rng, h, w, phase, noise):
    y, x = np.mgrid[0:h, 0:w]
    base = 128 + 60 * np.sin(2 * np.pi * x / 37.0 + phase) + 45 * np.cos(2 * np.pi * y / 23.0 - phase) + rng.normal(0, 6, (h, w))
    a = np.clip(np.rint(base), 0, 255).astype(np.uint8)
    b = np.clip(np.rint(base + rng.normal(0, noise, (h, w))), 0, 255).astype(np.uint8)
    return a, b


def make_inputs(seed=SEED):
    """-> the NB_GOP * UNIT frames in coding-unit order, each a dict:
         src, rec   {'y': uint8 [H,W], 'u', 'v': uint8 [H/2,W/2]}   the frame to code and its reconstruction
         alpha, beta float32 [H,W], warping float32 [H,W,3]          None for the I frame of a unit
         code        float32 [H,W,3]
         sections    four sizes in bytes (MOFNet z, y, CodecNet z, y; an I frame has no MOFNet sections)"""
    rng = np.random.default_rng(seed)
    hc, wc = (H + 1) // 2, (W + 1) // 2
    frames = []
    for k in range(NB_GOP * UNIT):
        intra = k % UNIT == 0
        noise = 32.0 + 4.0 * k
        src, rec = {}, {}
        for name, (h, w) in (('y', (H, W)), ('u', (hc, wc)), ('v', (hc, wc))):
            src[name], rec[name] = _plane_pair(rng, h, w, 0.3 * k + 'yuv'.index(name), noise)
        fr = {'src': src, 'rec': rec, 'code': rng.random((H, W, 3), dtype=np.float32)}
        if intra:
            fr.update(alpha=None, beta=None, warping=None, sections=[0, 0] + [int(v) for v in rng.integers(40, 900, 2)])
        else:
            fr.update(alpha=rng.random((H, W), dtype=np.float32), beta=rng.random((H, W), dtype=np.float32) ** 2,
                      warping=np.clip(fr['code'] + rng.normal(0, 0.05, (H, W, 3)).astype(np.float32), 0, 1).astype(np.float32),
                      sections=[int(v) for v in rng.integers(3, 400, 4)])
        frames.append(fr)
    return frames


def _yuv_dic(planes):
    return {k: torch.from_numpy(planes[k].astype(np.float32) / np.float32(255.0))[None, None] for k in 'yuv'}


def _nchw3(x):
    return torch.from_numpy(np.ascontiguousarray(x)).permute(2, 0, 1)[None].contiguous()


def generate(seed=SEED):
    """run the reference on make_inputs(seed) -> the fixture's arrays"""
    install_stubs()
    if REF not in sys.path:
        sys.path.insert(0, REF)
    from func_util.result_logging import generate_header_file, generate_log_metric_one_frame
    from model_mngt.loss_function import average_N_frame, compute_metrics_one_GOP
    for fn in (generate_header_file, compute_metrics_one_GOP):  # (this package aliases the reference's module names when asked to)
        assert os.path.abspath(sys.modules[fn.__module__].__file__).startswith(os.path.abspath(REF)), fn.__module__
    frames = make_inputs(seed)
    sequence_result = {}
    for g in range(NB_GOP):
        target, net_out = {}, {}
        for f in range(UNIT):
            fr = frames[g * UNIT + f]
            name = 'frame_%d' % f
            target[name] = _yuv_dic(fr['src'])
            ones, zeros = torch.ones((1, 3, H, W)), torch.zeros((1, 3, H, W))
            sec = fr['sections']
            net_out[name] = {  # the entries FullNet.GOP_forward fills (an I frame: maps of ones, a zero warping)
                'x_hat': _yuv_dic(fr['rec']),
                'alpha': ones if fr['alpha'] is None else torch.from_numpy(fr['alpha'])[None, None].repeat(1, 3, 1, 1),
                'beta': ones if fr['beta'] is None else torch.from_numpy(fr['beta'])[None, None].repeat(1, 3, 1, 1),
                'mode_rate_z': torch.tensor([8.0 * sec[0]]), 'mode_rate_y': torch.tensor([8.0 * sec[1]]),
                'codec_rate_z': torch.tensor([8.0 * sec[2]]), 'codec_rate_y': torch.tensor([8.0 * sec[3]]),
                'warping': zeros if fr['warping'] is None else _nchw3(fr['warping']),
                'code': _nchw3(fr['code']),
            }
        with torch.no_grad():
            _, result = compute_metrics_one_GOP({'net_out': net_out, 'target': target, 'l_mof': LAMBDA, 'l_codec': LAMBDA})
        for f in range(UNIT):
            sequence_result['frame_%d' % (g * UNIT + f + FIRST_FRAME)] = result['frame_%d' % f]
    sequence_result['sequence'] = average_N_frame({'x': sequence_result, 'nb_pad_frame': NB_PAD})
    worst = max(float(sequence_result[f]['ms_ssim']) for f in sequence_result)
    if not worst <= MAX_MS_SSIM:
        raise SystemExit('the reconstruction is not distorted enough: MS-SSIM %.4f > %.2f' % (worst, MAX_MS_SSIM))
    lines = [generate_header_file()]
    for f in sequence_result:
        sequence_result[f]['pic_name'], sequence_result[f]['frame_idx'] = SEQUENCE_NAME, f
        lines.append(generate_log_metric_one_frame(sequence_result[f]))
    names = [f for f in sequence_result if f != 'sequence']
    return {
        'seed': np.int64(seed), 'lambda_tradeoff': np.float64(LAMBDA), 'nb_pad_frame': np.int64(NB_PAD),
        'first_frame': np.int64(FIRST_FRAME), 'sequence_name': np.array(SEQUENCE_NAME), 'keys': np.array(KEYS),
        'frame_names': np.array(names),
        'frames': np.array([[float(sequence_result[f][k]) for k in KEYS] for f in names], np.float64),
        'average': np.array([float(sequence_result['sequence'][k]) for k in KEYS], np.float64),
        'lines': np.array(lines),
    }


def main():
    path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == '--out' else OUT
    out = generate()
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path), 'bytes')
    for line in out['lines']:
        print(line, end='')


if __name__ == '__main__':
    main()
