"""aivc_frame_sse_u8 / aivc_frame_aux_stats (include/aivc_hip_quality.h) against numpy, each case plain and under the guard-zone and
poison harness of tests/guarded.py with both fills (every input between guard zones, every buffer aivc_amd.ops allocates -- the
partial sums, the lanes, the results -- an arena whose untouched payload is poison; the two runs must agree byte for byte).

frame_sse_u8 is integer arithmetic: it must EQUAL numpy's int64 sums.  Shapes are (n, h, w); the chroma planes are ceil-sized.
  (3, 5, 3)      less than one wavefront per plane; frames 1 and 2 start off a 16-byte boundary (15 and 30 bytes in)
  (2, 35, 67)    odd sizes, chroma 18 x 34: heads in front of the first 16-byte boundary, 16-byte bodies, tails
  (2, 515, 517)  266255 luma bytes > the 262144 bytes one pass of the 64 workgroups of a plane covers: the strided walk
  0 against 255  every term the maximum 65025; identical planes: zeros
  planes whose alignment differs between source and reconstruction: the byte-by-byte path

frame_aux_stats adds fp64 terms in a fixed order: against math.fsum of the same terms (exact) the error of ANY order of n
additions is below n x 2^-53 x sum |term|.  (3, 5, 3): most lanes empty; (2, 35, 67); (2, 131, 129): 16899 pixels, more than
the 16384 lanes, so a lane adds more than one pixel.  Layouts: warping with 4 stored channels (16-byte loads), with 5, as the
3-channel slice of a 4-channel tensor (what FrameCodec.encode_batch hands over), code with 3 and 4 stored channels; the I
frame's NULL pointers; batches split differently give the same bits."""
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu


def planes(rng, n, h, w, kind='random'):
    hc, wc = (h + 1) // 2, (w + 1) // 2
    out = {}
    for k, shp in (('y', (n, h, w)), ('u', (n, hc, wc)), ('v', (n, hc, wc))):
        if kind == 'random':
            out[k] = rng.integers(0, 256, shp, dtype=np.uint8)
        else:
            out[k] = np.full(shp, kind, np.uint8)
    return out


def sse_numpy(a, b):
    return np.stack([((a[k].astype(np.int64) - b[k].astype(np.int64)) ** 2).reshape(a[k].shape[0], -1).sum(axis=1) for k in 'yuv'], axis=1)


def run_both_ways(call, place_plain, cuda):
    """call(placer) plain, then under guard_ops with both fills -> the plain result as a numpy array; all three must be equal bytes"""
    plain = call(place_plain).cpu().numpy()
    guarded_bytes = both_fills(lambda fill: call(lambda a: guarded(a, cuda, fill)))
    assert guarded_bytes == plain.tobytes()
    return plain


SSE_CASES = [(3, 5, 3, 'random', 'random'), (2, 35, 67, 'random', 'random'), (2, 515, 517, 'random', 'random'),
             (2, 35, 67, 0, 255), (2, 35, 67, 255, 0), (2, 35, 67, 'random', 'same')]


@pytest.mark.parametrize('n,h,w,ka,kb', SSE_CASES)
def test_frame_sse_u8_equals_numpy(n, h, w, ka, kb, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(n * 100000 + h * 100 + w)
    a = planes(rng, n, h, w, ka)
    b = {k: v.copy() for k, v in a.items()} if kb == 'same' else planes(rng, n, h, w, kb)
    want = sse_numpy(a, b)
    if (ka, kb) in ((0, 255), (255, 0)):
        assert want[0, 0] == 65025 * h * w
    if kb == 'same':
        assert not want.any()

    def call(place):
        got = ops.frame_sse_u8({k: place(a[k]) for k in 'yuv'}, {k: place(b[k]) for k in 'yuv'})
        assert got.dtype == torch.int64 and tuple(got.shape) == (n, 3)
        return got
    got = run_both_ways(call, lambda x: torch.from_numpy(x).to(cuda), cuda)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('n,h,w', [(3, 5, 3), (2, 35, 67)])
def test_frame_sse_u8_planes_of_different_alignment(n, h, w, cuda):
    """the reconstruction's planes start one byte into their buffers: no common 16-byte grid with the source's"""
    from aivc_amd import ops
    rng = np.random.default_rng(7 + h)
    a, b = planes(rng, n, h, w), planes(rng, n, h, w)
    want = sse_numpy(a, b)

    def call(place):
        shifted = {}
        for k in 'yuv':
            flat = place(np.concatenate([np.zeros(1, np.uint8), b[k].reshape(-1)]))
            shifted[k] = flat[1:].view(b[k].shape)
            assert shifted[k].is_contiguous() and shifted[k].data_ptr() % 2 == 1
        return ops.frame_sse_u8({k: place(a[k]) for k in 'yuv'}, shifted)
    got = run_both_ways(call, lambda x: torch.from_numpy(x).to(cuda), cuda)
    assert np.array_equal(got, want)


def test_frame_sse_u8_rejections(cuda):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    a = {k: torch.from_numpy(v) for k, v in planes(np.random.default_rng(1), 2, 6, 8).items()}
    with pytest.raises(AivcNativeError):
        ops.frame_sse_u8(a, a)  # CPU tensors
    dev = {k: v.to(cuda) for k, v in a.items()}
    with pytest.raises(ValueError):
        ops.frame_sse_u8(dev, dict(dev, u=dev['u'][:, :2]))


# ---- frame_aux_stats ---------------------------------------------------------------------------------------------------------------
def aux_inputs(rng, n, h, w, cs_warp, cs_code):
    return {'alpha': rng.random((n, h, w), dtype=np.float32), 'beta': rng.random((n, h, w), dtype=np.float32) ** 2,
            'warping': (rng.random((n, h, w, cs_warp), dtype=np.float32) * 2 - 0.5).astype(np.float32),
            'code': rng.random((n, h, w, cs_code), dtype=np.float32)}


def check_against_fsum(got, d, c, null=False):
    """got [n,3] against math.fsum of the kernel's terms, per frame, within count x 2^-53 x sum |term|"""
    n, h, w = d['code'].shape[:3]
    for f in range(n):
        code = d['code'][f, :, :, :c].astype(np.float64)
        warp = np.zeros_like(code) if null else d['warping'][f, :, :, :c].astype(np.float64)
        diff = warp - code
        terms = [np.ones(h * w) if null else d['alpha'][f].astype(np.float64).ravel(),
                 np.ones(h * w) if null else d['beta'][f].astype(np.float64).ravel(), (diff * diff).ravel()]
        for q, t in enumerate(terms):
            exact = math.fsum(t.tolist())
            bound = t.size * 2.0 ** -53 * math.fsum(np.abs(t).tolist())
            assert abs(float(got[f, q]) - exact) <= bound, (f, q, float(got[f, q]), exact, bound)
        if null:
            assert float(got[f, 0]) == h * w and float(got[f, 1]) == h * w


AUX_SHAPES = [(3, 5, 3), (2, 35, 67), (2, 131, 129)]
assert AUX_SHAPES[2][1] * AUX_SHAPES[2][2] > 16384


@pytest.mark.parametrize('n,h,w', AUX_SHAPES)
@pytest.mark.parametrize('cs_warp,cs_code', [(4, 3), (5, 4), (3, 3)])
def test_frame_aux_stats_against_fsum(n, h, w, cs_warp, cs_code, cuda):
    from aivc_amd import ops
    d = aux_inputs(np.random.default_rng(h * 1000 + w * 10 + cs_warp), n, h, w, cs_warp, cs_code)

    def call(place):
        t = {k: place(v) for k, v in d.items()}
        got = ops.frame_aux_stats(t['alpha'], t['beta'], t['warping'], t['code'], c=3)
        assert got.dtype == torch.float64 and tuple(got.shape) == (n, 3)
        return got
    check_against_fsum(run_both_ways(call, lambda x: torch.from_numpy(x).to(cuda), cuda), d, 3)


@pytest.mark.parametrize('n,h,w', AUX_SHAPES[:2])
def test_frame_aux_stats_channel_slice_in_place(n, h, w, cuda):
    """warping as FrameCodec.encode_batch hands it over: the first 3 channels of the 4-channel x_warp, a view"""
    from aivc_amd import ops
    d = aux_inputs(np.random.default_rng(h + w), n, h, w, 4, 3)

    def call(place):
        t = {k: place(v) for k, v in d.items()}
        view = t['warping'][..., :3]
        assert not view.is_contiguous() and view.data_ptr() == t['warping'].data_ptr()
        return ops.frame_aux_stats(t['alpha'], t['beta'], view, t['code'], c=3)
    got = run_both_ways(call, lambda x: torch.from_numpy(x).to(cuda), cuda)
    check_against_fsum(got, d, 3)
    whole = ops.frame_aux_stats(*(torch.from_numpy(d[k]).to(cuda) for k in ('alpha', 'beta', 'warping', 'code')), c=3)
    assert whole.cpu().numpy().tobytes() == got.tobytes()


@pytest.mark.parametrize('n,h,w', AUX_SHAPES)
@pytest.mark.parametrize('cs_code', [3, 4])
def test_frame_aux_stats_intra_frame_null_pointers(n, h, w, cs_code, cuda):
    """no alpha, beta, warping: sums of maps of ones (exactly h x w) and of code^2"""
    from aivc_amd import ops
    d = aux_inputs(np.random.default_rng(h * w + cs_code), n, h, w, 4, cs_code)
    got = run_both_ways(lambda place: ops.frame_aux_stats(None, None, None, place(d['code']), c=3),
                        lambda x: torch.from_numpy(x).to(cuda), cuda)
    check_against_fsum(got, d, 3, null=True)


def test_frame_aux_stats_bits_do_not_depend_on_the_batching(cuda):
    """the same 5 frames in one launch, one by one, and in batches of 2, 2, 1 (FrameCodec's max_batch): identical bits"""
    from aivc_amd import ops
    n, h, w = 5, 35, 67
    d = aux_inputs(np.random.default_rng(99), n, h, w, 4, 3)
    t = {k: torch.from_numpy(v).to(cuda) for k, v in d.items()}

    def run(max_batch):
        parts = [ops.frame_aux_stats(*(t[k][s:s + max_batch] for k in ('alpha', 'beta', 'warping', 'code')), c=3)
                 for s in range(0, n, max_batch)]
        return torch.cat(parts).cpu().numpy().tobytes()
    whole = run(n)
    assert run(1) == whole and run(2) == whole
    a = {k: torch.from_numpy(v).to(cuda) for k, v in planes(np.random.default_rng(3), n, h, w).items()}
    b = {k: torch.from_numpy(v).to(cuda) for k, v in planes(np.random.default_rng(4), n, h, w).items()}
    sse = ops.frame_sse_u8(a, b)
    split = torch.cat([ops.frame_sse_u8({k: a[k][s:s + 2] for k in 'yuv'}, {k: b[k][s:s + 2] for k in 'yuv'}) for s in range(0, n, 2)])
    assert torch.equal(sse, split)


def test_frame_aux_stats_rejections(cuda):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    d = aux_inputs(np.random.default_rng(5), 2, 4, 6, 4, 3)
    with pytest.raises(AivcNativeError):
        ops.frame_aux_stats(None, None, None, torch.from_numpy(d['code']), c=3)
    t = {k: torch.from_numpy(v).to(cuda) for k, v in d.items()}
    with pytest.raises(ValueError):
        ops.frame_aux_stats(t['alpha'][:, :2], t['beta'], t['warping'], t['code'], c=3)
    with pytest.raises(ValueError):
        ops.frame_aux_stats(t['alpha'], t['beta'], t['warping'][:1], t['code'], c=3)
    with pytest.raises(ValueError):
        ops.frame_aux_stats(None, None, None, t['code'][..., :2], c=3)
