"""aivc_channel_gain_rows / aivc_quantize_center_rows / aivc_dequantize_rows (include/aivc_hip_rates.h): one gain row per image of
a batch.  Their statement is the single-gain entry point applied image by image with that image's row (those are pinned to the
CPU oracle, tests/test_gpu_ops.py): the bits must be EQUAL.  Each case runs plain and under the guard-zone and poison harness of
tests/guarded.py with both fills; the three runs must agree byte for byte.  The single-gain entry points launch the row kernels
as their one-row case (csrc/latent.hip); a second test runs them on a whole batch, where that one row spans the images.

Shapes (n, h, w, c):
  (3, 5, 7, 6)    630 elements: 210 per image, less than a block each (three blocks over the grid's image axis), no multiple of
                  256, c no multiple of 4
  (1, 1, 1, 64)   one image, one position
  (4, 3, 3, 64)   576 elements per image: three blocks in x, the last one partly empty
Data: gains in +-[0.25, 4) with negative entries (the kernels take |g|), the last row of a batch of several images exactly 1.0;
mu on multiples of 1/8 and y = mu + d with d on multiples of 1/4, so that y - mu IS d in fp32: d holds the ties +-0.5, +-1.5,
+-2.5 (half to even), +-255.5, +-256.5 and values well past both ends of the alphabet [-256, 256]."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(3, 5, 7, 6), (1, 1, 1, 64), (4, 3, 3, 64)]
TIES = [0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 255.5, -255.5, 256.5, -256.5, 300.0, -300.0, 1000.25, -1000.25, 256.0, -256.0, 0.0]


def make_data(n, h, w, c):
    rng = np.random.default_rng(1000 * n + 100 * h + 10 * w + c)
    shape = (n, h, w, c)
    mu = rng.integers(-128, 129, shape).astype(np.float32) / 8
    d = rng.integers(-24, 25, shape).astype(np.float32) / 4
    flat = d.reshape(-1)
    where = rng.permutation(flat.size)[:min(flat.size, 3 * len(TIES))]
    flat[where] = np.resize(np.asarray(TIES, np.float32), where.size)
    y = mu + d
    assert np.array_equal(y - mu, d)  # exact in fp32: the ties reach rintf as ties
    gains = (rng.uniform(0.25, 4.0, (n, c)) * rng.choice([-1.0, 1.0], (n, c))).astype(np.float32)
    assert (gains < 0).any()
    if n > 1:
        gains[-1] = 1.0
    q = rng.integers(-256, 257, shape).astype(np.int16)
    q.reshape(-1)[:4] = (-256, 256, 0, -1)
    return {'y': y, 'mu': mu, 'gains': gains, 'q': q}


def run_case(place, d):
    """every entry point and NULL variant once, against the single-gain op image by image -> the row results"""
    from aivc_amd import ops
    t = {k: place(v) for k, v in d.items()}
    n = t['y'].shape[0]
    out = {}

    def per_image(fn):
        return [fn(i, slice(i, i + 1)) for i in range(n)]

    def same(rows, singles, what):
        for i, s in enumerate(singles):
            assert rows[i:i + 1].dtype == s.dtype and torch.equal(rows[i:i + 1], s), '%s: image %d' % (what, i)

    out['gain'] = ops.channel_gain_rows(t['y'], t['gains'])
    same(out['gain'], per_image(lambda i, s: ops.channel_gain(t['y'][s], t['gains'][i])), 'channel_gain_rows')
    out['gain_null'] = ops.channel_gain_rows(t['y'], None)
    same(out['gain_null'], per_image(lambda i, s: ops.channel_gain(t['y'][s], None)), 'channel_gain_rows, NULL gains')
    assert torch.equal(out['gain_null'], t['y'])

    out['q'], out['yh'] = ops.quantize_center_rows(t['y'], t['mu'], t['gains'])
    singles = per_image(lambda i, s: ops.quantize_center(t['y'][s], t['mu'][s], t['gains'][i]))
    same(out['q'], [q for q, _ in singles], 'quantize_center_rows q')
    same(out['yh'], [yh for _, yh in singles], 'quantize_center_rows y_hat')
    assert int(out['q'].min()) == -256 and int(out['q'].max()) == 256  # both ends of the alphabet were reached (and clamped)

    out['q_nogain'], out['yh_nogain'] = ops.quantize_center_rows(t['y'], t['mu'], None)
    singles = per_image(lambda i, s: ops.quantize_center(t['y'][s], t['mu'][s], None))
    same(out['q_nogain'], [q for q, _ in singles], 'quantize_center_rows q, NULL gains')
    same(out['yh_nogain'], [yh for _, yh in singles], 'quantize_center_rows y_hat, NULL gains')

    out['q_nomu'], out['yh_nomu'] = ops.quantize_center_rows(t['y'], None, t['gains'])
    singles = per_image(lambda i, s: ops.quantize_center(t['y'][s], None, t['gains'][i]))
    same(out['q_nomu'], [q for q, _ in singles], 'quantize_center_rows q, NULL mu')
    same(out['yh_nomu'], [yh for _, yh in singles], 'quantize_center_rows y_hat, NULL mu')

    out['q_only'], none = ops.quantize_center_rows(t['y'], t['mu'], t['gains'], want_yhat=False)
    assert none is None and torch.equal(out['q_only'], out['q'])
    none, out['yh_only'] = ops.quantize_center_rows(t['y'], t['mu'], t['gains'], want_q=False)
    assert none is None and torch.equal(out['yh_only'], out['yh'])

    out['deq'] = ops.dequantize_rows(t['q'], t['mu'], t['gains'])
    same(out['deq'], per_image(lambda i, s: ops.dequantize(t['q'][s], t['mu'][s], t['gains'][i])), 'dequantize_rows')
    out['deq_nogain'] = ops.dequantize_rows(t['q'], t['mu'], None)
    same(out['deq_nogain'], per_image(lambda i, s: ops.dequantize(t['q'][s], t['mu'][s], None)), 'dequantize_rows, NULL gains')
    out['deq_nomu'] = ops.dequantize_rows(t['q'], None, t['gains'])
    same(out['deq_nomu'], per_image(lambda i, s: ops.dequantize(t['q'][s], None, t['gains'][i])), 'dequantize_rows, NULL mu')
    # what the decoder does with the encoder's symbols is what the encoder kept
    assert torch.equal(ops.dequantize_rows(out['q'], t['mu'], t['gains']), out['yh'])
    return out


@pytest.mark.parametrize('n,h,w,c', SHAPES)
def test_rows_equal_single_gain_ops_image_by_image(n, h, w, c, cuda):
    d = make_data(n, h, w, c)
    plain = run_case(lambda a: torch.from_numpy(a).to(cuda), d)
    plain = {k: v.cpu().numpy().tobytes() for k, v in plain.items()}
    assert both_fills(lambda fill: run_case(lambda a: guarded(a, cuda, fill), d)) == plain


def run_whole_batch_case(place, d):
    """the single-gain ops on the WHOLE batch with one [c] vector (one flat launch: its blocks straddle the images) against the
    row ops given that vector n times -> the single-gain results"""
    from aivc_amd import ops
    t = {k: place(v) for k, v in d.items()}
    n = t['y'].shape[0]
    vec, table = place(d['gains'][0].copy()), place(np.repeat(d['gains'][:1], n, axis=0))
    out = {}

    def same(key, single, rows):
        assert single.dtype == rows.dtype and torch.equal(single, rows), key
        out[key] = single

    for tag, g, gs in (('', vec, table), ('_nogain', None, None)):
        same('gain' + tag, ops.channel_gain(t['y'], g), ops.channel_gain_rows(t['y'], gs))
        for mtag, mu in (('', t['mu']), ('_nomu', None)):
            q, yh = ops.quantize_center(t['y'], mu, g)
            q_rows, yh_rows = ops.quantize_center_rows(t['y'], mu, gs)
            same('q' + tag + mtag, q, q_rows)
            same('yh' + tag + mtag, yh, yh_rows)
            same('deq' + tag + mtag, ops.dequantize(t['q'], mu, g), ops.dequantize_rows(t['q'], mu, gs))
    return out


@pytest.mark.parametrize('n,h,w,c', [(3, 5, 7, 6), (4, 3, 3, 64)])
def test_single_gain_ops_on_a_whole_batch_equal_the_row_ops_with_one_vector_repeated(n, h, w, c, cuda):
    """The other tests compare one-image slices.  Here the single-gain entry points take the batch as ONE row of n * h * w * c
    elements: 256-thread blocks straddle the image boundaries (210 and 576 elements per image, no multiples of 256; c = 6 is no
    multiple of 4), and every byte must equal the row ops' with the vector repeated n times, NULL gain and NULL mu included."""
    d = make_data(n, h, w, c)
    plain = run_whole_batch_case(lambda a: torch.from_numpy(a).to(cuda), d)
    plain = {k: v.cpu().numpy().tobytes() for k, v in plain.items()}
    assert both_fills(lambda fill: run_whole_batch_case(lambda a: guarded(a, cuda, fill), d)) == plain


def test_wrong_table_shape_is_refused(cuda):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    y = torch.zeros((3, 2, 2, 6), device=cuda)
    for bad in (torch.ones(6, device=cuda), torch.ones((2, 6), device=cuda), torch.ones((3, 4), device=cuda)):
        with pytest.raises(AivcNativeError):
            ops.channel_gain_rows(y, bad)
    with pytest.raises(AivcNativeError):
        ops.channel_gain_rows(y.cpu(), torch.ones((3, 6)))


def test_gain_rows_row_by_row_equals_gain_vector(cuda):
    """a batch's table is gain_vector per distinct rate, stacked: fractional rates have the single-rate path's bits"""
    from aivc_amd.layers.multi_rate.gain_matrix import GainMatrix
    torch.manual_seed(3)
    gm = GainMatrix({'N': 3, 'nb_ft': 6, 'initialize_to_one': False}).to(cuda)
    rates = [0, 0.5, 1.25, 0.5]
    for mode in ('enc', 'dec'):
        rows = gm.gain_rows(rates, mode)
        assert tuple(rows.shape) == (4, 6) and rows.is_cuda and rows.is_contiguous() and rows.dtype == torch.float32
        for i, r in enumerate(rates):
            assert torch.equal(rows[i], gm.gain_vector(r, mode)), (mode, r)
        assert torch.equal(rows[1], rows[3]) and not torch.equal(rows[0], rows[1])
    scalar = GainMatrix({'N': 3, 'nb_ft': 6, 'initialize_to_one': False, 'scalar_gain': True}).to(cuda)
    rows = scalar.gain_rows([2, 0.25], 'dec', 6)
    assert tuple(rows.shape) == (2, 6) and rows.is_contiguous()
    for i, r in enumerate((2, 0.25)):
        assert torch.equal(rows[i], scalar.gain_vector(r, 'dec').expand(6))
