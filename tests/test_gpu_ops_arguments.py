"""What aivc_amd/ops.py does with an argument no other test passes: a tensor on the CPU, of another dtype, one element short, or a
strided view; an integer one past what the tensors hold.  ops.py is the only place where a tensor becomes a raw pointer, and the
kernels see addresses and integers: whatever the wrapper lets through is a stray access or silently wrong bytes.

ENTRIES is ONE list of valid small calls, each naming the public functions of aivc_amd.ops it enters through (`covers`:
tests/test_bridge_harness.py checks by introspection that every function that reaches the library is named).  An entry builds a
Case (tests/op_cases.py) from an existing builder where there is one -- a composite builder's case is cut into one call per wrapper,
with that builder's inputs and wants -- and with alt=True a DECOY: the same call on other values of the same shapes and dtypes
(tests/test_gpu_ops_streams.py).  A caller's output (`out=`) is an input here and has entries of its own (`outputs`).

3a, rejection (launches nothing: under bridge.recording every native function but the host-only queries raises Reached): for every
entry, every tensor leaf and each of on_cpu, other_dtype, one_short -- for an output strided too -- the call raises ValueError or
AivcNativeError.  EXEMPT lists the leaves one_short may be accepted for, each with its reason; SIZE_INTEGERS the integers one past
what the tensors hold, each bound taken from what include/aivc_hip*.h states for the entry point.

3b, views (the real library): for every entry and every input leaf, the strided form of the leaf gives the plain call's bits (and the
plain call the oracle's `want`), or the call raises; different bits are never acceptable.
"""
import contextlib
import hashlib
import zlib

import numpy as np
import pytest
import torch

import bridge
import conv_cases as cc
import op_cases as oc
from aivc_amd import abi
from op_cases import Case, eq, on

pytestmark = pytest.mark.gpu


class Entry:
    def __init__(self, name, covers, build, outputs=(), contract=None):
        """build(oracle, golden, alt) -> Case (alt: the decoy); outputs: the leaves that are a caller's output; contract: 'fp32w'
        (version 2 with the size rule lifted, on both sides) or 'bf16x3' where the form needs it"""
        self.name, self.covers, self.build, self.outputs, self.contract = name, tuple(covers), build, tuple(outputs), contract

    def __repr__(self):
        return self.name


@contextlib.contextmanager
def contract_of(entry, oracle):
    from aivc_amd import ops
    if entry.contract is None:
        yield
        return
    prev_h = ops.set_precision(entry.contract)
    prev_o = oracle.set_precision('fp32w') if entry.contract == 'fp32w' else None
    if entry.contract == 'fp32w':
        ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = True
    try:
        yield
    finally:
        ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = False
        ops.set_precision(prev_h)
        if prev_o is not None:
            oracle.set_precision(prev_o)


def shifted(case):
    """the decoy of a case whose builder takes no seed: every float v -> v / 2 + 1 / 4 (positive stays positive, a level in [0, 255]
    stays one), every byte b -> 255 - b; other integer leaves carry a format (packed bounds, CDF rows) and need a builder's decoy"""
    def alt(a):
        if a.dtype.kind == 'f':
            return (a * a.dtype.type(0.5) + a.dtype.type(0.25)).astype(a.dtype)
        assert a.dtype == np.uint8, a.dtype
        return (255 - a).astype(np.uint8)
    return Case(oc.place_all(case.inputs, alt), case.call, None, case.compare)


def part(case, names, call, want, compare=eq, **extra):
    """one wrapper's call cut from a composite builder's case: its inputs `names` (plus extra), its want"""
    inputs = {nm: case.inputs[nm] for nm in names}
    inputs.update(extra)
    return Case(inputs, call, want, compare)


def _eq_pair(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        eq(g, w)


def _item_is(got, want):
    assert got.item() == want


def _is(got, want):
    assert got == want


def _nothing_to_compare(got, want):
    assert tuple(got.shape) == (64,) and got.dtype == torch.int32


# ---- the conv family ---------------------------------------------------------------------------------------------------------------
def _conv_images(o, g, alt):
    c = cc.conv_images_cases(o, 9, 13, 2, True, [('a', 'f')])[0]
    return shifted(c) if alt else c


def _bf16x3(o, g, alt):
    """the first row has no fused GDN: its call does not touch beta and gamma, which are no arguments of it then"""
    c = cc.bf16x3_case(cc.BF16X3_CASES[0], 12 if alt else 11)
    assert cc.BF16X3_CASES[0][8] == 0
    return Case({k: c.inputs[k] for k in ('x', 'w', 'bias')}, c.call, None)


def _pack_images(o, g, alt):
    c = cc.pack_images_cases(o, 9, 13, 2, [('a', 'f3')])[0]
    return shifted(c) if alt else c


CONV_ENTRIES = [
    Entry('conv2d-direct', ['conv2d'], lambda o, g, alt: cc.conv_case(o, cc.CONV_CASES[4], 8 if alt else 7)),
    Entry('conv2d-mfma-tile', ['conv2d'], lambda o, g, alt: cc.mfma_tile_case(o, 8 if alt else 7, 32)),
    Entry('gdn-resident', ['gdn', 'conv2d'], lambda o, g, alt: cc.gdn_resident_case(o, (128, 1, 5, 7, alt, False))),
    Entry('conv2d-thin', ['conv2d'], lambda o, g, alt: cc.thin_walk_case(o, cc.THIN_WALK_CASES[2], 8 if alt else 7)),
    Entry('conv2d-wino-301', ['conv2d'], lambda o, g, alt: cc.wino_case(o, 301, cc.WINO_CASES[1], 8 if alt else 7), contract='fp32w'),
    Entry('conv2d-wino-302', ['conv2d'], lambda o, g, alt: cc.wino_case(o, 302, cc.POLY_CASES[6], 8 if alt else 7), contract='fp32w'),
    Entry('conv2d-wino-303', ['conv2d'], lambda o, g, alt: cc.wino_case(o, 303, cc.TC_CASES[1], 8 if alt else 7), contract='fp32w'),
    Entry('conv2d-fused-gdn', ['conv2d'], lambda o, g, alt: cc.fused_gdn_case(o, cc.FUSED_GDN_CASES[6], 8 if alt else 7)),
    Entry('conv2d-fused-tail', ['conv2d'], lambda o, g, alt: cc.fused_tail_case(o, cc.FUSED_TAIL_CASES[2], 8 if alt else 7)),
    Entry('conv2d-images', ['conv2d'], _conv_images),
    Entry('conv2d-bf16x3', ['conv2d'], _bf16x3, contract='bf16x3'),
    Entry('pack_images', ['pack_images'], _pack_images),
    Entry('pad_channels', ['pad_channels'], lambda o, g, alt: oc.pad_channels_case(o, 8 if alt else 7, (2, 3, 5), 3, 8)),
]
assert cc.FUSED_GDN_CASES[6] == (abi.MODE_CONV, 3, 1, 1, 32, 32, 9, 9, False, False) and cc.FUSED_TAIL_CASES[2][:8] == (3, 1, 64, 64, 128, 1, 9, 5)
assert cc.CONV_IMAGES_CASES[0] == (9, 13, 2)


# ---- frame and pixel ops -----------------------------------------------------------------------------------------------------------
def _to_444(u8, own_out):
    def build(o, g, alt):
        return oc.yuv420_to_444_case(o, oc.yuv_planes(4 if alt else 3, 9, 13), u8, c_store=8, c_off=4, own_out=own_out)
    return build


def _frame_to_yuv420(o, g, alt):
    x, skip, _ = oc.frame_sources(4 if alt else 3, 9, 13)
    return oc.frame_to_yuv420_case(o, x, 9, 13, skip=skip)


def _warp_blend(rows):
    def build(o, g, alt):
        h, w, s = oc.WARP_SHAPES[0][0], oc.WARP_SHAPES[0][1], oc.WARP_SHAPES[0][2]
        return oc.warp_blend_case(o, oc.warp_blend_sources(4 if alt else 3, h, w, s), h, w, abi.FRAME_B, rows=rows)
    return build


def _warp_mode(mode, pad, ac):
    def build(o, g, alt):
        c = oc.warp_modes_case(g('warp_modes'), 0, mode, pad, ac)
        return shifted(c) if alt else c
    return build


FRAME_ENTRIES = [
    Entry('yuv420_to_444-u8', ['yuv420_to_444'], _to_444(True, False)),
    Entry('yuv420_to_444-float', ['yuv420_to_444'], _to_444(False, False)),
    Entry('yuv420_to_444-out', ['yuv420_to_444'], _to_444(True, True), outputs=['out']),
    Entry('frame_to_yuv420', ['frame_to_yuv420'], _frame_to_yuv420),
    Entry('warp', ['warp'], lambda o, g, alt: oc.warp_case(o, 4 if alt else 3, *oc.WARP_SHAPES[0])),
    Entry('warp-bicubic-zeros', ['warp'], _warp_mode('bicubic', 'zeros', False)),
    Entry('warp-nearest-reflection', ['warp'], _warp_mode('nearest', 'reflection', True)),
    Entry('warp_blend', ['warp_blend'], _warp_blend(None)),
    Entry('warp_blend-rows', ['warp_blend'], _warp_blend((2, 5))),
    Entry('downsample2x', ['downsample2x'], lambda o, g, alt: oc.downsample2x_cases(o, 4 if alt else 3, 9, 13)[0]),
]


# ---- latent, entropy, range coder, rate, metrics: one call per wrapper from the composite builders ---------------------------------
def _latent(name):
    def build(o, g, alt):
        c = oc.latent_ops_case(o, 6 if alt else 5)
        w = c.want
        return {
            'hyper_params': lambda: part(c, ['hs'], lambda ops, d: ops.hyper_params(d['hs'], 8, 5, 7), (w['mu'], w['sigma']), _eq_pair),
            'channel_gain': lambda: part(c, ['y', 'gain'], lambda ops, d: ops.channel_gain(d['y'], d['gain']), w['gain']),
            'quantize_center': lambda: part(c, ['y', 'mu', 'gain'], lambda ops, d: ops.quantize_center(d['y'], d['mu'], d['gain']),
                                            (w['q'], w['yh']), _eq_pair),
            'dequantize': lambda: part(c, ['q', 'mu', 'gain'], lambda ops, d: ops.dequantize(d['q'], d['mu'], d['gain']), w['deq']),
            'gdn_reparam': lambda: part(c, ['beta', 'gamma'], lambda ops, d: ops.gdn_reparam(d['beta'], d['gamma'], 1e-3, 2 ** -18, 2 ** -36),
                                        (w['be'], w['ge']), _eq_pair),
        }[name]()
    return build


def _rows(name):
    """the `_rows` gain ops on (3, 5, 7, 6), tests/test_gpu_latent_rows.py's smallest: a row of gains per image == the single-gain op,
    image by image, in the oracle"""
    def build(o, g, alt):
        from test_gpu_latent_rows import make_data
        d = make_data(3, 5, 7, 6)
        if alt:
            d = {'y': d['y'][::-1] + np.float32(0.25), 'mu': d['mu'][::-1] + np.float32(0.25), 'gains': d['gains'][::-1] * np.float32(0.5),
                 'q': (-d['q'][::-1]).astype(np.int16)}
            d = {k: np.ascontiguousarray(v) for k, v in d.items()}
        per = lambda fn: [fn(i) for i in range(3)]  # noqa: E731
        if name == 'channel_gain_rows':
            want = np.concatenate(per(lambda i: o.channel_gain(d['y'][i:i + 1], d['gains'][i])))
            return Case({k: d[k] for k in ('y', 'gains')}, lambda ops, t: ops.channel_gain_rows(t['y'], t['gains']), want)
        if name == 'quantize_center_rows':
            two = per(lambda i: o.quantize_center(d['y'][i:i + 1], d['mu'][i:i + 1], d['gains'][i]))
            want = (np.concatenate([q for q, _ in two]), np.concatenate([yh for _, yh in two]))
            return Case({k: d[k] for k in ('y', 'mu', 'gains')}, lambda ops, t: ops.quantize_center_rows(t['y'], t['mu'], t['gains']), want, _eq_pair)
        want = np.concatenate(per(lambda i: o.dequantize(d['q'][i:i + 1], d['mu'][i:i + 1], d['gains'][i])))
        return Case({k: d[k] for k in ('q', 'mu', 'gains')}, lambda ops, t: ops.dequantize_rows(t['q'], t['mu'], t['gains']), want)
    return build


def _cdf(name):
    def build(o, g, alt):
        c = oc.cdf_case(o, 12 if alt else 11, (1, 5, 7, 8))
        w, maps, npos = c.want, c.maps, c.npos

        def rows_out(ops, d):
            got = ops.laplace_cdf_rows(d['sig'], maps, out=d['out'], row_off=3)
            assert got is d['out']
            return got

        def win_out(ops, d):
            got = ops.laplace_cdf_windows(d['sig'], maps, out=(d['win'], d['sp']), row_off=3)
            assert got[0] is d['win'] and got[1] is d['sp']
            return got

        def into(a, fill):
            """`a` from row 3 of a tensor that ends with it, `fill` in front: what the call must leave"""
            full = np.full((3 + a.shape[0],) + a.shape[1:], fill, a.dtype)
            full[3:3 + a.shape[0]] = a
            return full
        rows_i16, win_i16 = oc._i16(w['rows']), oc._i16(w['win'])
        return {
            'balle_cdf_table': lambda: part(c, ['params'], lambda ops, d: ops.balle_cdf_table(d['params'], want_float=True), (w['t'], w['c']), _eq_pair),
            'laplace_cdf_rows': lambda: part(c, ['sig'], lambda ops, d: ops.laplace_cdf_rows(d['sig'], maps), w['rows']),
            'laplace_cdf_rows-out': lambda: part(c, ['sig'], rows_out, into(rows_i16, 7), out=np.full((npos + 3, abi.CDF_ROW), 7, np.int16)),
            'laplace_cdf_windows': lambda: part(c, ['sig'], lambda ops, d: ops.laplace_cdf_windows(d['sig'], maps), (w['win'], w['sp']), _eq_pair),
            'laplace_cdf_windows-out': lambda: part(c, ['sig'], win_out, (into(win_i16, 7), into(w['sp'], 7)), _eq_pair,
                                                    win=np.full((npos + 3, abi.CDF_WIN), 7, np.int16), sp=np.full(npos + 3, 7, np.float32)),
            'laplace_bounds': lambda: part(c, ['sig', 'q'], lambda ops, d: ops.laplace_bounds(d['sig'], d['q'], maps), w['bounds']),
            'table_bounds': lambda: part(c, ['table', 'qz'], lambda ops, d: ops.table_bounds(d['table'], d['qz']), w['tbounds']),
            'nonzero_flags': lambda: part(c, ['qb'], lambda ops, d: ops.nonzero_flags(d['qb']), w['flags']),
        }[name]()
    return build


def _batch(name):
    def build(o, g, alt):
        shape, maps = oc.FRAME_BATCH_CASES[1]
        c = oc.frame_batch_case(o, 12 if alt else 11, shape, maps)
        n, h, wd, ch = shape
        npix, w, total = h * wd, c.want, c.total
        offs = np.cumsum([0] + [len(m) * npix for m in maps])
        live = [f for f, m in enumerate(maps) if m]

        def packed(per_frame, k=None):
            return np.concatenate([per_frame[f] if k is None else per_frame[f][k] for f in live])

        def windows(ops, d):
            got = ops.laplace_cdf_windows_batch(d['sig'], maps, (d['win'], d['sp']))
            assert got[0] == [int(v) for v in offs[:-1]]
            return d['win'][:total], d['sp'][:total]
        return {
            'laplace_bounds_batch': lambda: part(c, ['sig', 'q'], lambda ops, d: ops.laplace_bounds_batch(d['sig'], d['q'], maps)[0][:total],
                                                 packed(w['b'])),
            'laplace_cdf_windows_batch-out': lambda: part(c, ['sig'], windows, (packed(w['w'], 0), packed(w['w'], 1)), _eq_pair,
                                                          win=np.full((total, abi.CDF_WIN), 7, np.int16), sp=np.full(total, 7, np.float32)),
            'table_bounds_batch': lambda: part(c, ['table', 'q'], lambda ops, d: ops.table_bounds_batch(d['table'], d['q']), w['tb']),
            'scatter_symbols_batch': lambda: part(c, ['sym'], lambda ops, d: ops.scatter_symbols_batch(d['sym'], maps, n, npix, ch).view(shape), w['q']),
            'scatter_symbols': lambda: Case({'sym': c.inputs['syms'][0]}, lambda ops, d: ops.scatter_symbols(d['sym'], npix, ch, maps[0]).view(h, wd, ch),
                                            w['q'][0]),
        }[name]()
    return build


def _range_coder(windows):
    """1000 symbols decoded from full CDF rows, or from windows + sigma per position; the decoy: the rows of another scale (the call
    decodes the REAL case's payload either way)"""
    def build(o, g, alt):
        c = oc.range_coder_case(o, 1000, 0.1 if alt else 0.05, windows=True)
        ref = oc.range_coder_case(o, 1000, 0.05, windows=True) if alt else c
        payload = _payload(ref)
        if not windows:
            return Case({'rows': c.inputs['rows']}, lambda ops, d: ops.range_decode([payload], d['rows'], [0], [1000], [0]), [ref.want], _eq_pair)
        return Case({'win': c.inputs['win'], 'sp': c.inputs['sp']},
                    lambda ops, d: ops.range_decode([payload], d['win'], [0], [1000], [0], sigma_pos=d['sp']), [ref.want], _eq_pair)
    return build


def _payload(case):
    """the payload a range_coder_case / range_coder_pmf_case decodes (its call's closure holds it)"""
    return dict(zip(case.call.__code__.co_freevars, case.call.__closure__))['payload'].cell_contents


def _range_encode(o, g, alt):
    """-> the stream's bytes (what lies behind them in the output's capacity is not a result)"""
    c = oc.range_encode_case(o, 8 if alt else 7, [64], 0, 65, False)
    return Case({'bounds': c.inputs['streams'][0]}, lambda ops, d: oc.stream_bytes(*ops.range_encode([d['bounds']])), c.want, _is)


def _pmf_decode(o, g, alt):
    c = oc.range_coder_pmf_case(o, 5)
    if alt:  # other tables of the same shape (the call decodes the real case's payload)
        return Case({'table': oc.range_coder_pmf_case(o, 6).inputs['table']}, None, None)
    payload, n = _payload(c), c.qz.size
    return Case({'table': c.inputs['table']}, lambda ops, d: ops.range_decode([payload], d['table'], [0], [n], [42])[0], c.want)


def _bounds_rate(own_out):
    def build(o, g, alt):
        c = oc.bounds_rate_case(o, 8 if alt else 7, 1000)
        if not own_out:
            return c

        def call(ops, d):
            got = ops.bounds_rate(d['b'], out=d['out'])
            assert got is d['out']
            return got
        return Case({'b': c.inputs['b'], 'out': np.full(1, 7.0, np.float64)}, call, c.want, c.compare)
    return build


def _rate(name):
    def build(o, g, alt):
        c = oc.rate_estimates_case(o, 8 if alt else 7, (2, 6, 5, 7))
        w = c.want
        return {
            'laplace_prob': lambda: part(c, ['y', 'mu', 'sigma'], lambda ops, d: ops.laplace_prob(d['y'], d['mu'], d['sigma']), w['p_mu']),
            'table_prob': lambda: part(c, ['y', 'cdf'], lambda ops, d: ops.table_prob(d['y'], d['cdf']), w['p_z']),
            'rate_bits': lambda: part(c, ['p_zero'], lambda ops, d: ops.rate_bits(d['p_zero'], 2.0 ** -16, 1.0)[0], w['rate']),
        }[name]()
    return build


def _metrics(name):
    def build(o, g, alt):
        from oracle import metrics
        c = oc.metrics_case(o, 9, 13, 5)
        w = c.want
        win = metrics.window_clic(5, 5 * 1.5 / 11)
        c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
        case = {
            'ssim_means': lambda: part(c, ['a', 'b'], lambda ops, d: ops.ssim_means(d['a'], d['b'], win, c1, c2), w['ssim'],
                                       lambda got, want: np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-12)),
            'pool2x2': lambda: part(c, ['a'], lambda ops, d: ops.pool2x2(d['a'], 0), w['pool0']),
            'sq_err': lambda: part(c, ['ia', 'ib'], lambda ops, d: ops.sq_err(d['ia'], d['ib']), w['se_int'], _item_is),
        }[name]()
        if alt:
            case = shifted(case) if name != 'sq_err' else Case({k: 255 - v for k, v in case.inputs.items()}, case.call, None)
        return case
    return build


def _detmath(o, g, alt):
    a = np.random.default_rng(8 if alt else 7).uniform(-20, 20, 300).astype(np.float32)
    return oc.detmath_case(o, abi.DETMATH_EXPF, a)


def _gain_interp(o, g, alt):
    return oc.gain_interp_case(o, 8 if alt else 7, 8, 0.3)


LATENT_ENTRIES = (
    [Entry(nm, [nm], _latent(nm)) for nm in ('hyper_params', 'channel_gain', 'quantize_center', 'dequantize', 'gdn_reparam')]
    + [Entry(nm, [nm], _rows(nm)) for nm in ('channel_gain_rows', 'quantize_center_rows', 'dequantize_rows')]
    + [Entry('gain_interp', ['gain_interp'], _gain_interp), Entry('detmath_eval', ['detmath_eval'], _detmath)]
    + [Entry(nm, [nm.split('-')[0]], _cdf(nm), outputs={'laplace_cdf_rows-out': ['out'], 'laplace_cdf_windows-out': ['win', 'sp']}.get(nm, ()))
       for nm in ('balle_cdf_table', 'laplace_cdf_rows', 'laplace_cdf_rows-out', 'laplace_cdf_windows', 'laplace_cdf_windows-out',
                  'laplace_bounds', 'table_bounds', 'nonzero_flags')]
    + [Entry(nm, [nm.split('-')[0]] + (['frame_maps_to_device'] if 'batch' in nm else []), _batch(nm),
             outputs=['win', 'sp'] if nm.endswith('-out') else ())
       for nm in ('laplace_bounds_batch', 'laplace_cdf_windows_batch-out', 'table_bounds_batch', 'scatter_symbols_batch', 'scatter_symbols')]
    + [Entry('range_encode', ['range_encode'], _range_encode),
       Entry('range_decode', ['range_decode'], _range_coder(False)),
       Entry('range_decode-windows', ['range_decode'], _range_coder(True)),
       Entry('range_decode-pmf', ['range_decode'], _pmf_decode),
       Entry('bounds_rate', ['bounds_rate'], _bounds_rate(False)),
       Entry('bounds_rate-out', ['bounds_rate'], _bounds_rate(True), outputs=['out'])]
    + [Entry(nm, [nm], _rate(nm)) for nm in ('laplace_prob', 'table_prob', 'rate_bits')]
    + [Entry(nm, [nm], _metrics(nm)) for nm in ('ssim_means', 'pool2x2', 'sq_err')]
)


# ---- wrappers without a builder: a few lines each, on the smallest shapes of the op's own test -------------------------------------
def _rng(alt, seed=20):
    return np.random.default_rng(seed + (1 if alt else 0))


def _rgb8(o, g, alt):
    """(2, 5, 3) pixels, tests/test_gpu_color.py's odd shape: Pillow's convert('YCbCr'), chroma from sample (2i, 2j)"""
    from test_gpu_color import pil_ycbcr
    rgb = _rng(alt).integers(0, 256, (2, 5, 3, 3), dtype=np.uint8)
    ycc = pil_ycbcr(rgb)
    want = (ycc[..., 0], ycc[:, 0:4:2, 0:2:2, 1], ycc[:, 0:4:2, 0:2:2, 2])
    return Case({'rgb': rgb}, lambda ops, d: ops.rgb8_to_yuv420u8(d['rgb']), tuple(np.ascontiguousarray(a) for a in want), _eq_pair)


def _yuv8(o, g, alt):
    from test_gpu_color import pil_rgb, upsampled
    y, u, v = oc.yuv_planes(21 if alt else 20, 5, 3)
    want = pil_rgb(np.stack([y, upsampled(u, 5, 3), upsampled(v, 5, 3)], -1))
    return Case({'y': y, 'u': u, 'v': v}, lambda ops, d: ops.yuv8_to_rgb8(d['y'], d['u'], d['v']), want)


def _md5(o, g, alt):
    m = _rng(alt).integers(0, 256, (5, 7, 9), dtype=np.uint8)
    want = np.stack([np.frombuffer(hashlib.md5(p.tobytes()).digest(), np.uint8) for p in m])
    return Case({'planes': m}, lambda ops, d: ops.md5_planes(d['planes']), want)


def _pair_sad(o, g, alt):
    planes = [_rng(alt, 30 + i).integers(0, 256, 65, dtype=np.uint8) for i in range(3)]
    want = np.array([np.abs(planes[i + 1].astype(np.int64) - planes[i]).sum() for i in range(2)], np.int64)
    return Case({'planes': planes}, lambda ops, d: ops.pair_sad_u8(d['planes']), want)


def _resize(o, g, alt):
    import resize_cases as rc
    planes = [_rng(alt, 40 + i).integers(0, 256, (9, 13), dtype=np.uint8) for i in range(2)]
    want = np.stack([rc.pil_resize(p, 5, 17, 'bicubic') for p in planes])
    return Case({'planes': planes}, lambda ops, d: ops.resize_u8(d['planes'], 5, 17, 'bicubic'), want)


def _raw_read(o, g, alt):
    import rawvideo_cases as rvc
    rng, name, w, h = _rng(alt), 'yuv422p10le', 5, 3
    frames = [rvc.make_frame(name, w, h, rng) for _ in range(2)]
    want = tuple(np.stack(p) for p in zip(*(rvc.ingest(f, name, w, h) for f in frames)))
    offs = [0, frames[0].size]  # (tight: a blob one byte short no longer holds the second frame)
    return Case({'blob': np.concatenate(frames)}, lambda ops, d: ops.raw_to_yuv420u8(d['blob'], offs, name, w, h), want, _eq_pair)


def _raw_write(o, g, alt):
    import rawvideo_cases as rvc
    y, u, v = oc.yuv_planes(21 if alt else 20, 3, 5)
    want = np.stack([np.concatenate([np.frombuffer(b'FRAME\n', np.uint8), rvc.export(y[f], u[f], v[f], 'nv12')]) for f in range(2)])
    return Case({'y': y, 'u': u, 'v': v}, lambda ops, d: ops.yuv420u8_to_raw(d['y'], d['u'], d['v'], 'nv12', b'FRAME\n'), want)


def _png_picture(alt, n=2):
    import png_cases as pcs
    return np.stack([pcs.random_picture(5, 7, 3, 50 + 2 * i + (1 if alt else 0)) for i in range(n)])


def _png_encode(o, g, alt):
    import png_cases as pcs
    pix = _png_picture(alt)

    def compare(streams, want):
        for z, p in zip(streams, want):  # a zlib stream of the filtered rows of this picture, whichever filters won
            f = np.frombuffer(zlib.decompress(z), np.uint8).reshape(5, 1 + 7 * 3)
            np.testing.assert_array_equal(f, pcs.filter_rows(p, f[:, 0]))
    return Case({'pix': pix}, lambda ops, d: ops.png_encode(d['pix']), pix, compare)


def _png_unfilter(o, g, alt):
    import png_cases as pcs
    pix = _png_picture(alt)
    filt = [pcs.filter_rows(p, np.arange(5) % 5).reshape(-1) for p in pix]
    return Case({'filt': filt}, lambda ops, d: ops.png_unfilter(d['filt'], [(5, 7, 3)] * 2), list(pix), _eq_pair)


def _inflate(o, g, alt):
    """no tensor goes in: the streams are host bytes (and so there is no decoy to overwrite); the launch and the stream are tested"""
    import png_read_cases as prc
    data = [prc.markov_text(300, seed=3), prc.markov_text(200, seed=4)]
    return Case({}, lambda ops, d: ops.inflate([zlib.compress(b) for b in data], [len(b) for b in data], torch.device('cuda', 0)),
                [np.frombuffer(b, np.uint8) for b in data], _eq_pair)


def _frame_sse(o, g, alt):
    src, rec = (dict(zip('yuv', oc.yuv_planes(s + (10 if alt else 0), 5, 3, n=3))) for s in (60, 61))
    want = np.array([[((src[k][f].astype(np.int64) - rec[k][f]) ** 2).sum() for k in 'yuv'] for f in range(3)], np.int64)
    return Case({'src': src, 'rec': rec}, lambda ops, d: ops.frame_sse_u8(d['src'], d['rec']), want)


def _frame_aux(o, g, alt):
    from test_gpu_quality_stats import aux_inputs, check_against_fsum
    d = aux_inputs(_rng(alt), 3, 5, 3, 4, 3)
    return Case(d, lambda ops, t: ops.frame_aux_stats(t['alpha'], t['beta'], t['warping'], t['code']), d,
                lambda got, want: check_against_fsum(got.cpu().numpy(), want, 3))


def _hold_lds(own_out):
    def build(o, g, alt):
        """(the chain ends are the diagnostic's own business: the shape and type of what comes back is all there is to compare)"""
        if own_out:
            return Case({'out': np.full(64, 8 if alt else 7, np.int32)}, lambda ops, d: ops.diag_hold_lds(1024, 64, out=d['out']), 0, _nothing_to_compare)
        return Case({}, lambda ops, d: ops.diag_hold_lds(1024, 64), 0, _nothing_to_compare)
    return build


def _selfcheck(o, g, alt):
    return Case({}, lambda ops, d: ops.selfcheck_gdn_math(n_div_pairs=1 << 12, seed=3), (0, 0), _is)


def _slab(o, g, alt):
    """a row slab of a map the whole of which takes the Winograd chain: conv2d asks slab_contract which version the slab computes in"""
    c = cc.wino_case(o, 301, cc.WINO_CASES[0], 8 if alt else 7)
    return Case(c.inputs, lambda ops, d: c.call(ops, d, frame_h=8), c.want, c.compare)


OTHER_ENTRIES = [
    Entry('rgb8_to_yuv420u8', ['rgb8_to_yuv420u8'], _rgb8), Entry('yuv8_to_rgb8', ['yuv8_to_rgb8'], _yuv8),
    Entry('md5_planes', ['md5_planes'], _md5), Entry('pair_sad_u8', ['pair_sad_u8'], _pair_sad), Entry('resize_u8', ['resize_u8'], _resize),
    Entry('raw_to_yuv420u8', ['raw_to_yuv420u8'], _raw_read), Entry('yuv420u8_to_raw', ['yuv420u8_to_raw'], _raw_write),
    Entry('png_encode', ['png_encode'], _png_encode), Entry('png_unfilter', ['png_unfilter', 'png_unfilter_launch'], _png_unfilter),
    Entry('inflate', ['inflate', 'inflate_launch'], _inflate),
    Entry('frame_sse_u8', ['frame_sse_u8'], _frame_sse), Entry('frame_aux_stats', ['frame_aux_stats'], _frame_aux),
    Entry('diag_hold_lds', ['diag_hold_lds'], _hold_lds(False)), Entry('diag_hold_lds-out', ['diag_hold_lds'], _hold_lds(True), outputs=['out']),
    Entry('selfcheck_gdn_math', ['selfcheck_gdn_math'], _selfcheck),
    Entry('conv2d-slab', ['conv2d', 'slab_contract'], _slab, contract='fp32w'),
]

ENTRIES = CONV_ENTRIES + FRAME_ENTRIES + LATENT_ENTRIES + OTHER_ENTRIES
assert len({e.name for e in ENTRIES}) == len(ENTRIES)

# one_short may be ACCEPTED for these leaves only: no other argument and no integer of the call depends on the leaf's size, so the
# shortened tensor is a valid (other) call.  At most one leaf per function.
EXEMPT = {
    ('pad_channels', 'x'): 'any [..., c_in] with c_in <= c_out pads; c_in is read from x itself',
    ('detmath_eval', 'a'): 'a unary function of n arguments, n read from a itself',
    ('md5_planes', 'planes'): 'one message of any length',
    ('range_encode', 'bounds'): 'a stream of any length; the capacity of its output is computed from it',
    ('bounds_rate', 'b'): 'any number of bounds',
    ('bounds_rate-out', 'b'): 'any number of bounds (the same leaf of the same function)',
    ('rate_bits', 'p_zero'): 'any number of probabilities, the rates come back in its shape',
}
# an output that strided() has no form of
STRIDED_OUTPUT_EXEMPT = {('bounds_rate-out', 'out'): 'one element: torch calls it contiguous whatever its strides'}

by_name = {e.name: e for e in ENTRIES}
_exempt_leaves = {(by_name[nm].covers[0], leaf) for nm, leaf in EXEMPT}
assert len({fn for fn, _ in _exempt_leaves}) == len(_exempt_leaves), 'at most one exempt leaf per function'


def _ids(entries):
    return [e.name for e in entries]


def _device_case(entry, oracle, golden, cuda, change=None, k=None):
    from aivc_amd import ops
    case = entry.build(oracle, golden, False)
    put = on(cuda) if change is None else bridge.Target(on(cuda), k, change)
    return ops, case, case.place(put), put


@pytest.mark.parametrize('defect', sorted(bridge.DEFECTS))
@pytest.mark.parametrize('entry', ENTRIES, ids=_ids(ENTRIES))
def test_defective_tensor_is_rejected_before_the_library(entry, defect, cuda, oracle, golden):
    from aivc_amd import ops
    with contract_of(entry, oracle):
        case = entry.build(oracle, golden, False)
        failures = []
        for k, (leaf, _) in enumerate(bridge.leaves(case.inputs)):
            if defect == 'one_short' and (entry.name, leaf) in EXEMPT:
                continue
            put = bridge.Target(on(cuda), k, bridge.DEFECTS[defect])
            d = case.place(put)
            assert put.hit
            try:
                with bridge.recording(ops), bridge.raises_before_the_library('%s, %s %s' % (entry.name, leaf, defect)):
                    case.call(ops, d)
            except AssertionError as e:
                failures.append(str(e))
        assert not failures, '\n'.join(failures)


OUTPUT_ENTRIES = [e for e in ENTRIES if e.outputs]


@pytest.mark.parametrize('entry', OUTPUT_ENTRIES, ids=_ids(OUTPUT_ENTRIES))
def test_strided_output_is_rejected(entry, cuda, oracle, golden):
    from aivc_amd import ops
    case = entry.build(oracle, golden, False)
    names = [leaf for leaf, _ in bridge.leaves(case.inputs)]
    assert set(entry.outputs) <= set(names)
    for leaf in entry.outputs:
        if (entry.name, leaf) in STRIDED_OUTPUT_EXEMPT:
            continue
        put = bridge.Target(on(cuda), names.index(leaf), bridge.strided)
        d = case.place(put)
        with bridge.recording(ops), bridge.raises_before_the_library('%s, strided %s' % (entry.name, leaf)):
            case.call(ops, d)


def test_plain_call_reaches_the_library(cuda, oracle, golden):
    """the recorder's stand-in is what stops a call: every entry's PLAIN call gets as far as the library under it (so a rejection
    above is the wrapper's, not the harness's), and launches nothing"""
    from aivc_amd import ops
    for entry in ENTRIES:
        with contract_of(entry, oracle):
            case = entry.build(oracle, golden, False)
            d = case.place(on(cuda))
            with bridge.recording(ops), pytest.raises(bridge.Reached):
                case.call(ops, d)


# (entry, how the call is made with the integer one past what the tensors hold; the bound as the header states it)
def _si(name, call, bound):
    return pytest.param(name, call, id='%s: %s' % (name, bound))


SIZE_INTEGERS = [
    _si('frame_to_yuv420', lambda ops, d: ops.frame_to_yuv420(d['x'], 9 + 3 + 1, 13), 'h <= hx (aivc_frame_to_yuv420: hx >= h)'),
    _si('frame_to_yuv420', lambda ops, d: ops.frame_to_yuv420(d['x'], 9, 13 + 2 + 1), 'w <= wx (wx >= w)'),
    _si('downsample2x', lambda ops, d: ops.downsample2x(d['x'], 3, 4), 'ch0 + nch <= c (channel ch0 + j of x [n][h][w][c])'),
    _si('hyper_params', lambda ops, d: ops.hyper_params(d['hs'], 8, 7, 7), 'h <= hh (crop to [h][w])'),
    _si('hyper_params', lambda ops, d: ops.hyper_params(d['hs'], 8, 5, 10), 'w <= wh'),
    _si('warp_blend-rows', lambda ops, d: ops.warp_blend(d['mof'], d['prev'], d['next'], 9, 13, abi.FRAME_B, rows=(2, 6)), 'rows <= hm'),
    _si('warp_blend-rows', lambda ops, d: ops.warp_blend(d['mof'][:, :5], d['prev'], d['next'], 9, 13, abi.FRAME_B, rows=(5, 5)),
        'row0 + rows <= h'),
    _si('laplace_cdf_rows-out', lambda ops, d: ops.laplace_cdf_rows(d['sig'], [0, 2, 3, 7], out=d['out'], row_off=4),
        'row_off + n_maps * npix rows of `rows`'),
    _si('laplace_cdf_windows-out', lambda ops, d: ops.laplace_cdf_windows(d['sig'], [0, 2, 3, 7], out=(d['win'], d['sp']), row_off=4),
        'row_off + n_maps * npix positions of win / sigma_pos'),
    _si('laplace_cdf_rows', lambda ops, d: ops.laplace_cdf_rows(d['sig'], [0, 2, 3, 8]), 'maps.idx[m] < c'),
    _si('laplace_cdf_windows', lambda ops, d: ops.laplace_cdf_windows(d['sig'], [0, 2, 3, 8]), 'maps.idx[m] < c'),
    _si('laplace_bounds', lambda ops, d: ops.laplace_bounds(d['sig'], d['q'], [8]), 'maps.idx[m] < c'),
    _si('yuv420_to_444-out', lambda ops, d: ops.yuv420_to_444(d['y'], d['u'], d['v'], c_store=8, c_off=6, out=d['out']),
        'c_off + 3 <= c_store (writes channels c_off..c_off+2)'),
    _si('range_decode', lambda ops, d: ops.range_decode([b'\0' * 8], d['rows'], [1], [1000], [0]), 'row_off + n_sym <= rows'),
    _si('range_decode', lambda ops, d: ops.range_decode([b'\0' * 8], d['rows'], [0], [1001], [0]), 'row_off + n_sym <= rows'),
    _si('range_decode-pmf', lambda ops, d: ops.range_decode([b'\0' * 8], d['table'], [0], [42 * 5 + 1], [42]), 'row_off + ceil(n_sym / plane) <= rows'),
]


@pytest.mark.parametrize('name,call,', SIZE_INTEGERS)
def test_size_integer_past_the_tensors_is_rejected(name, call, cuda, oracle, golden):
    from aivc_amd import ops
    case = by_name[name].build(oracle, golden, False)
    d = case.place(on(cuda))
    with bridge.recording(ops), bridge.raises_before_the_library(name):
        call(ops, d)


# ---- 3b ----------------------------------------------------------------------------------------------------------------------------
def _bits(got):
    """a result of any nesting -> [numpy arrays / host values], for a bit-for-bit comparison of two runs of one call"""
    if isinstance(got, torch.Tensor):
        return [got.cpu().numpy()]
    if isinstance(got, dict):
        return [a for k in sorted(got) for a in _bits(got[k])]
    if isinstance(got, (list, tuple)):
        return [a for v in got for a in _bits(v)]
    return [got]


def same_bits(a, b, what):
    xs, ys = _bits(a), _bits(b)
    assert len(xs) == len(ys), what
    for x, y in zip(xs, ys):
        if isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), '%s: different bits' % what
        else:
            assert x == y, '%s: %r != %r' % (what, x, y)


@pytest.mark.parametrize('entry', ENTRIES, ids=_ids(ENTRIES))
def test_strided_input_gives_the_plain_bits_or_raises(entry, cuda, oracle, golden):
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    with contract_of(entry, oracle):
        case = entry.build(oracle, golden, False)
        plain = case.call(ops, case.place(on(cuda)))
        if case.want is not None:
            case.compare(plain, case.want)
        failures = []
        for k, (leaf, a) in enumerate(bridge.leaves(case.inputs)):
            if leaf in entry.outputs or a.size <= 1:  # (a tensor of one element has no strided form)
                continue
            d = case.place(bridge.Target(on(cuda), k, bridge.strided))
            try:
                got = case.call(ops, d)
            except (ValueError, AivcNativeError):
                continue
            try:
                same_bits(got, plain, '%s, strided %s' % (entry.name, leaf))
            except AssertionError as e:
                failures.append(str(e))
        torch.cuda.synchronize()
        assert not failures, '\n'.join(failures)
