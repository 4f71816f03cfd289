"""The cases of the GPU op tests, each stated once: what tests/test_gpu_ops.py, test_gpu_metrics.py, test_gpu_warp_modes.py (plain
device tensors) and tests/test_gpu_memory_discipline.py (every buffer an arena of tests/guarded.py) run.  The conv family is in
tests/conv_cases.py.  Not a test module.

A builder takes what a test passes (a table row or explicit parameters, a seed, the `oracle` fixture) and returns a Case:

  inputs    {name: numpy array | None | dict of planes | list of these}: the host-side statement of the case
  call      call(ops, d, **kw): the ops call(s) from the PLACED inputs d (same keys, device tensors)
  want      the expected result: the CPU oracle's, a reference-run fixture, or None until the test supplies it
  compare   compare(result, want) with the case's bound: bit exact (eq) unless the builder says otherwise
  (further keyword arguments of Case are plain facts about the case, kept as attributes)

A builder never makes a device tensor.  The test hands run() a placer, numpy array -> device tensor: on(dev) for a plain tensor,
lambda a: guarded(a, dev, fill) for an arena; so `case.check(case.run(ops, place))` is the whole body of most tests.  Where a seed
is asked for, a numpy Generator may be passed instead (default_rng hands it back): a test that draws several cases from one
stream passes its generator on."""
import numpy as np
import torch

from aivc_amd import abi
from numeric_regimes import assert_bits
from warp_modes_cases import BICUBIC_REFERENCE_DEVIATION, case_key, left_out


BICUBIC_ATOL = 4 * BICUBIC_REFERENCE_DEVIATION  # (derived in the docstring of tests/test_gpu_warp_modes.py)


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def on(dev):
    return lambda a: T(a, dev)


def eq(a_gpu, b_np):
    a = a_gpu.cpu().numpy()
    if isinstance(b_np, torch.Tensor):
        b_np = b_np.cpu().numpy()
    if a.dtype == np.int16 and b_np.dtype == np.uint16:
        a = a.view(np.uint16)
    if a.dtype == np.int32 and b_np.dtype == np.uint32:
        a = a.view(np.uint32)
    assert a.shape == b_np.shape
    if a.dtype.kind == 'f' and a.dtype == b_np.dtype:  # bit exact means bits: +0 is not -0, a NaN matches a NaN (assert_bits names the first difference)
        assert_bits(a, b_np)
    else:
        np.testing.assert_array_equal(a, b_np)


def eq_all(got, want):
    """dicts of results: the same keys, every entry bit exact"""
    assert set(got) == set(want), (sorted(got), sorted(want))
    for k in want:
        eq(got[k], want[k])


def place_all(v, put):
    if v is None:
        return None
    if isinstance(v, dict):
        return {k: place_all(x, put) for k, x in v.items()}
    if isinstance(v, (list, tuple)):
        return [place_all(x, put) for x in v]
    return put(v)


class Case:
    def __init__(self, inputs, call, want, compare=eq, **facts):
        self.inputs, self.call, self.want, self.compare = inputs, call, want, compare
        self.__dict__.update(facts)

    def place(self, put):
        return place_all(self.inputs, put)

    def run(self, ops, put, **kw):
        return self.call(ops, self.place(put), **kw)

    def check(self, result):
        self.compare(result, self.want)
        return result


def profiled(fn):
    """fn() with ops.PROFILE on -> (result, [variant code of every conv launch])"""
    from aivc_amd import ops
    ops.PROFILE = []
    try:
        y = fn()
        torch.cuda.synchronize()
        codes = [rec[0] for rec in ops.PROFILE]
    finally:
        ops.PROFILE = None
    return y, codes


def _i16(a):
    return np.ascontiguousarray(a).view(np.int16)


def _i32(a):
    return np.ascontiguousarray(a).view(np.int32)


# ---- pixel operations ------------------------------------------------------------------------------------------------------------
FRAME_SIZES = [(9, 13), (10, 14), (16, 16), (1, 1), (6, 1028)]  # h, w
WARP_SHAPES = [(9, 13, 3.0), (8, 8, 30.0), (5, 1, 2.0)]  # h, w, scale of the flow
AUX = ('pred', 'skip', 'x_warp', 'alpha', 'beta')


def yuv_planes(seed, h, w, n=2):
    """8-bit 4:2:0 planes y, u, v (chroma ceil-sized)"""
    rng = np.random.default_rng(seed)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    return tuple(rng.integers(0, 256, (n, hh, ww), dtype=np.uint8) for hh, ww in ((h, w), (hc, wc), (hc, wc)))


def yuv420_to_444_case(oracle, planes, u8, c_store=4, c_off=0, own_out=False):
    """bytes or floats in [0, 1] into channels c_off .. c_off + 3 of c_store stored ones, of a fresh tensor or of the caller's
    (filled with 7: its other channels stay)"""
    y, u, v = planes if u8 else (a.astype(np.float32) / np.float32(255) for a in planes)
    n, h, w = y.shape
    base = np.full((n, h, w, c_store), 7.0, np.float32) if own_out else np.zeros((n, h, w, c_store), np.float32)
    want = (oracle.yuv420u8_to_444 if u8 else oracle.yuv420_to_444)(y, u, v, c_store=c_store, c_off=c_off, out=base.copy())
    if c_store >= c_off + 4:
        want[..., c_off + 3] = 0.0  # (the image's zero pad channel: ops asks the kernel to write it)
    untouched = [c for c in range(c_store) if not c_off <= c < c_off + 4]
    assert np.array_equal(want[..., untouched], base[..., untouched])

    def call(ops, d):
        got = ops.yuv420_to_444(d['y'], d['u'], d['v'], c_store=c_store, c_off=c_off, out=d['out'])
        assert d['out'] is None or got is d['out']
        return got
    return Case({'y': y, 'u': u, 'v': v, 'out': base if own_out else None}, call, want)


def frame_sources(seed, h, w):
    """a synthesis output of 4 stored channels with margins, the skip frame, and the 3-channel even-pitch hand-over of the codec"""
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((2, h + 3, w + 2, 4), dtype=np.float32) * 0.4 + 0.5).astype(np.float32)
    skip = (rng.standard_normal((2, h, w, 4), dtype=np.float32) * 0.1).astype(np.float32)
    return x, skip, np.ascontiguousarray(x[:, :, :w + 2 - (w & 1), :3])


def frame_to_yuv420_case(oracle, src, h, w, skip=None, want_float=True):
    def call(ops, d):
        return ops.frame_to_yuv420(d['x'], h, w, skip=d['skip'], want_float=want_float)

    def compare(got, want):
        (gf, gb), (rf, rb) = got, want
        for a, b in zip(gb, rb):
            eq(a, b)
        if want_float:
            for a, b in zip(gf, rf):
                eq(a, b)
        else:
            assert gf == (None, None, None)
    return Case({'x': src, 'skip': skip}, call, oracle.frame_to_yuv420(src, h, w, skip=skip), compare)


def warp_case(oracle, seed, h, w, s):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, h, w, 4), dtype=np.float32)
    flow = (rng.standard_normal((2, h, w, 2), dtype=np.float32) * s).astype(np.float32)
    return Case({'x': x, 'flow': flow}, lambda ops, d: ops.warp(d['x'], d['flow']), oracle.warp(x, flow))


def warp_modes_case(g, s, mode, pad, ac):
    """a sampling mode against the reference-run fixture g (tests/golden/warp_modes.npz): NHWC in, the result compared as NCHW
    with the bounds of tests/test_gpu_warp_modes.py's docstring; what the mask zeroes is zero, not small"""
    key = case_key(s, mode, pad, ac)
    want = g['y_' + key]
    keep = np.broadcast_to(~left_out(g, s, mode, pad, ac)[:, None], want.shape)
    gone = np.broadcast_to((g['m_' + key] < 0.9998)[:, None], want.shape)

    def compare(y, want):
        got = y.cpu().numpy()
        assert got.shape == want.shape
        if mode == 'bicubic':
            np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=BICUBIC_ATOL)
        else:
            np.testing.assert_allclose(got[keep], want[keep], rtol=1e-5, atol=2e-6)
        assert (got[gone] == 0).all()
    inputs = {nm: np.ascontiguousarray(np.transpose(g['%s_%d' % (nm, s)], (0, 2, 3, 1))) for nm in ('x', 'flow')}
    return Case(inputs, lambda ops, d: ops.warp(d['x'], d['flow'], mode, pad, ac).permute(0, 3, 1, 2), want, compare, keep=keep)


def warp_blend_sources(seed, h, w, s):
    """MOFNet output with margins (8 channels, the flows scaled by s), previous and next reference frame"""
    rng = np.random.default_rng(seed)
    mof = rng.standard_normal((2, h + 2, w + 1, 8), dtype=np.float32)
    mof[..., 2:6] *= np.float32(s)
    return mof, rng.random((2, h, w, 4), dtype=np.float32), rng.random((2, h, w, 4), dtype=np.float32)


def warp_blend_case(oracle, sources, h, w, ft, general=False, want_aux=True, rows=None):
    """frame type ft on the 16-byte fast path (4 / 4 / 8 channels) or the general kernel (3 / 3 / 7); rows = (row0, n_rows): that
    band of the MOFNet output in, whole reference frames in, the band's rows out == the rows of the oracle's whole frame"""
    mof, prev, nxt = sources
    co = 4
    if general:
        mof, prev, nxt, co = np.ascontiguousarray(mof[..., :7]), prev[..., :3].copy(), nxt[..., :3].copy(), 3
    want = oracle.warp_blend(mof, prev, nxt, h, w, ft, co=co)
    if rows is not None:
        whole, mof = want, np.ascontiguousarray(mof[:, rows[0]:rows[0] + rows[1]])
        want = oracle.warp_blend(mof, prev, nxt, h, w, ft, co=co, rows=rows)
        for kk in AUX:
            np.testing.assert_array_equal(want[kk], whole[kk][:, rows[0]:rows[0] + rows[1]])
    keys = AUX if want_aux else AUX[:2]

    def compare(g, want):
        for kk in keys:
            eq(g[kk], want[kk])
        assert all(g[kk] is None for kk in AUX if kk not in keys)
    return Case({'mof': mof, 'prev': prev, 'next': nxt},
                lambda ops, d: ops.warp_blend(d['mof'], d['prev'], d['next'], h, w, ft, co=co, want_aux=want_aux, rows=rows), want, compare)


def downsample2x_cases(oracle, seed, h, w):
    """2x2 means of channel ranges that do not start at 0, planar output; an odd side drops its last row / column"""
    x = np.random.default_rng(seed).standard_normal((2, h, w, 6), dtype=np.float32)
    cases = []
    for ch0, nch in ((1, 2), (3, 3), (0, 6), (5, 1)):
        want = oracle.downsample2x(x, ch0, nch)
        assert want.shape == (2, nch, h // 2, w // 2)
        cases.append(Case({'x': x}, lambda ops, d, ch0=ch0, nch=nch: ops.downsample2x(d['x'], ch0, nch), want))
    return cases


def gain_interp_case(oracle, seed, n, lam):
    rng = np.random.default_rng(seed)
    g_r, g_t = (np.exp(rng.standard_normal(n)).astype(np.float32) for _ in range(2))
    return Case({'g_r': g_r, 'g_t': g_t}, lambda ops, d: ops.gain_interp(d['g_r'], d['g_t'], lam), oracle.gain_interp(g_r, g_t, lam))


def pad_channels_case(oracle, seed, shape, c_in, c_out):
    x = np.random.default_rng(seed).standard_normal(shape + (c_in,), dtype=np.float32)
    want = oracle.pad_channels(x, c_out)
    assert want.shape == shape + (c_out,) and np.array_equal(want[..., :c_in], x) and not want[..., c_in:].any()
    return Case({'x': x}, lambda ops, d: ops.pad_channels(d['x'], c_out), want)


def latent_ops_case(oracle, seed):
    """hyper_params, channel_gain, quantize_center with and without y_hat / mu / gain, dequantize, gdn_reparam"""
    rng = np.random.default_rng(seed)
    hs = (rng.standard_normal((1, 6, 9, 16), dtype=np.float32) * 8).astype(np.float32)
    hs[0, 0, 0, 8], hs[0, 0, 1, 8] = -30, 30
    mu, sg = oracle.hyper_params(hs, 8, 5, 7)
    y = (rng.standard_normal((1, 5, 7, 8), dtype=np.float32) * 20).astype(np.float32)
    y[0, 0, 0, :4] = [0.5, 1.5, 2.5, -0.5]
    y[0, 0, 1, :2] = [400, -400]
    gain = rng.standard_normal(8).astype(np.float32)
    q, yh = oracle.quantize_center(y, mu, gain)
    q0, yh0 = oracle.quantize_center(y)
    beta = np.abs(rng.standard_normal(8)).astype(np.float32)
    gamma = (rng.standard_normal((8, 8)) * 0.1).astype(np.float32)
    be, ge = oracle.gdn_reparam(beta, gamma, 1e-3, 2 ** -18, 2 ** -36)
    want = {'mu': mu, 'sigma': sg, 'gain': oracle.channel_gain(y, gain), 'gain_none': oracle.channel_gain(y, None), 'q': q, 'yh': yh,
            'q0': q0, 'yh0': yh0, 'q_only': q, 'deq': oracle.dequantize(q, mu, gain), 'deq0': oracle.dequantize(q0), 'be': be, 'ge': ge}

    def call(ops, d):
        out = {}
        out['mu'], out['sigma'] = ops.hyper_params(d['hs'], 8, 5, 7)
        out['gain'] = ops.channel_gain(d['y'], d['gain'])
        out['gain_none'] = ops.channel_gain(d['y'], None)
        out['q'], out['yh'] = ops.quantize_center(d['y'], d['mu'], d['gain'])
        out['q0'], out['yh0'] = ops.quantize_center(d['y'])
        out['q_only'], none = ops.quantize_center(d['y'], d['mu'], d['gain'], want_yhat=False)
        assert none is None
        out['deq'] = ops.dequantize(d['q'], d['mu'], d['gain'])
        out['deq0'] = ops.dequantize(d['q0'])
        out['be'], out['ge'] = ops.gdn_reparam(d['beta'], d['gamma'], 1e-3, 2 ** -18, 2 ** -36)
        return out
    return Case({'hs': hs, 'y': y, 'gain': gain, 'mu': mu, 'q': q, 'q0': q0, 'beta': beta, 'gamma': gamma}, call, want, eq_all)


# ---- entropy model and rate ------------------------------------------------------------------------------------------------------
def cdf_case(oracle, seed, sig_shape):
    """balle_cdf_table with and without the float table, laplace_cdf_rows / laplace_cdf_windows / laplace_bounds on 4 of 8 maps with
    sigma at both ends of its range, table_bounds, nonzero_flags of a batch whose images each have their own all-zero maps"""
    rng = np.random.default_rng(seed)
    params = (rng.standard_normal((6, abi.BALLE_PARAMS)) * 1.2).astype(np.float32)
    table, cdf = oracle.balle_cdf_table(params)
    sig = np.exp(rng.uniform(np.log(1e-4), np.log(148.4), sig_shape)).astype(np.float32)
    sig[0, 0, 0, 0], sig[0, 0, 0, 1] = 1e-4, 148.41316
    maps = [0, 2, 3, 7]
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig), -256, 255).astype(np.int16)
    qz = rng.integers(-5, 6, (1, 3, 4, 6)).astype(np.int16)
    qb = np.clip(np.rint(rng.laplace(0, 1, (5, 6, 7, 8)) * 3), -256, 255).astype(np.int16)
    for i, dead in enumerate(([], [0], [1, 7], list(range(8)), [3])):
        qb[i][..., dead] = 0
    win, sp = oracle.laplace_cdf_windows(sig, maps)
    want = {'t': table, 'c': cdf, 't_only': table, 'rows': oracle.laplace_cdf_rows(sig, maps), 'win': win, 'sp': sp,
            'bounds': oracle.laplace_bounds(sig, q, maps), 'tbounds': oracle.table_bounds(table, qz),
            'flags': np.array([[1 if k in oracle.nonzero_maps(qb[i:i + 1]) else 0 for k in range(8)] for i in range(5)], np.uint8)}

    def call(ops, d):
        out = {}
        out['t'], out['c'] = ops.balle_cdf_table(d['params'], want_float=True)
        out['t_only'] = ops.balle_cdf_table(d['params'])
        out['rows'] = ops.laplace_cdf_rows(d['sig'], maps)
        out['win'], out['sp'] = ops.laplace_cdf_windows(d['sig'], maps)
        out['bounds'] = ops.laplace_bounds(d['sig'], d['q'], maps)
        out['tbounds'] = ops.table_bounds(d['table'], d['qz'])
        out['flags'] = ops.nonzero_flags(d['qb'])
        return out
    return Case({'params': params, 'sig': sig, 'q': q, 'qz': qz, 'qb': qb, 'table': _i16(table)}, call, want, eq_all,
                maps=maps, npos=len(maps) * sig.shape[1] * sig.shape[2])


FRAME_BATCH_CASES = [((5, 7, 9, 16), [[0, 3, 15], [], [1], list(range(16)), [2, 14]]),  # shape, coded maps of every frame
                     ((4, 5, 6, 12), [list(range(12)), [], [0, 11], [5]])]                # (c % 8 != 0: the scatter's scalar tail)


def frame_batch_case(oracle, seed, shape, maps):
    """the _batch forms of the entropy kernels on ragged per-frame map lists with a frame that codes nothing, against the oracle
    frame by frame.  call(ops, d, out=(win, sp)): the caller's window / sigma tensors of at least `total` rows."""
    n, h, w, c = shape
    npix = h * w
    rng = np.random.default_rng(seed)
    sig = (np.abs(rng.standard_normal(shape)) * 2 + 0.05).astype(np.float32)
    q = np.clip(np.rint(rng.standard_normal(shape) * sig), -256, 256).astype(np.int16)
    table = rng.integers(0, 65535, (c, abi.CDF_ROW)).astype(np.uint16)
    syms = [_i16((q[f].reshape(npix, c)[:, m].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16)) if m else None for f, m in enumerate(maps)]
    want = {'b': [oracle.laplace_bounds(sig[f:f + 1], q[f:f + 1], m) if m else None for f, m in enumerate(maps)],
            'w': [oracle.laplace_cdf_windows(sig[f:f + 1], m) if m else None for f, m in enumerate(maps)],
            'tb': np.stack([oracle.table_bounds(table, q[f:f + 1]) for f in range(n)]), 'q': np.zeros_like(q)}
    for f, m in enumerate(maps):
        want['q'][f][..., m] = q[f][..., m]

    def call(ops, d, out):
        r = {'win': out[0], 'sp': out[1]}
        r['b'], r['offs'] = ops.laplace_bounds_batch(d['sig'], d['q'], maps)
        offs2, r['tab'] = ops.laplace_cdf_windows_batch(d['sig'], maps, out)
        assert offs2 == r['offs']
        r['tb'] = ops.table_bounds_batch(d['table'], d['q'])
        r['q'] = ops.scatter_symbols_batch(d['sym'], maps, n, npix, c, table=r['tab'])
        r['q2'] = ops.scatter_symbols_batch(d['sym'], maps, n, npix, c)  # (its own device table)
        for f, m in enumerate(maps):
            if m:
                r['q1_%d' % f] = ops.scatter_symbols(d['syms'][f], npix, c, m)
        return r

    def compare(r, want):
        for f, m in enumerate(maps):
            if m:
                sl = slice(r['offs'][f], r['offs'][f] + len(m) * npix)
                eq(r['b'][sl], want['b'][f])
                eq(r['win'][sl], want['w'][f][0]), eq(r['sp'][sl], want['w'][f][1])
                eq(r['q1_%d' % f].view(h, w, c), want['q'][f])
        eq(r['tb'], want['tb'])
        eq(r['q'].view(n, h, w, c), want['q']), eq(r['q2'].view(n, h, w, c), want['q'])
    inputs = {'sig': sig, 'q': q, 'table': _i16(table), 'sym': np.concatenate([s for s in syms if s is not None]), 'syms': syms}
    return Case(inputs, call, want, compare, total=sum(len(m) for m in maps) * npix)


def straddle_stream(rng, n, burst):
    """packed (c_lo | c_hi << 16) bounds whose intervals keep sitting across the middle of the coder's range: every such
    symbol adds ~14 straddle (E3) steps to the pending count, `burst` of them in a row push it past 32 and far beyond,
    then a symbol that settles releases the run -- the encoder's long-run path, followed by ordinary symbols"""
    out = []
    while len(out) < n:
        for _ in range(int(rng.integers(1, burst + 1))):
            d = int(rng.integers(1, 4))
            out.append((0x8000 - d) | ((0x8000 + int(rng.integers(1, 4))) << 16))
        lo = int(rng.integers(0, 0xF000))
        out.append(lo | ((lo + int(rng.integers(1, 0x0FFF))) << 16))
        for _ in range(int(rng.integers(0, 40))):
            lo = int(rng.integers(0, 0xFFF0))
            hi = lo + int(rng.integers(1, 0x10000 - lo))
            out.append(lo | ((hi & 0xFFFF) << 16))  # hi = 2^16 packs as 0
    return np.array(out[:n], np.uint32)


def stream_bytes(out, ln, offs):
    """what ops.range_encode returned -> the bytes of every stream"""
    out_h, ln_h = out.cpu().numpy(), ln.cpu().numpy()
    return [out_h[off:off + int(m)].tobytes() for (off, cap), m in zip(offs, ln_h)]


def range_encode_case(oracle, seed, fixed_lens, n_random, max_len, straddle):
    """a batch of streams for ONE ops.range_encode call: the fixed lengths, then n_random ones below max_len; ordinary Laplace
    symbols and, with `straddle`, adversarial straddle runs in every third stream.  call(ops, d, bounds=...): another list of
    tensors that hold the first streams (slices of one tensor, fewer streams)."""
    rng = np.random.default_rng(seed)
    lens = list(fixed_lens) + [int(v) for v in rng.integers(1, max_len, n_random)]
    streams = []
    for i, n in enumerate(lens):
        if straddle and i % 3 == 2:
            streams.append(straddle_stream(rng, n, burst=1 + i % 9))
        else:
            sig = np.clip(np.exp(rng.uniform(np.log(0.05), np.log(40.0), (1, 1, max(n, 1), 1))), 1e-4, 148.4).astype(np.float32)
            q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig / np.sqrt(2)), -256, 255).astype(np.int16)
            streams.append(oracle.laplace_bounds(sig, q, [0])[:n])
    want = [oracle.range_encode(b) for b in streams]
    assert max(len(w) for w in want) > 0

    def compare(result, want):
        for i, (got, w) in enumerate(zip(stream_bytes(*result), want)):
            assert got == w, (i, lens[i])
    return Case({'streams': [_i32(b) for b in streams]}, lambda ops, d, bounds=None: ops.range_encode(d['streams'] if bounds is None else bounds),
                want, compare, lens=lens)


RANGE_CODER_CASES = [(1, 1.0), (63, 0.3), (64, 2.0), (65, 5.0), (1000, 0.05), (5000, 1.0), (20000, 40.0), (3000, 1e-4), (70000, 0.8)]  # n_sym, scale
RANGE_DECODE_CASES = [(1, 1.0), (65, 5.0), (1000, 0.05), (5000, 40.0)]  # (the guarded decoder's)


def range_coder_case(oracle, n_sym, scale, trim=True, windows=False):
    """one stream of Laplace symbols on 4 maps: n_sym of them (trim) or whole maps; encoded (call(..., encode=True)) and decoded from
    full CDF rows with the bit count; with `windows` also from 64-entry windows + sigma per position, and twice side by side, the
    second from its own row offset, into a flat output"""
    rng = np.random.default_rng(n_sym)
    c = 4
    npix = (n_sym + c - 1) // c
    sig = (np.exp(rng.uniform(np.log(0.05), np.log(4.0), (1, 1, npix, c))) * scale).astype(np.float32)
    sig = np.clip(sig, 1e-4, 148.4).astype(np.float32)
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig / np.sqrt(2)), -256, 255).astype(np.int16)
    maps = list(range(c))
    n = n_sym if trim else npix * c
    bounds = oracle.laplace_bounds(sig, q, maps)[:n]
    payload = oracle.range_encode(bounds)
    rows = oracle.laplace_cdf_rows(sig, maps)[:n]
    sym, bits = oracle.range_decode(payload, rows, n, want_bits=True)
    np.testing.assert_array_equal(sym, (q.reshape(-1, c).T.reshape(-1)[:n].astype(np.int32) + 256).astype(np.uint16))
    assert len(payload) == (bits + 2 + 7) // 8  # the bits shifted in by renormalisation account for the payload length
    inputs = {'bounds': _i32(bounds), 'rows': _i16(rows)}
    if windows:
        win, sp = oracle.laplace_cdf_windows(sig, maps)
        inputs.update(win=_i16(win[:n]), sp=sp[:n], rows2=_i16(np.concatenate([rows, rows])))

    def call(ops, d, encode=True):
        out = {}
        if encode:
            out['enc'] = ops.range_encode([d['bounds']])
        (out['sym'],), out['bits'] = ops.range_decode([payload], d['rows'], [0], [n], [0], want_bits=True)
        if windows:
            (out['sym_w'],), out['bits_w'] = ops.range_decode([payload], d['win'], [0], [n], [0], sigma_pos=d['sp'], want_bits=True)
            out['flat'] = ops.range_decode([payload, payload], d['rows2'], [0, n], [n, n], [0, 0], flat=True)
        return out

    def compare(out, want):
        if 'enc' in out:
            assert stream_bytes(*out['enc']) == [payload]
        eq(out['sym'], sym)
        assert int(out['bits'].cpu()[0]) == bits
        if windows:
            eq(out['sym_w'], sym)
            assert int(out['bits_w'].cpu()[0]) == bits
            eq(out['flat'], np.concatenate([sym, sym]))
    return Case(inputs, call, sym, compare)


FORCED = [-256, -255, -33, -32, 30, 31, 32, 254, 255, 256]  # symbols 0, 1, 223, 224, 286, 287, 288, 510, 511, 512


def forced_case(sigma, repeat=7):
    """a stream that visits the edges of the decoder's window, of the alphabet and of the last octet, at one sigma"""
    q = np.array((FORCED + [0, 1, -1]) * repeat, np.int16).reshape(1, 1, -1, 1)
    return np.full(q.shape, sigma, np.float32), q


def range_coder_pmf_case(oracle, seed):
    """pmf tables: 42 symbols per row of 5; decoded and scattered back to [42, 5]"""
    rng = np.random.default_rng(seed)
    params = (rng.standard_normal((5, abi.BALLE_PARAMS)) * 0.8).astype(np.float32)
    table, _ = oracle.balle_cdf_table(params)
    qz = rng.integers(-3, 4, (1, 6, 7, 5)).astype(np.int16)
    bounds = oracle.table_bounds(table, qz)
    payload = oracle.range_encode(bounds)

    def call(ops, d, encode=True):
        out = {}
        if encode:
            out['enc'] = ops.range_encode([d['bounds']])
        out['sym'] = ops.range_decode([payload], d['table'], [0], [qz.size], [42])[0]
        out['back'] = ops.scatter_symbols(out['sym'], 42, 5, list(range(5)))
        return out

    def compare(out, want):
        if 'enc' in out:
            assert stream_bytes(*out['enc']) == [payload]
        eq(out['sym'], want)
        eq(out['back'], qz.reshape(42, 5))
    return Case({'bounds': _i32(bounds), 'table': _i16(table)}, call, oracle.range_decode(payload, table, qz.size, plane=42), compare, qz=qz)


def bounds_rate_case(oracle, seed, n):
    rng = np.random.default_rng(seed)
    lo = rng.integers(0, 0xFFFF, n)
    hi = lo + 1 + (rng.integers(0, 0x10000, n) % (0x10000 - lo))
    b = (lo | ((hi & 0xFFFF) << 16)).astype(np.uint32)

    def compare(got, want):
        assert float(got.cpu()) == want
    return Case({'b': _i32(b)}, lambda ops, d: ops.bounds_rate(d['b']), oracle.bounds_rate(b), compare)


def rate_estimates_case(oracle, seed, shape):
    """laplace_prob with and without mu, table_prob, rate_bits"""
    rng = np.random.default_rng(seed)
    y = np.rint(rng.standard_normal(shape) * 6).astype(np.float32)
    mu = rng.standard_normal(shape).astype(np.float32)
    sigma = np.exp(rng.uniform(-3, 3, shape)).astype(np.float32)
    params = (rng.standard_normal((shape[1], abi.BALLE_PARAMS)) * 0.8).astype(np.float32)
    _, cdf = oracle.balle_cdf_table(params)
    p_zero = oracle.laplace_prob(y, None, sigma)
    rate, total = oracle.rate_bits(p_zero, 2.0 ** -16, 1.0)
    want = {'p_mu': oracle.laplace_prob(y, mu, sigma), 'p_zero': p_zero, 'p_z': oracle.table_prob(y, cdf), 'rate': rate}

    def call(ops, d):
        out = {'p_mu': ops.laplace_prob(d['y'], d['mu'], d['sigma']), 'p_zero': ops.laplace_prob(d['y'], None, d['sigma']),
               'p_z': ops.table_prob(d['y'], d['cdf'])}
        out['rate'], out['total'] = ops.rate_bits(d['p_zero'], 2.0 ** -16, 1.0)
        return out

    def compare(out, want):
        eq_all({k: v for k, v in out.items() if k != 'total'}, want)
        assert float(out['total'].cpu()) == total
    return Case({'y': y, 'mu': mu, 'sigma': sigma, 'cdf': cdf, 'p_zero': p_zero}, call, want, compare)


# ---- deterministic transcendentals -----------------------------------------------------------------------------------------------
def detmath_case(oracle, fn, a, b=None):
    """aivc_detmath_eval of one function of include/aivc_detmath.h at the arguments a (and b): device bits == host bits, a NaN
    matching any NaN (payload and sign of a NaN are not part of the contract)"""
    from detmath_cases import same_bits
    dt = np.float64 if abi.detmath_is_fp64(fn) else np.float32
    a = np.ascontiguousarray(a, dt)
    b = None if b is None else np.ascontiguousarray(b, dt)

    def compare(got, want):
        got = got.cpu().numpy()
        ok = same_bits(got, want)
        if not ok.all():
            i = np.flatnonzero(~ok)
            u = np.uint64 if dt == np.float64 else np.uint32
            raise AssertionError('detmath fn %d: device != host at %d of %d arguments; first a = %r (bits 0x%X)%s: device %r (0x%X), host %r (0x%X)'
                                 % (fn, i.size, a.size, a[i[0]], int(a.view(u)[i[0]]), '' if b is None else ', b = %r' % b[i[0]],
                                    got[i[0]], int(got.view(u)[i[0]]), want[i[0]], int(want.view(u)[i[0]])))
    return Case({'a': a, 'b': b}, lambda ops, d: ops.detmath_eval(fn, d['a'], d['b']), oracle.detmath_eval(fn, a, b), compare, n=a.size)


WINDOW_CHUNK_TMIN = {0: 25.5, 1: 17.5, 2: 9.5, 3: 1.5, 5: 7.5, 6: 15.5, 7: 23.5}  # csrc/entropy.hip: |t| of a chunk's entry nearest to the centre


def saturation_threshold_case(oracle, chunk):
    """laplace_cdf_windows where the windows kernel decides, per wavefront and 8-entry chunk, whether every lane is saturated
    (tmin / b > 17.5f for b = sigma / 1.41421354f: the entries are then k or 65023 + k without any fp64 work).  sigma takes the 9
    floats around tmin * 1.41421354f / 17.5f of this chunk, on both sides of that test, over (1, 9, 13, 6) with maps [0, 2, 5]: 351
    positions in stream order = 5 whole wavefronts and one of 31 valid lanes --
      0: every lane just saturated            1: one lane just unsaturated, the others just saturated
      2: the band in turn, both sides         3: every lane just unsaturated
      4: the band at random                   5 (31 valid lanes): every valid lane just saturated
    -> Case with the oracle's windows and sigma per position, which equal the slice of its full rows; q / payload: a stream coded
    with these rows whose symbols leave the window too (the decoder's slow path rebuilds rows from sigma_pos).
    What this proves: the shortcut writes the entries the long path writes, lane by lane, where lanes disagree about it.  What it
    cannot: at the threshold both paths give the same entries by construction (expm1f is -1 from -17.33 on), so a predicate that
    is slightly off (17.0f, or any lane instead of all) passes here as well."""
    h, w, c, maps = 9, 13, 6, [0, 2, 5]
    npix, tmin = h * w, np.float32(WINDOW_CHUNK_TMIN[chunk])
    s0 = tmin * np.float32(1.41421354) / np.float32(17.5)
    band = (s0.view(np.int32) + np.arange(-4, 5, dtype=np.int32)).view(np.float32)
    sat = tmin / (band / np.float32(1.41421354)) > np.float32(17.5)  # the kernel's own test, in IEEE fp32
    assert sat.any() and not sat.all() and np.all(sat[:-1] >= sat[1:]), (band, sat)  # (saturated below a threshold inside the band)
    lo, hi = band[sat][-1], band[~sat][0]  # the last saturated sigma and the first unsaturated one: neighbours
    rng = np.random.default_rng(chunk)
    per_pos = np.empty(len(maps) * npix, np.float32)
    per_pos[0:64] = lo
    per_pos[64:128] = lo
    per_pos[64 + 37] = hi
    per_pos[128:192] = band[np.arange(64) % band.size]
    per_pos[192:256] = hi
    per_pos[256:320] = rng.choice(band, 64)
    per_pos[320:] = band[sat][rng.integers(0, int(sat.sum()), per_pos.size - 320)]
    sig = rng.uniform(0.5, 2.0, (1, h, w, c)).astype(np.float32)  # (the maps that are not coded)
    sig.reshape(npix, c)[:, maps] = per_pos.reshape(len(maps), npix).T  # position = map * npix + pixel
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig / np.sqrt(2)), -256, 255).astype(np.int16)
    q.reshape(-1)[::7] = np.array([33, -33, 40, -34, 32, -32, 31], np.int16)[np.arange(q.size)[::7] % 7]
    rows = oracle.laplace_cdf_rows(sig, maps)
    win, sp = oracle.laplace_cdf_windows(sig, maps)
    np.testing.assert_array_equal(sp, per_pos)
    np.testing.assert_array_equal(win, rows[:, abi.CDF_WIN0:abi.CDF_WIN0 + abi.CDF_WIN])
    payload = oracle.range_encode(oracle.laplace_bounds(sig, q, maps))
    sym = oracle.range_decode(payload, rows, per_pos.size)
    np.testing.assert_array_equal(sym, (q.reshape(npix, c)[:, maps].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16))
    assert (np.abs(sym.astype(np.int32) - 256) > 32).any()

    def call(ops, d):
        out = {}
        out['win'], out['sp'] = ops.laplace_cdf_windows(d['sig'], maps)
        (out['sym'],), _ = ops.range_decode([payload], out['win'], [0], [per_pos.size], [0], sigma_pos=out['sp'], want_bits=True)
        return out
    return Case({'sig': sig}, call, {'win': win, 'sp': sp, 'sym': sym}, eq_all, saturated=sat, band=band)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
def metrics_case(oracle, h, w, ws):
    """ssim_means, pool2x2 with both edges, sq_err on three fp64 planes and a noisy copy.  fp64 kernels: 1e-12 against the fp64
    oracle (separable against 2-D window summation order); integer-valued planes: the sum of squares is exact in fp64"""
    from oracle import metrics
    rng = np.random.default_rng(h * 100 + w)
    a = rng.uniform(0, 255, (3, h, w))
    b = np.clip(a + rng.normal(0, 9, a.shape), 0, 255)
    win = metrics.window_clic(ws, ws * 1.5 / 11)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    ia, ib = np.rint(a), np.rint(b)
    want = {'ssim': oracle.ssim_means(a, b, win, c1, c2), 'pool0': oracle.pool2x2(a, 0), 'pool1': oracle.pool2x2(a, 1),
            'se': oracle.sq_err(a, b)[0], 'se_int': oracle.sq_err(ia, ib)[0]}

    def call(ops, d):
        out = {'ssim': ops.ssim_means(d['a'], d['b'], win, c1, c2), 'se': ops.sq_err(d['a'], d['b']), 'se_int': ops.sq_err(d['ia'], d['ib'])}
        for edge in (0, 1):
            out['pool%d' % edge] = ops.pool2x2(d['a'], edge)
        return out

    def compare(out, want):
        np.testing.assert_allclose(out['ssim'].cpu().numpy(), want['ssim'], rtol=0, atol=1e-12)
        for edge in (0, 1):
            np.testing.assert_array_equal(out['pool%d' % edge].cpu().numpy(), want['pool%d' % edge])
        assert abs(out['se'].item() - want['se']) <= 1e-12 * want['se']
        assert out['se_int'].item() == want['se_int']
    return Case({'a': a, 'b': b, 'ia': ia, 'ib': ib}, call, want, compare)
