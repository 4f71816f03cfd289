"""The regimes of the pixel, latent, entropy and rate ops beyond N(0, 1) data, finite flows and sigma inside [1e-4, 148.4], each
stated once: the value sets, and builders that return tests/op_cases.py Case objects.  tests/test_op_regimes.py (the CPU oracle
against this suite's own numpy restatements) and tests/test_gpu_op_regimes.py / tests/test_gpu_memory_discipline.py (the device
against the oracle, bit for bit) run them.  The analogue of tests/numeric_regimes.py for everything that is not a conv: what
the conv regimes prove the convs emit -- inf, NaN, signed zeros, subnormals -- is what these kernels are fed next.  Not a test
module.

Every builder asserts its reach condition ON THE ORACLE'S RESULT, on the CPU, so a seed cannot quietly miss the regime.  The
contract the values are held to is written in include/aivc_hip.h and include/aivc_detmath.h:
  * a NaN sample position of the warp (a NaN flow; inf * 0 on an axis of size 1) is position 0, +-inf the nearer edge;
  * a NaN pixel is byte 0 and a NaN float level; a NaN latent is q = 0 and a NaN y_hat;
  * a cdf is clamped to [0, 1] before it is quantised, a NaN cdf to 0: every float is a sigma with a defined row.
"""
import numpy as np

from aivc_amd import abi
from numeric_regimes import planted
from op_cases import Case, _i16, _i32, eq_all, frame_sources, frame_to_yuv420_case, warp_blend_case
from warp_modes_cases import sample_position

f32 = np.float32
NAN, INF, BIG = f32(np.nan), f32(np.inf), f32(3e38)
TINY = f32(1e-45)  # the smallest subnormal


def around(v, n=4):
    """v and the n floats on each side of it, ascending for v > 0"""
    return (np.array([v], f32).view(np.int32) + np.arange(-n, n + 1, dtype=np.int32)).view(f32)


def total_bits(v):
    """a float64 total as its bit pattern, every NaN as one value: totals are compared by bits, not with =="""
    v = np.float64(v)
    return 'nan' if np.isnan(v) else int(v.view(np.uint64))


def _some_pixels(rng, shape, frac=0.2):
    """indices (tuple of arrays) of round(frac * pixels) distinct pixels of an [n, h, w] grid, at least one"""
    npix = int(np.prod(shape))
    k = max(1, int(round(frac * npix)))
    return np.unravel_index(rng.permutation(npix)[:k], shape)


def _assert_planted_fraction(mask):
    """5 % to 50 % of the pixels carry a planted value (a grid of fewer than 4 pixels: at least one of them does)"""
    if mask.size < 4:
        assert mask.any()
    else:
        assert 0.05 <= mask.mean() <= 0.5, float(mask.mean())


# ---- warp and warp_blend ---------------------------------------------------------------------------------------------------------
# A set is a list of kinds; a kind maps (row, col, h, w, fx, fy) of a planted pixel to its flow.  `integer`: the sample lands on a
# whole position inside the frame, exactly on size - 1, and on position 0 (-col, -row).
FLOWS = {
    'nan_x': [lambda r, q, h, w, fx, fy: (NAN, fy)],
    'nan_y': [lambda r, q, h, w, fx, fy: (fx, NAN)],
    'nan_xy': [lambda r, q, h, w, fx, fy: (NAN, NAN)],
    'inf': [lambda r, q, h, w, fx, fy: (INF, fy), lambda r, q, h, w, fx, fy: (-INF, fy), lambda r, q, h, w, fx, fy: (fx, INF),
            lambda r, q, h, w, fx, fy: (fx, -INF), lambda r, q, h, w, fx, fy: (INF, -INF)],
    'big': [lambda r, q, h, w, fx, fy: (BIG, fy), lambda r, q, h, w, fx, fy: (-BIG, fy), lambda r, q, h, w, fx, fy: (fx, BIG),
            lambda r, q, h, w, fx, fy: (fx, -BIG), lambda r, q, h, w, fx, fy: (-BIG, BIG)],
    'integer': [lambda r, q, h, w, fx, fy: (f32((q + 2) % w - q), f32((r + 1) % h - r)),
                lambda r, q, h, w, fx, fy: (f32(w - 1 - q), f32(h - 1 - r)),
                lambda r, q, h, w, fx, fy: (f32(-q), f32(-r))],
}
WARP_REGIME_SHAPES = [(2, 5, 7), (2, 5, 1), (1, 1, 1)]  # n, h, w; the axes of size 1: (g + 1) / 2 * (size - 1) is inf * 0 for an infinite flow
BLEND_SIZES = [(6, 8), (5, 7)]
# alpha = clamp(m0 + 0.5, 0, 1) (beta from m1 likewise): NaN, +-inf, the two ends of the clamp and one float to either side
ALPHA_BETA = np.concatenate([np.array([NAN, INF, -INF], f32), around(f32(-0.5), 1), around(f32(0.5), 1)])


def plant_flows(rng, flow, name, h, w, where=None):
    """flow [n, hm, wm, 2] (hm >= h, wm >= w: the frame is its top left corner) -> bool [n, h, w]: the planted pixels"""
    n = flow.shape[0]
    where = _some_pixels(rng, (n, h, w)) if where is None else where
    kinds = FLOWS[name]
    mask = np.zeros((n, h, w), bool)
    for i, (b, r, q) in enumerate(zip(*where)):
        flow[b, r, q] = kinds[i % len(kinds)](r, q, h, w, flow[b, r, q, 0], flow[b, r, q, 1])
        mask[b, r, q] = True
    return mask


def warp_regime_case(oracle, name, shape, seed):
    """aivc_warp (ops.warp in the codec's mode) on an N(0, 1) * 2 flow with the set `name` planted, 4 channels.  Reach: 5 % to 50 %
    of the pixels carry a planted flow; the oracle is finite at every pixel (the image is finite: a NaN or infinite flow is a
    position inside the frame, nothing else)"""
    n, h, w = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, 4), dtype=f32)
    flow = (rng.standard_normal((n, h, w, 2), dtype=f32) * f32(2)).astype(f32)
    mask = plant_flows(rng, flow, name, h, w)
    want = oracle.warp(x, flow)
    _assert_planted_fraction(mask)
    assert np.isfinite(want).all(), (name, shape, np.argwhere(~np.isfinite(want))[:4].tolist())
    return Case({'x': x, 'flow': flow}, lambda ops, d: ops.warp(d['x'], d['flow']), want, planted=mask)


def warp_taps_of(flow_nhwc, h, w):
    """-> (y0, x0) int [n, h, w]: the first tap of every pixel of the codec's warp, from the fp32 position restated in
    tests/warp_modes_cases.py, clamped with a NaN at 0; the taps of a pixel are (y0, x0), (y0, x0 + 1), (y0 + 1, x0),
    (y0 + 1, x0 + 1), those inside the frame"""
    y0, x0 = [], []
    for f in flow_nhwc:
        px, py = sample_position(np.transpose(f, (2, 0, 1))[None], h, w, True)
        with np.errstate(invalid='ignore'):
            px = np.where(px > 0, px, f32(0))
            py = np.where(py > 0, py, f32(0))
        x0.append(np.floor(np.minimum(px, f32(w - 1))).astype(np.int64))
        y0.append(np.floor(np.minimum(py, f32(h - 1))).astype(np.int64))
    return np.stack(y0), np.stack(x0)


def warp_image_case(oracle, shape, seed):
    """inf and NaN PIXELS under flows that land on whole positions: a tap of weight 0 still multiplies its pixel (0 * inf = NaN).
    Pixels (0, 0) of image 0 and (1, 1) of the last image sample position 0 exactly (flow -col, -row: weights 1, 0, 0, 0).
    Reach, as Nonfinite.reach of tests/numeric_regimes.py: some outputs are non-finite, fewer than half, none outside the
    footprint (a channel of an output pixel may be non-finite only if one of its taps inside the frame is, in that channel);
    and the weight-0 product itself: an output is NaN where the tap of weight 1 is finite and a tap of weight 0 is inf"""
    n, h, w = shape
    assert h >= 3 and w >= 3
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, 4), dtype=f32)
    flow = rng.integers(-2, 3, (n, h, w, 2)).astype(f32)
    flow[0, 0, 0] = 0
    flow[n - 1, 1, 1] = -1
    x[0, 0, 1, 0] = INF       # the weight-0 neighbour of pixel (0, 0) of image 0, to the right
    x[0, 1, 0, 1] = NAN       # ... below
    x[n - 1, 1, 1, 2] = -INF  # the weight-0 diagonal neighbour of position 0 of the last image
    x[n - 1, h - 1, w - 1, 3] = INF
    want = oracle.warp(x, flow)
    bad = ~np.isfinite(want)
    y0, x0 = warp_taps_of(flow, h, w)
    allowed = np.zeros_like(bad)
    for b in range(n):
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0[b] + dy, x0[b] + dx
                ok = (yy < h) & (xx < w)
                allowed[b] |= ok[..., None] & ~np.isfinite(x[b, np.minimum(yy, h - 1), np.minimum(xx, w - 1)])
    assert 0 < bad.sum() < bad.size / 2, int(bad.sum())
    assert not (bad & ~allowed).any(), np.argwhere(bad & ~allowed)[:4].tolist()
    assert np.isnan(want[0, 0, 0, 0]) and np.isfinite(x[0, 0, 0, 0])
    assert np.isnan(want[0, 0, 0, 1]) and np.isnan(want[n - 1, 1, 1, 2]) and np.isfinite(x[n - 1, 0, 0, 2])
    return Case({'x': x, 'flow': flow}, lambda ops, d: ops.warp(d['x'], d['flow']), want)


def warp_blend_regime_case(oracle, name, size, ft, general=False, rows=None, seed=0):
    """warp_blend_case of tests/op_cases.py (bit exact on pred, skip, x_warp, alpha, beta) with the flow set `name` planted in the
    MOFNet channels 2..3 (previous reference) and 4..5 (next) and ALPHA_BETA in channels 0 and 1, at pixels of their own.
    Reach: the planted fractions; x_warp is finite at every pixel whose alpha and beta channels are ordinary (the references
    are finite), and ALPHA_BETA shows in the oracle's alpha as NaN, 0, 1 and values strictly between"""
    h, w = size
    rng = np.random.default_rng(seed)
    mof = rng.standard_normal((2, h + 2, w + 1, 8), dtype=f32)
    mof[..., 2:6] *= f32(2)
    prev, nxt = rng.random((2, h, w, 4), dtype=f32), rng.random((2, h, w, 4), dtype=f32)
    px = _some_pixels(rng, (2, h, w), 0.45)  # the first half takes flows, the second alpha / beta
    k = len(px[0]) // 2
    fl = tuple(a[:k] for a in px)
    ab = tuple(a[k:] for a in px)
    mask = plant_flows(rng, mof[..., 2:4], name, h, w, fl)
    plant_flows(rng, mof[..., 4:6], name, h, w, tuple(a[::-1] for a in fl))  # (the same pixels, the kinds in another order)
    mask_ab = np.zeros((2, h, w), bool)
    for i, (b, r, q) in enumerate(zip(*ab)):
        mof[b, r, q, 0] = ALPHA_BETA[i % ALPHA_BETA.size]
        mof[b, r, q, 1] = ALPHA_BETA[(i // 2) % ALPHA_BETA.size]
        mask_ab[b, r, q] = True
    case = warp_blend_case(oracle, (mof, prev, nxt), h, w, ft, general=general, want_aux=True, rows=rows)
    _assert_planted_fraction(mask)
    _assert_planted_fraction(mask_ab)
    whole = oracle.warp_blend(mof if not general else np.ascontiguousarray(mof[..., :7]), prev[..., :3 if general else 4].copy(),
                              nxt[..., :3 if general else 4].copy(), h, w, ft, co=3 if general else 4)
    assert np.isfinite(whole['x_warp'][~mask_ab]).all()
    al = whole['alpha'][mask_ab]
    assert np.isnan(al).any() and (al == 0).any() and (al == 1).any() and ((al > 0) & (al < 1)).any()
    return case


# ---- frame_to_yuv420 -------------------------------------------------------------------------------------------------------------
def cast8_ties():
    """every fp32 c near (k + 0.5) / 255 whose fp32 product 255.0f * c is k + 0.5 exactly -> [(c, k)]; found by search over the
    floats around each quotient.  At least one k of each parity must exist (asserted)"""
    out = []
    for k in range(255):
        for c in around(f32((k + 0.5) / 255.0), 3):
            if f32(255.0) * c == f32(k + 0.5):
                out.append((c, k))
    assert any(k % 2 == 0 for _, k in out) and any(k % 2 == 1 for _, k in out), len(out)
    return out


FRAME_REGIME_SIZES = [(10, 14), (9, 13), (1, 1)]  # (10, 14) in the hand-over layout (3 channels, even pitch) takes the vector kernel


def frame_pixel_values():
    """NaN, +-inf, below 0, above 1, the floats around 0 and 1, then two ties of each parity"""
    ties = cast8_ties()
    ev, od = [c for c, k in ties if k % 2 == 0], [c for c, k in ties if k % 2 == 1]
    head = [NAN, INF, -INF, f32(-0.25), f32(1.5), np.nextafter(f32(0), f32(1)), np.nextafter(f32(0), f32(-1)), f32(-0.0),
            np.nextafter(f32(1), f32(0)), np.nextafter(f32(1), f32(2)), f32(0), f32(1)]
    return np.array(head + [ev[0], od[0], ev[len(ev) // 2], od[len(od) // 2], ev[-1], od[-1]], f32)


def frame_regime_case(oracle, size, handover, with_skip, want_float, seed=0):
    """frame_to_yuv420_case of tests/op_cases.py with frame_pixel_values() planted in all three channels of a fifth of the pixels
    (the skip there a signed zero, so that x + skip is the planted value), inf + -inf through the skip at one pixel, and three
    chroma blocks of subnormals (+1e-45, -1e-45, mixed with zeros: 0.5f * 1e-45f is a tie that rounds to a zero of its sign).
    Reach (frames of 100 pixels or more): a NaN level with byte 0, bytes 0 and 255, the ties rounded to even in the luma bytes,
    and a level -0.0 in the chroma planes"""
    h, w = size
    rng = np.random.default_rng(seed)
    x, skip, x3 = frame_sources(seed, h, w)
    vals = frame_pixel_values()
    where = _some_pixels(rng, (2, h, w))
    luma_planted = []
    for i, (b, r, q) in enumerate(zip(*where)):
        for ch in range(3):
            x[b, r, q, ch] = vals[(i + 5 * ch) % vals.size]
        skip[b, r, q, :3] = [0.0, -0.0, 0.0]
        luma_planted.append((b, r, q, x[b, r, q, 0]))
    big = h >= 4 and w >= 6
    if big:
        for j, (r0, q0, block) in enumerate(((0, 0, [TINY] * 4), (2, 2, [-TINY] * 4), (0, 4, [TINY, 0, -TINY, -0.0]))):
            for ch in (1, 2):
                x[1, r0:r0 + 2, q0:q0 + 2, ch] = np.array(block, f32).reshape(2, 2)
            skip[1, r0:r0 + 2, q0:q0 + 2, :3] = -0.0 if j else 0.0
        x[0, h - 1, w - 1, :3] = [INF, -INF, INF]
        skip[0, h - 1, w - 1, :3] = [-INF, INF, 1.0] if with_skip else 0.0
    src = np.ascontiguousarray(x[:, :, :w + 2 - (w & 1), :3]) if handover else x
    case = frame_to_yuv420_case(oracle, src, h, w, skip=skip if with_skip else None, want_float=want_float)
    (fy, fu, fv), (by, bu, bv) = case.want
    ties = dict((c.tobytes(), k) for c, k in cast8_ties())
    for b, r, q, v in luma_planted:  # what the contract says of a planted luma value, pixel by pixel
        if np.isnan(v):
            assert by[b, r, q] == 0 and np.isnan(fy[b, r, q])
        elif v.tobytes() in ties:
            k = ties[v.tobytes()]
            assert by[b, r, q] == k + (k & 1), (v, k, by[b, r, q])
    if h * w >= 100:
        seen = [v.tobytes() in ties for _, _, _, v in luma_planted]
        assert any(seen) and np.isnan(fy).any() and (by == 0).any() and (by == 255).any()
        assert ((fu == 0) & np.signbit(fu)).any() or ((fv == 0) & np.signbit(fv)).any()
        if with_skip:
            assert np.isnan(fy[0, h - 1, w - 1]) and by[0, h - 1, w - 1] == 0
    return case


def frame_ties_case(oracle, size, handover, seed=0):
    """EVERY tie of cast8_ties() in the luma of a frame (frame_regime_case plants six of them): pixel i of the two images takes
    tie i, as many as the frame holds -- all of them at (10, 14).  Reach: each byte is the even neighbour of its k + 0.5"""
    h, w = size
    x, _, _ = frame_sources(seed, h, w)
    ties = cast8_ties()
    slots = [(b, r, q) for b in range(2) for r in range(h) for q in range(w)][:len(ties)]
    assert len(slots) == len(ties) or size != (10, 14)
    for (b, r, q), (c, _) in zip(slots, ties):
        x[b, r, q, 0] = c
    src = np.ascontiguousarray(x[:, :, :w + 2 - (w & 1), :3]) if handover else x
    case = frame_to_yuv420_case(oracle, src, h, w, skip=None, want_float=True)
    by = case.want[1][0]
    for (b, r, q), (c, k) in zip(slots, ties):
        assert by[b, r, q] == k + (k & 1), (c, k, by[b, r, q])
    assert {k & 1 for _, k in ties[:len(slots)]} == {0, 1}
    return case


# ---- latent ops ------------------------------------------------------------------------------------------------------------------
LATENT_SHAPE = (2, 5, 7, 8)
GAIN = np.array([0.0, -0.0, np.inf, np.nan, 1.3, -0.7, 2.0, 1e-20], f32)
GAIN_ROWS = np.stack([GAIN, np.array([1.0, np.nan, -0.0, 0.5, np.inf, 0.0, -3.0, 1e-42], f32)])
# (y - mu, rounded half to even and clamped to the alphabet): ties for k even and odd of both signs, the edge of the alphabet
QUANT_TIES = [(0.5, 0), (1.5, 2), (2.5, 2), (-0.5, 0), (-1.5, -2), (-2.5, -2), (255.5, 256), (-255.5, -256),
              (256.5, 256), (-256.5, -256), (257.0, 256), (-257.0, -256)]


def latent_regime_case(oracle, seed=0):
    """quantize_center, dequantize, channel_gain and their _rows forms (one gain row per image).  Planted, each in all 8 channels
    (so under every gain): y - mu at QUANT_TIES (mu a whole number: the difference is exact); y at +-inf, NaN, +-3e38 and
    subnormals; y == mu with both zeros; mu at inf under an infinite y (inf - inf) and at NaN; the gains 0, -0, inf, NaN
    (0 * inf) beside ordinary ones; q at +-256 and at the int16 extremes for dequantize.
    Reach: q at a tie is the even neighbour; q is 0 and y_hat NaN where y - mu is NaN; q reaches +-256; y_hat holds NaN, +-inf
    and both zeros"""
    rng = np.random.default_rng(seed)
    n, h, w, c = LATENT_SHAPE
    y = (rng.standard_normal(LATENT_SHAPE, dtype=f32) * f32(20)).astype(f32)
    mu = rng.standard_normal(LATENT_SHAPE, dtype=f32)
    px = list(zip(*_some_pixels(rng, (n, h, w), 0.45)))
    ties, nan_px = [], []
    for (d, want_q), (b, r, q_) in zip(QUANT_TIES, px):
        mu[b, r, q_] = f32(3.0)
        y[b, r, q_] = f32(3.0) + f32(d)
        ties.append(((b, r, q_), want_q))
    rest = px[len(QUANT_TIES):]
    specials = [(INF, None), (-INF, None), (NAN, None), (BIG, None), (-BIG, None), (TINY, 0.0), (-TINY, 0.0), (-TINY, -0.0), (f32(1e-40), None),
                (f32(2.5), 2.5), (f32(-0.0), -0.0), (f32(0.0), -0.0), (INF, INF), (-INF, INF), (f32(1.0), NAN), (f32(1.0), -INF)]
    assert len(rest) >= len(specials), (len(rest), len(specials))
    for (yv, mv), (b, r, q_) in zip(specials, rest):
        y[b, r, q_] = yv
        if mv is not None:
            mu[b, r, q_] = f32(mv)
        with np.errstate(invalid='ignore'):
            if np.isnan(f32(yv) - mu[b, r, q_]).any():
                nan_px.append((b, r, q_))
    q, yh = oracle.quantize_center(y, mu, GAIN)
    q0, yh0 = oracle.quantize_center(y)
    for p, want_q in ties:
        assert (q[p] == want_q).all(), (p, q[p], want_q)
    assert len(nan_px) >= 3
    for p in nan_px:
        assert (q[p] == 0).all() and np.isnan(yh[p]).all()
    assert (q == 256).any() and (q == -256).any() and np.isnan(yh).any() and np.isinf(yh).any()
    assert ((yh0 == 0) & np.signbit(yh0)).any() and ((yh0 == 0) & ~np.signbit(yh0)).any()
    q_ext = q.copy()
    q_ext[0, 0, 0], q_ext[0, 0, 1], q_ext[1, 0, 0], q_ext[1, 0, 1] = 32767, -32768, 256, -256
    per = lambda f, *a: np.stack([f(*[t[i:i + 1] for t in a], GAIN_ROWS[i])[0] for i in range(n)])
    qr = np.stack([oracle.quantize_center(y[i:i + 1], mu[i:i + 1], GAIN_ROWS[i])[0][0] for i in range(n)])
    yhr = np.stack([oracle.quantize_center(y[i:i + 1], mu[i:i + 1], GAIN_ROWS[i])[1][0] for i in range(n)])
    want = {'gain': oracle.channel_gain(y, GAIN), 'gain_none': oracle.channel_gain(y, None), 'q': q, 'yh': yh, 'q0': q0, 'yh0': yh0, 'q_only': q,
            'deq': oracle.dequantize(q_ext, mu, GAIN), 'deq0': oracle.dequantize(q_ext),
            'gain_rows': per(oracle.channel_gain, y), 'q_rows': qr, 'yh_rows': yhr, 'deq_rows': per(oracle.dequantize, q_ext, mu)}
    assert np.array_equal(qr, q)  # (the gain does not reach q)

    def call(ops, d):
        out = {'gain': ops.channel_gain(d['y'], d['gain']), 'gain_none': ops.channel_gain(d['y'], None)}
        out['q'], out['yh'] = ops.quantize_center(d['y'], d['mu'], d['gain'])
        out['q0'], out['yh0'] = ops.quantize_center(d['y'])
        out['q_only'], none = ops.quantize_center(d['y'], d['mu'], d['gain'], want_yhat=False)
        assert none is None
        out['deq'] = ops.dequantize(d['q_ext'], d['mu'], d['gain'])
        out['deq0'] = ops.dequantize(d['q_ext'])
        out['gain_rows'] = ops.channel_gain_rows(d['y'], d['gains'])
        out['q_rows'], out['yh_rows'] = ops.quantize_center_rows(d['y'], d['mu'], d['gains'])
        out['deq_rows'] = ops.dequantize_rows(d['q_ext'], d['mu'], d['gains'])
        return out
    return Case({'y': y, 'mu': mu, 'gain': GAIN, 'gains': GAIN_ROWS, 'q_ext': q_ext}, call, want, eq_all)


LOG_VAR_MIN, LOG_VAR_MAX = f32(-18.4207), f32(10.0)  # the clamp constants of hyper_params


def hyper_params_regime_case(oracle, seed=0):
    """lv at NaN, +-inf, -0 and the 4 floats on each side of both clamp constants.  Reach: sigma holds a NaN (the clamp's comparisons
    pass one), both ends of its range, and values strictly inside next to either end"""
    rng = np.random.default_rng(seed)
    hs = (rng.standard_normal((1, 6, 9, 16), dtype=f32) * f32(8)).astype(f32)
    vals = np.concatenate([np.array([NAN, INF, -INF, -0.0], f32), around(LOG_VAR_MIN), around(LOG_VAR_MAX)])
    spots = [(r, q, ch) for r in range(5) for q in range(7) for ch in range(8, 16)]
    for v, i in zip(vals, rng.permutation(len(spots))):
        r, q, ch = spots[i]
        hs[0, r, q, ch] = v
    hs[0, 0, 0, :8] = [NAN, INF, -INF, -0.0, TINY, -TINY, BIG, -BIG]  # (mu is a copy)
    mu, sg = oracle.hyper_params(hs, 8, 5, 7)
    lo, hi = sigma_range(oracle)
    assert np.isnan(sg).any() and (sg == lo).sum() >= 6 and (sg == hi).sum() >= 6
    assert ((sg > lo) & (sg < lo * f32(1.00001))).any() and ((sg < hi) & (sg > hi * f32(0.99999))).any()
    assert lo <= np.nanmin(sg) and np.nanmax(sg) <= hi

    def call(ops, d):
        m, s = ops.hyper_params(d['hs'], 8, 5, 7)
        return {'mu': m, 'sigma': s}
    return Case({'hs': hs}, call, {'mu': mu, 'sigma': sg}, eq_all)


GAIN_INTERP_VALUES = np.array([0.0, -0.0, 1e-45, 1e-40, np.inf, np.nan, -1.5, 2.0, 2.0 ** -126], f32)
GAIN_INTERP_LAMBDAS = [0.0, 1.0, 0.3]


def gain_interp_regime_case(oracle, lam):
    """every pair of GAIN_INTERP_VALUES.  Reach: at lam = 1 the result is |g_r| by bits (x^1 * y^0 = x * 1), at lam = 0 |g_t|
    (a NaN matching a NaN); at 0.3 zeros and non-zero values both occur"""
    g_r, g_t = (a.reshape(-1).copy() for a in np.meshgrid(GAIN_INTERP_VALUES, GAIN_INTERP_VALUES, indexing='ij'))
    want = oracle.gain_interp(g_r, g_t, lam)
    if lam in (0.0, 1.0):
        g = g_r if lam == 1.0 else g_t
        src = np.where(g < 0, -g, g)  # (the header's |g|: `g < 0 ? -g : g` keeps a -0.0)
        assert ((want.view(np.uint32) == src.view(np.uint32)) | (np.isnan(want) & np.isnan(src))).all()
    else:
        assert (want == 0).any() and (want != 0).any()
    return Case({'g_r': g_r, 'g_t': g_t}, lambda ops, d: ops.gain_interp(d['g_r'], d['g_t'], lam), want)


def _plant_nonfinite_and_subnormal(x):
    """planted() of tests/numeric_regimes.py (+inf, two NaN, -inf) and a 2 x 2 block of subnormals of both signs, in place"""
    n, h, w, c = x.shape
    for i, r, q, ch, v in planted(x.shape):
        x[i, r, q, ch] = v
    x[n - 1, 0:2, 2:4, :] = np.array([TINY, -TINY, f32(3e-39), -0.0], f32).reshape(2, 2, 1)
    return x


def downsample2x_regime_cases(oracle, seed=0):
    """2 x 2 means over planted non-finite values and subnormals (0.5f * 1e-45f rounds to a zero).  Reach: a non-finite mean only
    where its block holds a non-finite value, some of them, and a subnormal or zero mean from the subnormal block"""
    h, w = 5, 7
    x = _plant_nonfinite_and_subnormal(np.random.default_rng(seed).standard_normal((2, h, w, 6), dtype=f32))
    cases = []
    for ch0, nch in ((1, 2), (0, 6), (5, 1)):
        want = oracle.downsample2x(x, ch0, nch)
        blocks = (~np.isfinite(x[:, :h // 2 * 2, :w // 2 * 2, ch0:ch0 + nch])).reshape(2, h // 2, 2, w // 2, 2, nch).any(axis=(2, 4))
        bad = ~np.isfinite(want)
        assert np.array_equal(bad, np.transpose(blocks, (0, 3, 1, 2))) and (bad.any() or (ch0, nch) == (5, 1))
        assert (np.abs(want[1, :, 0, 1]) < f32(2.0 ** -126)).all()
        cases.append(Case({'x': x}, lambda ops, d, ch0=ch0, nch=nch: ops.downsample2x(d['x'], ch0, nch), want))
    return cases


def pad_channels_regime_case(oracle, seed=0):
    x = _plant_nonfinite_and_subnormal(np.random.default_rng(seed).standard_normal((2, 5, 7, 3), dtype=f32))
    want = oracle.pad_channels(x, 8)
    assert np.array_equal(want[..., :3].view(np.uint32), x.view(np.uint32)) and not want[..., 3:].any() and not np.signbit(want[..., 3:]).any()
    return Case({'x': x}, lambda ops, d: ops.pad_channels(d['x'], 8), want)


GDN_BOUNDS = (f32(1e-3), f32(2.0 ** -18), f32(2.0 ** -36))  # beta_bound, gamma_bound, pedestal (as latent_ops_case)


def gdn_reparam_regime_case(oracle, seed=0):
    """beta and gamma at the 4 floats on each side of their bounds, NaN, +-inf, -0 and subnormals.  Reach: what is at or below
    the bound (a NaN too: `v > bound ? v : bound`) gives bound^2 - pedestal, the floats above it give more, +inf gives +inf"""
    rng = np.random.default_rng(seed)
    c = 8
    bb, gb, ped = GDN_BOUNDS
    extra = np.array([NAN, INF, -INF, -0.0, TINY, -TINY], f32)
    beta = np.abs(rng.standard_normal(c)).astype(f32)
    gamma = (rng.standard_normal((c, c)) * 0.1).astype(f32)
    bvals, gvals = np.concatenate([around(bb), extra]), np.concatenate([around(gb), extra])
    beta[:] = bvals[rng.permutation(bvals.size)[:c]]
    beta[0], beta[1], beta[2] = NAN, INF, np.nextafter(bb, f32(1))
    gamma.reshape(-1)[rng.permutation(c * c)[:gvals.size]] = gvals
    be, ge = oracle.gdn_reparam(beta, gamma, float(bb), float(gb), float(ped))
    floor_b, floor_g = bb * bb - ped, gb * gb - ped
    assert be[0] == floor_b and be[1] == INF and be[2] > floor_b
    with np.errstate(invalid='ignore'):
        low = ~(gamma > gb)
    assert (ge[low] == floor_g).all() and (ge[~low] > floor_g).all() and np.isinf(ge).sum() == 1 and low.sum() >= 10
    return Case({'beta': beta, 'gamma': gamma},
                lambda ops, d: dict(zip(('be', 'ge'), ops.gdn_reparam(d['beta'], d['gamma'], float(bb), float(gb), float(ped)))),
                {'be': be, 'ge': ge}, eq_all)


# ---- sigma sets of the entropy model and the rate estimates ----------------------------------------------------------------------
def sigma_range(oracle):
    """(lowest, highest) sigma hyper_params can return: exp(lv / 2) at its two clamp constants"""
    hs = np.zeros((1, 1, 2, 2), f32)
    hs[0, 0, :, 1] = [-INF, INF]
    sg = oracle.hyper_params(hs, 1, 1, 2)[1].reshape(-1)
    return sg[0], sg[1]


def sigma_sets(oracle):
    """S_REACH: what hyper_params can hand the entropy model at the edge of its range and around it -- a NaN (its clamp passes
    one) and the 4 floats on each side of both ends.  S_API: what the API accepts beyond it and can still be coded.
    S_OUT: sigmas whose cdf leaves [0, 1]: defined rows, not codable (they do not increase)"""
    lo, hi = sigma_range(oracle)
    return {'S_REACH': np.concatenate([np.array([NAN], f32), around(lo), around(hi)]),
            'S_API': np.array([1e-45, 1e-38, 2.0 ** -126, 1e-6, 1e3, 1e4, 3e38, np.inf], f32),
            'S_OUT': np.array([0.0, -0.0, -1.0, -np.inf], f32)}


SIGMA_SETS = ('S_REACH', 'S_API', 'S_OUT')
ENTROPY_SHAPE, ENTROPY_MAPS = (1, 9, 13, 6), [0, 2, 5]  # 351 positions in stream order: 5 whole wavefronts and one of 31 valid lanes


def sigma_layout(rng, special):
    """sigma per stream position, laid out over the wavefronts of the windows kernel as saturation_threshold_case lays its band out:
      0: ordinary lanes (sigma in [0.5, 2]), every special value ALONE among them, three lanes apart
      1: the special values in turn            2: every lane the first special value      3: every lane the last one
      4: lanes that saturate the outer chunks (sigma 0.01), one special value among them
      5 (31 valid lanes): the special values in turn"""
    per_pos = rng.uniform(0.5, 2.0, 351).astype(f32)
    assert special.size * 3 <= 64
    per_pos[np.arange(special.size) * 3 + 1] = special
    per_pos[64:128] = special[np.arange(64) % special.size]
    per_pos[128:192] = special[0]
    per_pos[192:256] = special[-1]
    per_pos[256:320] = f32(0.01)
    per_pos[256 + 37] = special[len(special) // 2]
    per_pos[320:] = special[(np.arange(31) + 3) % special.size]
    return per_pos


def sigma_regime_case(oracle, name, seed=0):
    """laplace_cdf_rows, laplace_cdf_windows (single and _batch) and laplace_bounds over sigma_layout of the set `name`.  Over S_REACH
    and S_API also a stream the ORACLE encodes from these rows, with symbols inside and outside the 64-entry window, decoded from
    the oracle's rows and from the device's windows + sigma_pos (the decoder's slow path rebuilds the rows from sigma_pos).
    Reach (S_REACH, S_API): entries 0..512 of every row of the oracle increase strictly -- the rows can be coded; the oracle's
    own decoders, from rows and from windows, return the symbols.  Always: windows == the slice of the rows."""
    rng = np.random.default_rng(seed)
    (_, h, w, c), maps = ENTROPY_SHAPE, ENTROPY_MAPS
    npix = h * w
    special = sigma_sets(oracle)[name]
    per_pos = sigma_layout(rng, special)
    sig = rng.uniform(0.5, 2.0, ENTROPY_SHAPE).astype(f32)
    sig.reshape(npix, c)[:, maps] = per_pos.reshape(len(maps), npix).T  # position = map * npix + pixel
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * 2.0), -256, 255).astype(np.int16)
    q.reshape(-1)[::7] = np.array([33, -33, 40, -34, 32, -32, 31, 256, -256, 255, 100], np.int16)[np.arange(q.size)[::7] % 11]
    rows = oracle.laplace_cdf_rows(sig, maps)
    win, sp = oracle.laplace_cdf_windows(sig, maps)
    bounds = oracle.laplace_bounds(sig, q, maps)
    assert np.array_equal(sp.view(np.uint32), per_pos.view(np.uint32))
    np.testing.assert_array_equal(win, rows[:, abi.CDF_WIN0:abi.CDF_WIN0 + abi.CDF_WIN])
    want = {'rows': rows, 'win': win, 'sp': sp, 'win_b': win, 'sp_b': sp, 'bounds': bounds}
    coded = name != 'S_OUT'
    payload = sym = None
    if coded:
        assert (np.diff(rows[:, :2 * abi.AC_MAX_VAL + 1].astype(np.int64), axis=1) > 0).all()
        payload = oracle.range_encode(bounds)
        sym = (q.reshape(npix, c)[:, maps].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16)
        np.testing.assert_array_equal(oracle.range_decode(payload, rows, per_pos.size), sym)
        np.testing.assert_array_equal(oracle.range_decode_windows(payload, win, sp, per_pos.size), sym)
        inside = np.abs(sym.astype(np.int32) - 256) <= 30
        assert inside.any() and (~inside).any()
        want.update(sym=sym, sym_w=sym)

    def call(ops, d):
        import torch
        out = {'rows': ops.laplace_cdf_rows(d['sig'], maps), 'bounds': ops.laplace_bounds(d['sig'], d['q'], maps)}
        out['win'], out['sp'] = ops.laplace_cdf_windows(d['sig'], maps)
        out['win_b'] = torch.zeros((per_pos.size, abi.CDF_WIN), dtype=torch.int16, device=d['sig'].device)
        out['sp_b'] = torch.zeros(per_pos.size, dtype=torch.float32, device=d['sig'].device)
        ops.laplace_cdf_windows_batch(d['sig'], [maps], (out['win_b'], out['sp_b']))
        if coded:
            (out['sym'],) = ops.range_decode([payload], d['rows'], [0], [per_pos.size], [0])
            (out['sym_w'],) = ops.range_decode([payload], out['win'], [0], [per_pos.size], [0], sigma_pos=out['sp'])
        return out
    return Case({'sig': sig, 'q': q, 'rows': _i16(rows)}, call, want, eq_all, per_pos=per_pos, special=special, coded=coded)


RATE_P_MIN, RATE_P_MAX = 2.0 ** -16, 1.0


def rate_regime_case(oracle, seed=0):
    """laplace_prob (with and without mu), table_prob, rate_bits and bounds_rate over the three sigma sets together, y at NaN, +-inf,
    non-integers and +-257, p at 0, NaN, p_min, p_max, the floats around both and beyond.  rate_bits runs on the planted p (a NaN
    total) and on the oracle's finite laplace_prob values; every total is compared by bits (total_bits: a NaN matches a NaN).
    Reach: laplace_prob holds NaN, zeros and values inside (0, 1]; table_prob is NaN exactly at the y that are not whole
    numbers of [-256, 256]; the rates of the planted p hold NaN, both ends 16 and 0, and values between"""
    rng = np.random.default_rng(seed)
    sets = sigma_sets(oracle)
    special = np.concatenate([sets[k] for k in SIGMA_SETS])
    shape = (2, 4, 5, 8)  # [b, c, h, w]
    y = np.rint(rng.standard_normal(shape) * 6).astype(f32)
    mu = rng.standard_normal(shape).astype(f32)
    sigma = np.exp(rng.uniform(-3, 3, shape)).astype(f32)
    flat = rng.permutation(y.size)
    sigma.reshape(-1)[flat[:2 * special.size]] = np.concatenate([special, special])
    yvals = np.array([NAN, INF, -INF, 0.5, -3.25, 257.0, -257.0, 256.0, -256.0, -0.0, TINY], f32)
    y.reshape(-1)[flat[special.size:special.size + yvals.size]] = yvals  # (over special sigmas) ...
    y.reshape(-1)[flat[-yvals.size:]] = yvals                              # ... and over ordinary ones
    params = (rng.standard_normal((shape[1], abi.BALLE_PARAMS)) * 0.8).astype(f32)
    _, cdf = oracle.balle_cdf_table(params)
    p_mu, p_zero, p_z = oracle.laplace_prob(y, mu, sigma), oracle.laplace_prob(y, None, sigma), oracle.table_prob(y, cdf)
    assert np.isnan(p_zero).any() and (p_zero == 0).any() and ((p_zero > 0) & (p_zero <= 1)).any()
    whole = (y >= -256) & (y <= 256) & (np.rint(y) == y)
    assert np.array_equal(np.isnan(p_z), ~whole) and (~whole).sum() >= 2 * 7
    pmin, pmax = f32(RATE_P_MIN), f32(RATE_P_MAX)
    p = np.concatenate([np.array([0.0, -0.0, NAN, -1.0, 2.0, 1e-30, TINY, INF, -INF], f32), around(pmin, 2), around(pmax, 2),
                        rng.random(40, dtype=f32)])
    p_fin = np.where(np.isnan(p_zero), f32(0.25), p_zero).astype(f32)
    rate_p, total_p = oracle.rate_bits(p, RATE_P_MIN, RATE_P_MAX)
    rate_f, total_f = oracle.rate_bits(p_fin, RATE_P_MIN, RATE_P_MAX)
    assert np.isnan(total_p) and np.isfinite(total_f)
    assert np.isnan(rate_p).any() and (rate_p == 16).any() and (rate_p == 0).any() and ((rate_p > 0) & (rate_p < 16)).any()
    sg4 = np.ascontiguousarray(np.transpose(sigma, (0, 2, 3, 1)))  # NHWC for the bounds
    qb = np.clip(np.rint(rng.standard_normal(sg4.shape) * 40), -256, 256).astype(np.int16)
    with np.errstate(invalid='ignore'):
        qb[sg4 <= 0] = 0  # (S_OUT: the symbol across the centre of the row, whose bounds come out in the wrong order)
    bnd = np.concatenate([oracle.laplace_bounds(sg4[i:i + 1], qb[i:i + 1], list(range(shape[1]))) for i in range(shape[0])])
    lo, hi16 = bnd & 0xFFFF, bnd >> 16
    assert ((hi16 != 0) & (hi16 <= lo)).any()  # (the rows of S_OUT do not increase: priced as the smallest probability)
    total_b = oracle.bounds_rate(bnd)
    assert np.isfinite(total_b)
    want = {'p_mu': p_mu, 'p_zero': p_zero, 'p_z': p_z, 'rate_p': rate_p, 'rate_f': rate_f}
    totals = {'total_p': total_bits(total_p), 'total_f': total_bits(total_f), 'total_b': total_bits(total_b)}

    def call(ops, d):
        out = {'p_mu': ops.laplace_prob(d['y'], d['mu'], d['sigma']), 'p_zero': ops.laplace_prob(d['y'], None, d['sigma']),
               'p_z': ops.table_prob(d['y'], d['cdf'])}
        out['rate_p'], out['total_p'] = ops.rate_bits(d['p'], RATE_P_MIN, RATE_P_MAX)
        out['rate_f'], out['total_f'] = ops.rate_bits(d['p_fin'], RATE_P_MIN, RATE_P_MAX)
        out['total_b'] = ops.bounds_rate(d['bnd'])
        return out

    def compare(out, want):
        eq_all({k: v for k, v in out.items() if not k.startswith('total')}, want)
        for k, bits in totals.items():
            got = total_bits(float(out[k].cpu()))
            assert got == bits, (k, got, bits)
    return Case({'y': y, 'mu': mu, 'sigma': sigma, 'cdf': cdf, 'p': p, 'p_fin': p_fin, 'bnd': _i32(bnd)}, call, want, compare)


# ---- the table of regime cases: what the plain GPU test and the guarded harness both run ------------------------------------------
def _b(f, *a, **kw):
    return lambda oracle: f(oracle, *a, **kw)


REGIME_CASES = {}
for _name in FLOWS:
    for _shape in WARP_REGIME_SHAPES:
        REGIME_CASES['warp-%s-%dx%dx%d' % ((_name,) + _shape)] = _b(warp_regime_case, _name, _shape, 11)
REGIME_CASES['warp-image-2x5x7'] = _b(warp_image_case, (2, 5, 7), 12)
for _name in FLOWS:
    for _size in BLEND_SIZES:
        for _ft in (1, 2):  # P, B
            for _kind, _kw in (('fast', {}), ('general', {'general': True}), ('rows', {'rows': (2, 3)})):
                REGIME_CASES['warp_blend-%s-%dx%d-ft%d-%s' % (_name, _size[0], _size[1], _ft, _kind)] = _b(
                    warp_blend_regime_case, _name, _size, _ft, seed=13, **_kw)
for _size in FRAME_REGIME_SIZES:
    for _skip in (False, True):
        for _fl in (True, False):
            REGIME_CASES['frame_to_yuv420-%dx%d-%s-%s' % (_size[0], _size[1], 'skip' if _skip else 'noskip', 'float' if _fl else 'bytes')] = _b(
                frame_regime_case, _size, _size == (10, 14), _skip, _fl, seed=14)
for _size in FRAME_REGIME_SIZES[:2]:
    REGIME_CASES['frame_to_yuv420-%dx%d-ties' % _size] = _b(frame_ties_case, _size, _size == (10, 14), seed=14)
REGIME_CASES['latent'] = _b(latent_regime_case, seed=15)
REGIME_CASES['hyper_params'] = _b(hyper_params_regime_case, seed=16)
for _lam in GAIN_INTERP_LAMBDAS:
    REGIME_CASES['gain_interp-%g' % _lam] = _b(gain_interp_regime_case, _lam)
for _i in range(3):
    REGIME_CASES['downsample2x-%d' % _i] = (lambda i: lambda oracle: downsample2x_regime_cases(oracle, 17)[i])(_i)
REGIME_CASES['pad_channels'] = _b(pad_channels_regime_case, seed=18)
REGIME_CASES['gdn_reparam'] = _b(gdn_reparam_regime_case, seed=19)
for _name in SIGMA_SETS:
    REGIME_CASES['sigma-%s' % _name] = _b(sigma_regime_case, _name, seed=20)
REGIME_CASES['rate'] = _b(rate_regime_case, seed=21)

# Ops or sigma values that could not be held by bits: (case id, the sentence of include/aivc_hip.h behind the exception).  The
# analogue of ZERO_SIGN_OPEN in tests/numeric_regimes.py; empty: every case above is compared bit for bit.
NOT_HELD_BY_BITS = []
