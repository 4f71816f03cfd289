"""The CPU oracle against a plain restatement of the arithmetic contract (include/aivc_hip.h) in EXACT arithmetic, under every
numeric regime of tests/numeric_regimes.py: tests/test_gpu_contract_regimes.py trusts the oracle where operands and partial sums
are subnormal, chains underflow to signed zeros or overflow midway, and operands are infinite or NaN; this pins it there.

fma32(a, b, c) is the exact a * b + c in Python integers (every fp32 number is a multiple of 2^-149, every product one of
2^-298), rounded once to the nearest fp32, ties to even: gradual underflow, overflow to +-inf, the IEEE sign of an exact zero
(-0 only if the product and c are both negative zeros; +0 for an exact cancellation) and the IEEE rules for non-finite
operands.  No C and no numpy float arithmetic takes part in a chain.  The chains are the header's, term by term:

  tap chain   kk = t * c_in + ci over the taps in (ky, kx) order, in groups of 8 in AIVC_K_ORDER, the last group zero padded
              (a term +0 * +0); transposed: the taps of the pixel's parity class, an out-of-image tap a zero input in its place;
              v = acc + bias; leaky, relu, mul, res
  version 2   F(2x2, 3x3) exactly as written: R_i, V_p, M_p over ci in groups of 8, S0 + S1 with the zero coefficients skipped
              and one addition or subtraction per term, U from oracle.winograd_weights

At two dozen output positions per case (the four corners, every edge, interior pixels, the pixels around each planted special
value) a few channels are compared with oracle.conv2d by detmath_cases.same_bits.  The polyphase and class forms (302 / 303)
keep their fp64 and weight-transform checks (tests/test_oracle_winograd.py)."""
import math

import numpy as np
import pytest

from aivc_amd import abi
from numeric_regimes import REGIMES, assert_bits, planted, row_facts

INF = math.inf


def _units(a):
    """a finite fp32 number (a Python float) in units of 2^-149"""
    return int(math.ldexp(a, 149))


def round32(s, unit):
    """the integer s != 0 in units of 2^-unit -> the nearest fp32 number, ties to even"""
    n = abs(s)
    shift = max(unit - 149, n.bit_length() - 24)
    if shift > 0:
        q, rem = n >> shift, n & ((1 << shift) - 1)
        half = 1 << (shift - 1)
        if rem > half or (rem == half and (q & 1)):
            q += 1
    else:
        q = n << -shift
    if q.bit_length() + shift - unit > 128:
        return -INF if s < 0 else INF
    return math.copysign(math.ldexp(q, shift - unit), s)


def fma32(a, b, c):
    if a != a or b != b or c != c:
        return math.nan
    if abs(a) == INF or abs(b) == INF:
        if a == 0 or b == 0:
            return math.nan
        p = math.copysign(INF, a) * math.copysign(1.0, b)
        return math.nan if (abs(c) == INF and c != p) else p
    if abs(c) == INF:
        return c
    ia, ib = _units(a), _units(b)
    if ia == 0 or ib == 0:
        if c != 0:
            return c
        neg = (math.copysign(1.0, a) * math.copysign(1.0, b) < 0) and math.copysign(1.0, c) < 0
        return -0.0 if neg else 0.0
    s = ia * ib + (_units(c) << 149)
    return 0.0 if s == 0 else round32(s, 298)


def add32(a, b):
    return fma32(1.0, a, b)


def test_fma32_against_ieee_cases():
    """the exact fma on cases worked by hand: rounding at a tie, gradual underflow, overflow, signed zeros, non-finite operands"""
    f = lambda e: math.ldexp(1.0, e)  # noqa: E731
    bits = lambda v: np.float32(v).view(np.uint32)  # noqa: E731
    cases = [
        ((1.0 + f(-23), 1.0 + f(-23), 0.0), 1.0 + f(-22)),            # 1 + 2^-22 + 2^-46 rounds down
        ((1.0 + f(-12), 1.0 + f(-12), 0.0), 1.0 + f(-11)),            # 1 + 2^-11 + 2^-24: a tie, to even
        ((1.0 + f(-12), 1.0 + f(-12), -1.0), f(-11) + f(-24)),        # ... and the fma keeps the 2^-24 a rounded product loses
        ((1.0, 1.0, f(-24)), 1.0),                                    # a tie goes to even
        ((1.0 + f(-23), 1.0, f(-24)), 1.0 + f(-22)),
        ((f(-75), f(-75), 0.0), 0.0), ((-f(-75), f(-75), 0.0), -0.0),  # 2^-150 is a tie between 0 and 2^-149: to even, with the sign
        ((f(-75), 1.5 * f(-75), 0.0), f(-149)),
        ((f(-64), f(-64), f(-149)), f(-128) + f(-149)),
        ((f(-126), 0.75, 0.0), 0.75 * f(-126)), ((f(-149), 0.5, 0.0), 0.0), ((f(-149), 0.75, 0.0), f(-149)),
        ((f(100), f(27), f(127)), INF), ((-f(100), f(28), 0.0), -INF), ((f(127), 1.0, f(127) * (1 - f(-24))), INF),
        ((f(127), 1.0, f(127) * (1 - f(-23))), f(128) - f(104)),
        ((0.0, 3.0, -0.0), 0.0), ((0.0, -3.0, -0.0), -0.0), ((-0.0, 3.0, 0.0), 0.0), ((0.0, 0.0, -0.0), 0.0), ((2.0, 3.0, -6.0), 0.0),
        ((0.0, 3.0, -5.0), -5.0), ((INF, 0.0, 1.0), math.nan), ((INF, 2.0, -INF), math.nan), ((INF, -2.0, -INF), -INF),
        ((1.0, 2.0, INF), INF), ((math.nan, 0.0, 0.0), math.nan), ((-INF, -1.0, 5.0), INF),
    ]
    for args, want in cases:
        got = fma32(*args)
        assert bits(got) == bits(want) or (got != got and want != want), (args, got, want)
    # and against the host's own single rounding where a double holds the exact result
    rng = np.random.default_rng(3)
    a, b = (rng.standard_normal(2000).astype(np.float32) for _ in range(2))
    for x, y in zip(a.tolist(), b.tolist()):
        assert bits(fma32(x, y, 0.0)) == bits(np.float32(np.float64(x) * np.float64(y)))
        lo = float(np.float32(x) * np.float32(2.0 ** -126))  # a subnormal operand, a subnormal product
        assert bits(fma32(lo, y, 0.0)) == bits(np.float32(np.float64(lo) * np.float64(y)))


K_ORDER = [0, 4, 1, 5, 2, 6, 3, 7]
assert K_ORDER == [((i & 1) << 2) | (i >> 1) for i in range(8)]  # AIVC_K_ORDER


def act32(act, v):
    if act == abi.ACT_LEAKY:
        return v if v > 0 else fma32(v, float(np.float32(0.01)), -0.0)
    if act == abi.ACT_RELU:
        return v if v > 0 else 0.0
    assert act == abi.ACT_NONE
    return v


def epilogue(acc, i, n, oy, ox, co, a1, a2):
    v = acc if i['bias'] is None else add32(acc, float(i['bias'][co]))
    v = act32(a1, v)
    if i.get('mul') is not None:
        v = fma32(float(i['mul'][n, oy, ox, co]), v, -0.0)
    if i.get('res') is not None:
        v = add32(v, float(i['res'][n, oy, ox, co]))
    return act32(a2, v)


def tap_chain(x, w, mode, k, s, pad, n, oy, ox, co):
    """the accumulator of output (n, oy, ox, co): the contract's chain, zero terms included"""
    h, wd, ci = x.shape[1:]
    terms = []  # (input value, weight) in kk order
    if mode == abi.MODE_TCONV:
        tpad = (k + 1) // 2 - 1
        taps = [(ky, kx) for ky in range((oy + tpad) & 1, k, 2) for kx in range((ox + tpad) & 1, k, 2)]
    else:
        taps = [(ky, kx) for ky in range(k) for kx in range(k)]
    for ky, kx in taps:
        if mode == abi.MODE_TCONV:
            ty, tx = oy + tpad - ky, ox + tpad - kx
            iy, ix = ty >> 1, tx >> 1
            px = x[n, iy, ix] if (ty >= 0 and tx >= 0 and iy < h and ix < wd) else None  # out of the image: zero inputs in place
        else:
            px = x[n, min(max(oy * s + ky - pad, 0), h - 1), min(max(ox * s + kx - pad, 0), wd - 1)]
        wk = w[co, ky, kx]
        terms += [(0.0 if px is None else float(px[c]), float(wk[c])) for c in range(ci)]
    terms += [(0.0, 0.0)] * (-len(terms) % 8)  # the last group zero padded
    acc = 0.0
    for g in range(0, len(terms), 8):
        for e in K_ORDER:
            a, b = terms[g + e]
            acc = fma32(a, b, acc)
    return acc


WINO_A, WINO_B, WINO_S = (0, 1, 2, 1), (2, 2, 1, 3), (-1.0, 1.0, -1.0, -1.0)
WINO_T = ((1, 1, 1, 0), (0, 1, -1, -1))


def wino_u_index(co, p, ci, c_in):
    """AIVC_WINO_U_INDEX"""
    return (((((co // 64) * (c_in // 8) + ci // 8) * 16 + p) * 2 + (ci % 8) // 4) * 64 + co % 64) * 4 + ci % 4


def wino_tile_v(x, n, ty, tx):
    """V_p[ci] of tile (ty, tx), p = 0..15: rows first, then columns"""
    h, wd, ci = x.shape[1:]
    d = [[x[n, min(max(2 * ty - 1 + r, 0), h - 1), min(max(2 * tx - 1 + c, 0), wd - 1)].tolist() for c in range(4)] for r in range(4)]
    v = []
    for i in range(4):
        r_i = [[fma32(WINO_S[i], d[WINO_B[i]][c][ch], d[WINO_A[i]][c][ch]) for ch in range(ci)] for c in range(4)]
        for j in range(4):
            v.append([fma32(WINO_S[j], r_i[WINO_B[j]][ch], r_i[WINO_A[j]][ch]) for ch in range(ci)])
    return v


def wino_acc(v, u, co, a, b, c_in):
    half = []
    for p0 in (0, 8):
        sh = 0.0
        for p in range(p0, p0 + 8):
            cf = WINO_T[a][p >> 2] * WINO_T[b][p & 3]
            if not cf:
                continue
            m = 0.0
            for g in range(0, c_in, 8):
                for e in K_ORDER:
                    m = fma32(v[p][g + e], float(u[wino_u_index(co, p, g + e, c_in)]), m)
            sh = add32(sh, m) if cf > 0 else fma32(-1.0, m, sh)
        half.append(sh)
    return add32(half[0], half[1])


ROWS = [
    # form, mode, k, stride, pad, c_in, c_out, (n, h, w), act1, act2, bias, mul, res
    ('conv', abi.MODE_CONV, 1, 1, 0, 8, 8, (2, 6, 10), abi.ACT_RELU, 0, True, True, True),
    ('conv', abi.MODE_CONV, 3, 1, 1, 32, 32, (1, 9, 11), abi.ACT_LEAKY, 0, True, False, True),
    ('conv', abi.MODE_CONV, 5, 2, 2, 12, 64, (2, 13, 17), 0, abi.ACT_LEAKY, True, False, False),  # c_in not a multiple of 8
    ('tconv', abi.MODE_TCONV, 5, 2, 0, 8, 6, (2, 7, 9), abi.ACT_LEAKY, 0, True, True, False),
    ('tconv', abi.MODE_TCONV, 3, 2, 0, 32, 64, (2, 5, 6), 0, 0, True, False, True),
    ('wino', abi.MODE_CONV, 3, 1, 1, 32, 128, (1, 7, 9), abi.ACT_LEAKY, 0, True, False, True),
]


def positions(n, ho, wo, scale, specials):
    """about two dozen (image, oy, ox): corners, edges, interior, and the outputs around each planted special (input pixel
    (i, y, x) maps to output pixel scale * (y, x))"""
    out = []
    for i in sorted({0, n - 1}):
        out += [(i, 0, 0), (i, 0, wo - 1), (i, ho - 1, 0), (i, ho - 1, wo - 1), (i, 0, wo // 2), (i, ho - 1, wo // 3), (i, ho // 2, 0),
                (i, ho // 3, wo - 1), (i, ho // 2, wo // 2), (i, ho // 2 - 1, wo // 2 + 1)]
    for i, y, x in specials:
        cy, cx = int(y * scale), int(x * scale)
        out += [(i, min(max(cy + dy, 0), ho - 1), min(max(cx + dx, 0), wo - 1)) for dy, dx in ((0, 0), (-1, 1), (1, -1), (2, 2))]
    return list(dict.fromkeys(out))[:28]


@pytest.mark.parametrize('regime', REGIMES, ids=repr)
@pytest.mark.parametrize('row', ROWS, ids=lambda r: '%s-k%d-s%d-%dto%d' % (r[0], r[2], r[3], r[5], r[6]))
def test_oracle_equals_the_exact_chain(row, regime, oracle):
    form, mode, k, s, pad, ci, co, (n, h, w), a1, a2, has_b, has_m, has_r = row
    rng = np.random.default_rng(abs(hash(row[1:7])) % (2 ** 31))
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    x = rng.standard_normal((n, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    drawn = {'x': x, 'w': wt, 'bias': rng.standard_normal(co, dtype=np.float32) if has_b else None,
             'mul': rng.standard_normal((n, ho, wo, co), dtype=np.float32) if has_m else None,
             'res': rng.standard_normal((n, ho, wo, co), dtype=np.float32) if has_r else None}
    rf = row_facts(mode, k, s, pad, a1, a2, variant=301 if form == 'wino' else None)
    i = regime(rng, drawn, rf)
    fixed = dict(mode=mode, stride=s, pad=pad)
    prev, any_size = oracle.set_precision('fp32w' if form == 'wino' else 'fp32'), oracle.WINO_ANY_SIZE
    oracle.WINO_ANY_SIZE = form == 'wino'
    try:
        with np.errstate(all='ignore'):
            want = oracle.conv2d(i['x'], i['w'], i['bias'], mul=i['mul'], res=i['res'], act1=a1, act2=a2, **fixed)
            regime.reach(rf, i, want, lambda: oracle.conv2d(i['x'], i['w'], i['bias'], **fixed))
        u = oracle.winograd_weights(i['w']) if form == 'wino' else None
    finally:
        oracle.WINO_ANY_SIZE = any_size
        oracle.set_precision(prev)
    scale = 2 if mode == abi.MODE_TCONV else 1.0 / s
    specials = [p[:3] for p in planted((n, h, w, ci))]
    for nm in ('res', 'mul'):  # (their planted values sit at output pixels)
        if i[nm] is not None:
            specials += [(int(q[0]), q[1] / scale, q[2] / scale) for q in np.argwhere(~np.isfinite(i[nm]))]
    channels = sorted({0, co // 2, co - 1})
    got, ref, tiles = [], [], {}
    for (img, oy, ox) in positions(n, ho, wo, scale, specials):
        for c in channels:
            if form == 'wino':
                key = (img, oy >> 1, ox >> 1)
                if key not in tiles:
                    tiles[key] = wino_tile_v(i['x'], *key)
                acc = wino_acc(tiles[key], u, c, oy & 1, ox & 1, ci)
            else:
                acc = tap_chain(i['x'], i['w'], mode, k, s, pad, img, oy, ox, c)
            got.append(epilogue(acc, i, img, oy, ox, c, a1, a2))
            ref.append(want[img, oy, ox, c])
    assert_bits(np.array(ref, np.float32), np.array(got, np.float32), '%s under %r (oracle against the exact chain)' % (form, regime))
