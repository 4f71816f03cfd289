"""The numeric regimes of the conv contract beyond N(0, 1), each stated once: what tests/test_contract_regimes.py (the CPU oracle
against exact arithmetic) and tests/test_gpu_contract_regimes.py (every launch kind against the oracle) dress their cases in.
Not a test module.

A regime is a callable  dress(rng, inputs, row) -> inputs  that a builder of tests/conv_cases.py applies to what it has drawn,
before it asks the oracle for `want`.  It rewrites x, w, bias, res, mul and the float image sources; never the 8-bit planes,
never the (I)GDN beta / gamma (in the GDN modes `w` and `bias` ARE gamma and beta and stay).  `row` is the builder's plain
statement of the launch (row_facts below).  After the oracle has run, the builder calls  dress.reach(row, inputs, want, chain):
the CPU-checkable condition ON THE ORACLE'S RESULT that proves the regime was reached, asserted whatever the seed.

Scales are chosen per kind of row so that the oracle alone meets the condition (the draw is x ~ N(0, 1), w ~ N(0, 1) / sqrt(K),
so a chain's result is ~ N(0, 1) * sx * sw):

  * what cannot be scaled is compensated where it can: an 8-bit image source keeps its levels, the scale of x goes into the weight
    columns that read it; a bias / residual of unit scale would bury a subnormal result, so both take the scale of the result;
  * GDN modes: y = x / sqrt(beta + gamma . x^2) follows x alone, so x carries the whole scale;
  * an activation that hides the chain's result -- sigmoid (0.5 at a vanishing argument), relu (+0 for every -0, 0 for a NaN) --
    has the condition asserted on the oracle's result WITHOUT activation, gate and residual (`chain()`), as conv_case does for its
    sigmoid rows; the comparison of the test is always on the full result;
  * graded: the per-channel scales run from below the smallest subnormal (those entries round to +-0: the vanishing terms) up to a
    top placed so that the chain's result straddles 2^-126 (fp32 has no room for 2^-140 .. 2^0 under a subnormal result);
  * overflow, forward GDN: x / sqrt(inf) is a finite 0, so the condition is asserted on the inverse form of the same operands
    (`chain(inverse=True)`: non-finite exactly where the normaliser overflowed); inverse forms: one overflowing square makes the
    normaliser of the whole pixel infinite, so x is scaled to 2^64 / z with z the normal quantile that leaves ~20 % of the pixels
    one; Winograd forms: x up to the largest finite numbers, so that the INPUT TRANSFORM overflows (and gives inf - inf) in
    ~20 % of the tiles, the weights small enough that nothing else does; fused 1x1 tail: 0.6 % of the 64 intermediates
    infinite, i.e. a third of the tail's outputs;
  * nonfinite: fewer than half of the outputs may be touched, so a row of tiny images takes more of them (row['n'])."""
import math

import numpy as np

from aivc_amd import abi
from detmath_cases import same_bits

FLT_MIN = np.float32(2.0 ** -126)


def p2(e):
    return np.float32(2.0 ** e)


def row_facts(mode=abi.MODE_CONV, k=1, stride=1, pad=0, act1=0, act2=0, variant=None, fused_gdn=None, tail=False, plane_cols=()):
    """what a regime needs to know of a launch.  variant: 301 / 302 / 303 for the Winograd forms (tests/conv_cases.py WINO_FORMS),
    fused_gdn: None or the `inverse` flag, plane_cols: the stored input channels that 8-bit planes feed"""
    hidden = act1 in (abi.ACT_SIGMOID, abi.ACT_RELU) or act2 in (abi.ACT_SIGMOID, abi.ACT_RELU)
    gdn_mode = mode in (abi.MODE_GDN, abi.MODE_IGDN)
    inverse = mode == abi.MODE_IGDN or bool(fused_gdn)
    return dict(mode=mode, k=k, stride=stride, pad=pad, variant=variant, gdn_mode=gdn_mode, inverse=inverse,
                forward_gdn_mode=mode == abi.MODE_GDN, tail=tail, plane_cols=tuple(plane_cols), hidden=hidden)


# ---- rewriting the drawn arrays --------------------------------------------------------------------------------------------------
def _mul(a, s):
    with np.errstate(over='ignore', under='ignore', invalid='ignore'):
        return None if a is None else (a * np.asarray(s, np.float32)).astype(np.float32)


def _map_x(d, f):
    """f on x, or on every float image source of d['parts']"""
    if 'parts' in d:
        d['parts'] = [f(p) if isinstance(p, np.ndarray) else p for p in d['parts']]
    else:
        d['x'] = f(d['x'])


def _x_arrays(d):
    return [p for p in d['parts'] if isinstance(p, np.ndarray)] if 'parts' in d else [d['x']]


def _scale(d, row, sx=1.0, sw=1.0, so=None, s3=1.0):
    """x by sx (per stored channel where sx is an array), w by sw and, in the columns that 8-bit planes feed, by sx as well;
    bias, tail bias and residual by so; the tail's weights by s3.  GDN modes: w and bias are gamma and beta and stay."""
    sx = np.asarray(sx, np.float32)
    _map_x(d, lambda a: _mul(a, sx if sx.ndim == 0 else sx[:a.shape[-1]]))
    if not row['gdn_mode']:
        cols = np.ones(d['w'].shape[-1], np.float32)
        for c in row['plane_cols']:
            cols[c] = sx if sx.ndim == 0 else sx[c]
        d['w'] = _mul(_mul(d['w'], sw), cols)
        if so is not None:
            d['bias'] = _mul(d['bias'], so)
    if so is not None:
        d['res'] = _mul(d.get('res'), so)
        if 'b3' in d:
            d['b3'] = _mul(d['b3'], so)
    if 'w3' in d:
        d['w3'] = _mul(d['w3'], s3)
    return d


def _tconv_binade(row):
    """a parity class of a transposed conv holds a quarter of the k x k taps its weights were scaled for: its sums are half as large"""
    return 1 if row['mode'] == abi.MODE_TCONV and row['variant'] is None else 0


def _signed_zeros(rng, a):
    return None if a is None else np.copysign(np.float32(0), rng.standard_normal(a.shape)).astype(np.float32)


def _normal_quantile(p):
    """z with P(|N(0, 1)| > z) = p"""
    lo, hi = 0.0, 10.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if math.erfc(mid / math.sqrt(2.0)) > p else (lo, mid)
    return lo


# ---- fractions of an array -------------------------------------------------------------------------------------------------------
def _frac(mask):
    return float(mask.mean())


def subnormal(a):
    return (a != 0) & (np.abs(a) < FLT_MIN)


def normal(a):
    return np.isfinite(a) & (np.abs(a) >= FLT_MIN)


class Regime:
    name = None

    def __repr__(self):
        return self.name

    def __call__(self, rng, inputs, row):
        d = dict(inputs)
        self.dress(rng, d, row)
        return d

    def fact(self, row, want, chain):
        return chain() if row['hidden'] else want


class SubOperands(Regime):
    """x subnormal or just above (N(0, 1) * 2^-126), w unchanged: results a mix of subnormal and normal"""
    name = 'sub_operands'

    def dress(self, rng, d, row):
        _scale(d, row, sx=p2(-126 + _tconv_binade(row)), so=p2(-126))

    def reach(self, row, inputs, want, chain):
        f = self.fact(row, want, chain)
        assert _frac(subnormal(f)) >= 0.05 and _frac(normal(f)) >= 0.05, (self.name, _frac(subnormal(f)), _frac(normal(f)))


class SubProducts(Regime):
    """x and w both near 2^-64: every product underflows gradually, every result is subnormal"""
    name = 'sub_products'

    def dress(self, rng, d, row):
        if row['gdn_mode']:
            _scale(d, row, sx=p2(-129), so=p2(-129))
        else:
            _scale(d, row, sx=p2(-65), sw=p2(-64), so=p2(-130))

    def reach(self, row, inputs, want, chain):
        f = self.fact(row, want, chain)
        assert _frac(subnormal(f)) >= 0.90, (self.name, _frac(subnormal(f)))


class Graded(Regime):
    """a power-of-two scale per stored input channel of x, in shuffled order, w unchanged: normal, subnormal and vanishing terms
    within one chain (SPAN binades from the top, which lies where the module's docstring says)"""
    name = 'graded'
    SPAN = 40

    def dress(self, rng, d, row):
        ci = _x_arrays(d)[0].shape[-1] if 'parts' not in d else d['w'].shape[-1]
        if row['gdn_mode']:
            e = np.linspace(-149, -118, ci)
        else:
            step = self.SPAN / max(ci - 1, 1)
            top = round(-126 + 0.5 * math.log2(ci * (1.0 - 4.0 ** -step))) + _tconv_binade(row)
            e = np.linspace(top - self.SPAN, top, ci)
        sx = np.exp2(np.round(rng.permutation(e))).astype(np.float32)  # (below 2^-149: 0, the product with x an exact zero)
        if 'parts' in d:  # one source is 4 stored channels of the stack: its own slice of the scales, the planes' in w
            parts, out = d['parts'], []
            for i, p in enumerate(parts):
                out.append(_mul(p, sx[4 * i:4 * i + p.shape[-1]]) if isinstance(p, np.ndarray) else p)
            d['parts'] = out
            cols = np.ones(ci, np.float32)
            for c in row['plane_cols']:
                cols[c] = sx[c]
            d['w'] = _mul(d['w'], cols)
            d['bias'] = _mul(d['bias'], p2(-126))
        else:
            _scale(d, row, sx=sx, so=p2(-126))

    reach = SubOperands.reach


class AllUnderflow(Regime):
    """x and w near 2^-77 (every product below 2^-150 in magnitude, however short the chain: with 2^-75 a chain of 8 terms leaves a
    quarter of its results at +-2^-149), no bias, a residual of signed zeros: every result is a zero whose sign the chain decides.
    kind 'neg_bias': bias all -0.0;  'checker': exact +0 on a checkerboard of x's pixels (squares of 2 x 2, so that a stride-2 chain
    does not always END in a zero term, which leaves no -0) next to the regime's values.
    GDN modes: x itself is signed zeros.  A fused 1x1 tail needs its biases (without them the request is two launches) and
    non-zero intermediates (exact zeros from +0 stay +0): x, w near 2^-30, the tail's weights near 2^-94, both biases -0.0."""

    def __init__(self, kind):
        self.kind = kind
        self.name = 'all_underflow' + {'plain': '', 'neg_bias': '_neg_bias', 'checker': '_checker'}[kind]

    def dress(self, rng, d, row):
        if row['gdn_mode']:
            _map_x(d, lambda a: _signed_zeros(rng, a))
        elif row['tail']:
            _scale(d, row, sx=p2(-30), sw=p2(-30), s3=p2(-94))
        else:
            _scale(d, row, sx=p2(-77), sw=p2(-77))
        if not row['gdn_mode']:
            for nm in ('bias', 'b3'):  # (v + -0.0 is v for every v, both zeros included: what a launch without bias computes)
                if d.get(nm) is not None:
                    d[nm] = np.full_like(d[nm], -0.0) if (row['tail'] or self.kind == 'neg_bias') else None
        d['res'] = _signed_zeros(rng, d.get('res'))
        if self.kind == 'checker':
            def checker(a):
                a = a.copy()
                yy, xx = np.meshgrid(np.arange(a.shape[1]), np.arange(a.shape[2]), indexing='ij')
                a[:, (yy // 2 + xx // 2) % 2 == 0] = 0.0
                return a
            _map_x(d, checker)

    def reach(self, row, inputs, want, chain):
        f = self.fact(row, want, chain)
        zeros = f == 0
        neg = zeros & np.signbit(f)
        assert _frac(zeros) >= 0.90, (self.name, _frac(zeros))
        padded = row['mode'] == abi.MODE_CONV and (row['k'] ** 2 * inputs['w'].shape[-1]) % 8 != 0
        # the tap chains; a Winograd form's S0 + S1 turns a -0 into +0, and so does the zero padding of a last group (K % 8 != 0)
        # ... and the zero pad channel of an image stack's last image: the last term of every chain
        if row['variant'] is None and not padded and 'parts' not in inputs:
            assert neg.any() and (zeros & ~neg).any(), (self.name, int(neg.sum()), int(zeros.sum()))


class Overflow(Regime):
    """x * 2^100, w * 2^27: part of the chains reach +-inf midway (inf - inf = NaN after that); the kinds of row for which
    these scales leave nothing finite or nothing infinite take the ones the module's docstring derives"""
    name = 'overflow'

    def dress(self, rng, d, row):
        x0 = _x_arrays(d)[0]
        c = x0.shape[-1]
        tiny = x0.shape[1] * x0.shape[2] < 8  # (transposed: most taps of so small an image lie outside it)
        if row['variant'] is not None:  # sigma of a transformed input: 2 sx (4 terms; fewer under zero extension); 16 positions x the (virtual) input channels per tile
            cv = c * (4 if row['variant'] == 302 else 1)
            sigma = 1.75 if row['variant'] == 303 else 2.0  # (on the rows' small images much of a class form's patch is zero extension)
            _scale(d, row, sx=np.float32(2.0 ** 128 / (sigma * _normal_quantile(0.2 / (16 * cv)))), sw=p2(-3))
        elif row['gdn_mode'] or row['inverse']:
            co = d['w'].shape[0] if 'w' in d else c
            sx = np.float32(2.0 ** (64 + _tconv_binade(row)) / _normal_quantile(0.2 / co))
            _scale(d, row, sx=sx)
        elif row['tail']:
            _scale(d, row, sx=np.float32(1.375 * 2.0 ** 100), sw=p2(26))
        else:
            live = np.mean([p is not None for p in d['parts']]) if 'parts' in d else 1.0  # (an absent image: a third of the terms zero)
            _scale(d, row, sx=p2(100), sw=np.float32(2.0 ** (27 + _tconv_binade(row) + (1 if tiny else 0)) / math.sqrt(live)))

    def fact(self, row, want, chain):
        if row['forward_gdn_mode']:
            return chain(inverse=True)
        return chain() if row['hidden'] else want

    def reach(self, row, inputs, want, chain):
        f = self.fact(row, want, chain)
        fin = _frac(np.isfinite(f))
        assert 1.0 - fin >= 0.01 and fin >= 0.50, (self.name, fin)


def interior_pixel(h, w):
    return (h // 2, w // 2) if h * w >= 64 else (min(1, h - 1), min(1, w - 1))


def edge_pixel(h, w):
    return (0, w // 2) if h * w >= 64 else (0, min(1, w - 1))


def planted(shape):
    """[(image, row, column, channel, value)] in an [n, h, w, c] tensor with c usable channels: +inf at a corner pixel of image
    0, NaN at an interior and at an edge pixel of it, -inf at the last pixel of the last image in the last channel"""
    n, h, w, c = shape
    return [(0, 0, 0, 0, np.inf), (0,) + interior_pixel(h, w) + (1 % c, np.nan), (0,) + edge_pixel(h, w) + (2 % c, np.nan),
            (n - 1, h - 1, w - 1, c - 1, -np.inf)]


class Nonfinite(Regime):
    """ordinary operands and a handful of non-finite ones: planted() in x (the first float source of an image stack: its 3 real
    channels), one inf and one NaN in res and in mul where the row has them; nothing in w, beta, gamma or bias"""
    name = 'nonfinite'

    def dress(self, rng, d, row):
        done = []

        def plant(a):
            if done:
                return a
            done.append(1)
            a = a.copy()
            n, h, w, c = a.shape
            for i, y, x, ch, v in planted((n, h, w, 3 if 'parts' in d else c)):
                a[i, y, x, ch] = v
            return a
        _map_x(d, plant)
        for nm in ('res', 'mul'):
            if d.get(nm) is not None:
                a = d[nm] = d[nm].copy()
                n, h, w, c = a.shape
                a[0, h - 1, 0, c // 2] = np.inf if nm == 'res' else -np.inf
                a[n - 1, h // 2, w - 1, 0] = np.nan

    def fact(self, row, want, chain):
        return want  # the footprint is a statement about the full result (an activation only takes non-finite values away)

    def reach(self, row, inputs, want, chain):
        bad = ~np.isfinite(want)
        assert 0 < bad.sum() < bad.size / 2, (self.name, int(bad.sum()), bad.size)
        allowed = footprint(row, inputs, want.shape)
        assert not (bad & ~allowed).any(), (self.name, 'outside the footprint', np.argwhere(bad & ~allowed)[:4].tolist())


def _reads(row, size_in, size_out):
    """[size_out, size_in] 0 / 1: which input rows (columns) the contract lets an output row (column) read"""
    m = np.zeros((size_out, size_in), np.int64)
    k, s, pad, variant = row['k'], row['stride'], row['pad'], row['variant']
    for o in range(size_out):
        if variant is not None:  # the whole 2x2 tile's 4x4 patch, in the grid of the form
            g = o >> 1 if variant == 303 else o
            t = g >> 1
            for r in range(4):
                q = 2 * t - 1 + r
                if variant == 302:  # both phases of the patch row: input rows clamp(2 q + py)
                    for py in (0, 1):
                        m[o, min(max(2 * q + py, 0), size_in - 1)] = 1
                elif variant == 303:
                    if 0 <= q < size_in:
                        m[o, q] = 1
                else:
                    m[o, min(max(q, 0), size_in - 1)] = 1
        elif row['mode'] == abi.MODE_TCONV:
            tpad = (k + 1) // 2 - 1
            for kk in range(k):
                t = o + tpad - kk
                if t >= 0 and t % 2 == 0 and t // 2 < size_in:
                    m[o, t // 2] = 1
        elif row['gdn_mode']:
            m[o, o] = 1
        else:
            for kk in range(k):
                m[o, min(max(o * s + kk - pad, 0), size_in - 1)] = 1
    return m


def footprint(row, inputs, out_shape):
    """[n, ho, wo, co] bool: the outputs that have a non-finite operand inside the footprint the contract gives them -- k x k
    input pixels for the tap chains, the tile's patch for the Winograd forms (every channel: a chain runs over all of them, and
    a fused (I)GDN over the pixel's outputs), their own element of res / mul"""
    n, ho, wo, _ = out_shape
    bad_px = np.zeros(_x_arrays(inputs)[0].shape[:3], bool)
    for a in _x_arrays(inputs):
        bad_px |= (~np.isfinite(a)).any(axis=-1)
    ry, rx = _reads(row, bad_px.shape[1], ho), _reads(row, bad_px.shape[2], wo)
    allowed = np.einsum('oy,nyx,px->nop', ry, bad_px.astype(np.int64), rx) > 0
    allowed = np.broadcast_to(allowed[..., None], out_shape).copy()
    for nm in ('res', 'mul'):
        if inputs.get(nm) is not None:
            allowed |= ~np.isfinite(inputs[nm])
    return allowed


REGIMES = [SubOperands(), SubProducts(), Graded(), AllUnderflow('plain'), AllUnderflow('neg_bias'), AllUnderflow('checker'), Overflow(),
           Nonfinite()]

# ---- the comparison ----------------------------------------------------------------------------------------------------------------
# Launches that leave the sign of a zero result open: (variant code, regime name, the sentence of include/aivc_hip.h behind it).
# For these entries only, mismatch() accepts a zero of either sign where the oracle's result is a zero.
_UNDERFLOW = ('all_underflow', 'all_underflow_neg_bias', 'all_underflow_checker')
_SKIPS = 'skips zero terms of the chain (the padding of the last group, out-of-image taps): "a kernel may skip one"'
_PADS = 'the register-staged K loop pads K to whole tiles of 32 with zero terms: "or add further terms whose weight is zero"'
_THIN = 'walks the 3 x 3 input neighbourhood for all four classes, the taps a class lacks as zero weights: "or add further terms whose weight is zero"'
_SPARSE4 = 'AIVC_CONV_SPARSE4: the terms of the images\' zero pad channels are not issued: "a kernel may skip one"'
ZERO_SIGN_OPEN = (
    [(0, r, _SKIPS) for r in _UNDERFLOW] +
    [(v, r, _PADS) for v in (103, 110, 113, 115, 160, 161) for r in _UNDERFLOW] +
    [(2, r, _THIN) for r in _UNDERFLOW + ('sub_products',)] +   # (sub_products: one result in 75600 cancels to a zero)
    [(191, r, _SPARSE4) for r in _UNDERFLOW])


def zero_sign_open(codes, regime):
    return any(v in codes and r == regime.name for v, r, _ in ZERO_SIGN_OPEN)


def mismatch(got, want, sign_of_zero_open=False):
    """elementwise: where got is not want, bit for bit (detmath_cases.same_bits: a NaN matches a NaN)"""
    bad = ~same_bits(got, want)
    if sign_of_zero_open:
        bad &= ~((want == 0) & (got == 0))
    return bad


def assert_bits(got, want, what='', sign_of_zero_open=False):
    """the failure names the first index, both values and both bit patterns"""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    bad = mismatch(got, want, sign_of_zero_open)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        u = np.uint64 if got.dtype == np.float64 else np.uint32
        raise AssertionError('%s%d of %d differ; first at %s: got %r (0x%08x), want %r (0x%08x)' % (
            what and what + ': ', int(bad.sum()), bad.size, i, float(got[i]), int(got.view(u)[i]), float(want[i]), int(want.view(u)[i])))
