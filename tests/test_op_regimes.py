"""CPU tier of tests/op_regimes.py: the ORACLE itself, pinned on the regimes before any device is held to it.

Every builder runs here (its reach condition is an assertion on the oracle's result), and the oracle's results are compared with
restatements that are this file's own: plain numpy, every operation rounded to fp32, every float -> integer conversion written
with its NaN and range handling spelled out.  Elementwise ops, the entropy model and the rate estimates are compared by bits
(tests/numeric_regimes.py assert_bits: +0 is not -0, a NaN matches a NaN).  The transcendental inside a restatement
(exp, pow, log, the Laplace cdf) is the oracle's aivc_detmath_eval, which tests/test_detmath.py pins on its own; what is restated
is everything around it: clamps, conversions, operation order.

The warp is held to warp_fp64 of tests/test_warp_modes.py (position in fp32 in the reference's order with grid_sample's clip
taking a NaN to 0, weights and sums in fp64) with that file's bilinear bound, ROUNDINGS['bilinear'] * 2^-24 * max|x|; non-finite
results must agree in kind (NaN with NaN, an infinity with the same infinity).  warp_blend's x_warp adds 4 roundings of terms
bounded by max|x| to each side's 8 (1 - beta, two products, one sum); pred, skip, alpha and beta are elementwise: by bits.

tests/golden/warp_nonfinite.npz (tools/gen_golden_warp.py) is what the reference's own warp() returned for the flow sets of
op_regimes.FLOWS in all 18 modes: the restatement is held to it with the bounds of tests/test_warp_modes.py, the oracle (the
codec's mode) to the restatement on the same inputs."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import op_regimes as R  # noqa: E402
from aivc_amd import abi  # noqa: E402
from numeric_regimes import assert_bits  # noqa: E402
from test_warp_modes import ROUNDINGS, warp_fp64  # noqa: E402
from warp_modes_cases import CASES, MAX_LEFT_OUT, case_key, left_out  # noqa: E402

f32 = np.float32
IDS = sorted(R.REGIME_CASES)
QUIET = dict(over='ignore', under='ignore', invalid='ignore', divide='ignore')


@pytest.mark.parametrize('case_id', IDS)
def test_every_builder_reaches_its_regime(case_id, oracle):
    """the builder's own assertions on the oracle's result; and no case is exempt from the comparison by bits"""
    case = R.REGIME_CASES[case_id](oracle)
    assert case.want is not None
    assert R.NOT_HELD_BY_BITS == []


# ---- warp ------------------------------------------------------------------------------------------------------------------------
def nchw(a):
    return np.ascontiguousarray(np.transpose(a, (0, 3, 1, 2)))


def warp_restated(x, flow):
    """x [n, h, w, c], flow [n, h, w, 2] -> fp64 [n, h, w, c]: the codec's mode, image by image"""
    out = [warp_fp64(nchw(x[b:b + 1]), nchw(flow[b:b + 1]), 'bilinear', 'border', True)[0][0] for b in range(x.shape[0])]
    return np.transpose(np.stack(out), (0, 2, 3, 1))


def assert_same_kind_and_close(got, want64, bound, what=''):
    """NaN where the restatement has NaN, the same infinity where it has one, within `bound` everywhere else"""
    got = got.astype(np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), (what, 'NaN at', np.argwhere(np.isnan(got) != np.isnan(want64))[:4].tolist())
    inf = np.isinf(want64)
    assert np.array_equal(np.isinf(got), inf) and np.array_equal(got[inf], want64[inf]), (what, 'infinities')
    fin = np.isfinite(want64)
    dev = np.abs(got[fin] - want64[fin]).max() if fin.any() else 0.0
    print('%-40s max |oracle - fp64| = %.3e (bound %.3e)' % (what, dev, bound))
    assert dev <= bound, (what, dev, bound)


def x_bound(x, roundings=ROUNDINGS['bilinear']):
    return roundings * 2.0 ** -24 * float(np.abs(x[np.isfinite(x)]).max())


WARP_IDS = [i for i in IDS if i.startswith('warp-')]


@pytest.mark.parametrize('case_id', WARP_IDS)
def test_warp_oracle_against_the_fp64_restatement(case_id, oracle):
    """a NaN flow is a sample at position 0 (the restatement's, torch's and aivc_warp_modes'), not a pixel of zeros"""
    case = R.REGIME_CASES[case_id](oracle)
    x, flow = case.inputs['x'], case.inputs['flow']
    with np.errstate(**QUIET):
        want64 = warp_restated(x, flow)
    assert_same_kind_and_close(case.want, want64, x_bound(x), case_id)


def clamp01_restated(v):
    """`v < 0 ? 0 : (v > 1 ? 1 : v)`: a NaN passes"""
    with np.errstate(invalid='ignore'):
        return np.where(v < 0, f32(0), np.where(v > 1, f32(1), v)).astype(f32)


@pytest.mark.parametrize('case_id', [i for i in IDS if i.startswith('warp_blend-') and i.endswith('-fast')])
def test_warp_blend_oracle_against_the_restatement(case_id, oracle):
    case = R.REGIME_CASES[case_id](oracle)
    mof, prev, nxt = case.inputs['mof'], case.inputs['prev'], case.inputs['next']
    ft = int(case_id.split('-ft')[1][0])
    n, h, w, _ = prev.shape
    m = mof[:, :h, :w]
    with np.errstate(**QUIET):
        alpha, beta = clamp01_restated(m[..., 0] + f32(0.5)), clamp01_restated(m[..., 1] + f32(0.5))
        vp, vn = m[..., 2:4], m[..., 4:6]
        if ft == 1:
            beta, vn = np.ones_like(beta), np.zeros_like(vn)
        wp, wn = warp_restated(prev[..., :3], np.ascontiguousarray(vp)), warp_restated(nxt[..., :3], np.ascontiguousarray(vn))
        b64 = beta.astype(np.float64)[..., None]
        xw64 = b64 * wp + (f32(1) - beta).astype(np.float64)[..., None] * wn
    want = case.want
    assert_bits(want['alpha'], alpha, 'alpha')
    assert_bits(want['beta'], beta, 'beta')
    assert_same_kind_and_close(want['x_warp'][..., :3], xw64, x_bound(np.stack([prev, nxt]), 2 * ROUNDINGS['bilinear'] + 4), case_id)
    assert not want['x_warp'][..., 3].any() and not want['pred'][..., 3].any() and not want['skip'][..., 3].any()
    with np.errstate(**QUIET):  # elementwise from the oracle's own x_warp
        xw = want['x_warp'][..., :3]
        assert_bits(want['pred'][..., :3], xw * alpha[..., None], 'pred')
        assert_bits(want['skip'][..., :3], (f32(1) - alpha)[..., None] * xw, 'skip')


# ---- the reference's own answer to non-finite flows ------------------------------------------------------------------------------
NONFINITE_CASES = [c for c in CASES if c[0] == 0]


def test_nonfinite_fixture_holds_what_it_claims(golden):
    g = golden('warp_nonfinite')
    assert g['x_0'].shape == (1, 4, 9, 11) and len(g.files) == 2 + 2 * len(NONFINITE_CASES)
    flow = g['flow_0']
    assert np.isnan(flow).any(axis=1).sum() == 15 and np.isinf(flow).any(axis=1).sum() == 5 and (np.abs(flow) == R.BIG).any(axis=1).sum() == 5
    assert np.isfinite(g['x_0']).all()
    for s, mode, pad, ac in NONFINITE_CASES:
        with np.errstate(**QUIET):
            out = left_out(g, s, mode, pad, ac)  # (asserts the cap itself)
        assert out.mean() <= MAX_LEFT_OUT
    # the codec's mode: the reference returns a finite sample at every pixel, the NaN flows included
    assert np.isfinite(g['y_0_bilinear_border_1']).all()


def test_the_fixture_tool_plants_the_flow_sets_of_op_regimes():
    """tools/gen_golden_warp.py states the flow sets itself (a tool does not import the tests): the same names in the same order,
    and every kind gives the flow op_regimes.FLOWS gives, at every pixel of the fixture's frame"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tools'))
    import gen_golden_warp as tool
    sets = tool.nonfinite_flow_sets()
    assert [nm for nm, _ in sets] == list(R.FLOWS)
    _, _, h, w = tool.NONFINITE_SHAPE
    fx, fy = f32(0.75), f32(-1.25)  # the drawn flow of the pixel
    for nm, kinds in sets:
        assert len(kinds) == len(R.FLOWS[nm])
        for kind, mine in zip(kinds, R.FLOWS[nm]):
            for r in range(h):
                for q in range(w):
                    a = kind(r, q, h, w) if callable(kind) else kind
                    a = np.array([fx if a[0] is None else a[0], fy if a[1] is None else a[1]], f32)
                    assert_bits(a, np.array(mine(r, q, h, w, fx, fy), f32), nm)


@pytest.mark.parametrize('s,mode,pad,ac', NONFINITE_CASES, ids=[case_key(*c) for c in NONFINITE_CASES])
def test_fp64_restatement_matches_the_reference_on_nonfinite_flows(s, mode, pad, ac, golden):
    g = golden('warp_nonfinite')
    x, flow, key = g['x_0'], g['flow_0'], case_key(s, mode, pad, ac)
    with np.errstate(**QUIET):
        y64, m64 = warp_fp64(x, flow, mode, pad, ac)
        keep = ~left_out(g, s, mode, pad, ac)
    keep_y = np.broadcast_to(keep[:, None], y64.shape)
    bound = ROUNDINGS[mode] * 2.0 ** -24
    assert_same_kind_and_close(g['y_' + key][keep_y], y64[keep_y], bound * float(np.abs(x).max()), key)
    assert_same_kind_and_close(g['m_' + key][keep], m64[keep], bound, key + ' mask')


def test_oracle_matches_the_restatement_on_the_nonfinite_fixture(oracle, golden):
    g = golden('warp_nonfinite')
    x = np.ascontiguousarray(np.transpose(g['x_0'], (0, 2, 3, 1)))
    flow = np.ascontiguousarray(np.transpose(g['flow_0'], (0, 2, 3, 1)))
    with np.errstate(**QUIET):
        want64 = warp_restated(x, flow)
    got = oracle.warp(x, flow)
    assert_same_kind_and_close(got, want64, x_bound(x), 'oracle.warp on warp_nonfinite')
    # ... and so the reference's fp32 result: two fp32 evaluations, each within the bound of the fp64 value
    assert np.abs(nchw(got) - g['y_0_bilinear_border_1']).max() <= 2 * x_bound(x)


# ---- elementwise ops, by bits ----------------------------------------------------------------------------------------------------
def cast8_restated(v):
    """-> (byte, float level): round(255 clamp(v, 0, 1)) half to even; a NaN is byte 0 and a NaN level"""
    with np.errstate(**QUIET):
        c = np.where(v < 0, f32(0), v)
        c = np.where(c > 1, f32(1), c).astype(f32)
        r = np.rint(f32(255) * c).astype(f32)
        byte = np.where(np.isnan(r), f32(0), r)
        assert ((byte >= 0) & (byte <= 255)).all()
        return byte.astype(np.uint8), (r / f32(255)).astype(f32)


def frame_to_yuv420_restated(x, h, w, skip):
    with np.errstate(**QUIET):
        v = x[:, :h, :w, :3].astype(f32)
        if skip is not None:
            v = (v + skip[..., :3]).astype(f32)
        hc, wc, hf, wf = (h + 1) // 2, (w + 1) // 2, h // 2, w // 2
        planes = [cast8_restated(v[..., 0])]
        for ch in (1, 2):
            if hf == 0 or wf == 0:
                val = np.zeros((x.shape[0], hc, wc), f32)
            else:
                p = v[:, :2 * hf, :2 * wf, ch]
                top = (f32(0.5) * p[:, 0::2, 0::2] + f32(0.5) * p[:, 0::2, 1::2]).astype(f32)
                bot = (f32(0.5) * p[:, 1::2, 0::2] + f32(0.5) * p[:, 1::2, 1::2]).astype(f32)
                val = (f32(0.5) * top + f32(0.5) * bot).astype(f32)
                val = val[:, np.minimum(np.arange(hc), hf - 1)][:, :, np.minimum(np.arange(wc), wf - 1)]  # replicate pad
            planes.append(cast8_restated(val))
    return [p[1] for p in planes], [p[0] for p in planes]


@pytest.mark.parametrize('case_id', [i for i in IDS if i.startswith('frame_to_yuv420-')])
def test_frame_to_yuv420_oracle_by_bits(case_id, oracle):
    case = R.REGIME_CASES[case_id](oracle)
    h, w = (int(v) for v in case_id.split('-')[1].split('x'))
    floats, bytes_ = frame_to_yuv420_restated(case.inputs['x'], h, w, case.inputs['skip'])
    (fy, fu, fv), (by, bu, bv) = case.want
    for nm, got, want in zip('yuv', (by, bu, bv), bytes_):
        np.testing.assert_array_equal(got, want, nm)
    for nm, got, want in zip('yuv', (fy, fu, fv), floats):
        assert_bits(got, want, nm)


def quantize_restated(y, mu, gain):
    """-> (q int16, y_hat): a NaN difference is q = 0 and stays NaN in y_hat"""
    with np.errstate(**QUIET):
        r = np.rint(y if mu is None else (y - mu).astype(f32)).astype(f32)
        r = np.where(r < -256, f32(-256), np.where(r > 256, f32(256), r)).astype(f32)
        level = np.where(np.isnan(r), f32(0), r)
        assert ((level >= -256) & (level <= 256)).all()
        v = r if mu is None else (r + mu).astype(f32)
        if gain is not None:
            v = (v * np.abs(gain)).astype(f32)
        return level.astype(np.int16), v


def dequantize_restated(q, mu, gain):
    with np.errstate(**QUIET):
        v = q.astype(f32)
        if mu is not None:
            v = (v + mu).astype(f32)
        return v if gain is None else (v * np.abs(gain)).astype(f32)


def test_latent_ops_oracle_by_bits(oracle):
    case = R.REGIME_CASES['latent'](oracle)
    d, want = case.inputs, case.want
    y, mu, q_ext = d['y'], d['mu'], d['q_ext']
    rows = d['gains'][:, None, None, :]
    with np.errstate(**QUIET):
        restated = {'gain': (y * np.abs(d['gain'])).astype(f32), 'gain_none': y, 'gain_rows': (y * np.abs(rows)).astype(f32),
                    'deq': dequantize_restated(q_ext, mu, d['gain']), 'deq0': dequantize_restated(q_ext, None, None),
                    'deq_rows': dequantize_restated(q_ext, mu, rows)}
    restated['q'], restated['yh'] = quantize_restated(y, mu, d['gain'])
    restated['q0'], restated['yh0'] = quantize_restated(y, None, None)
    restated['q_rows'], restated['yh_rows'] = quantize_restated(y, mu, rows)
    restated['q_only'] = restated['q']
    assert set(restated) == set(want)
    for k in sorted(want):
        if want[k].dtype == np.int16:
            np.testing.assert_array_equal(want[k], restated[k], k)
        else:
            assert_bits(want[k], restated[k], k)


def test_hyper_params_oracle_by_bits(oracle):
    case = R.REGIME_CASES['hyper_params'](oracle)
    hs = case.inputs['hs']
    with np.errstate(**QUIET):
        lv = hs[:, :5, :7, 8:]
        lv = np.where(lv < R.LOG_VAR_MIN, R.LOG_VAR_MIN, lv)  # (a NaN passes both)
        lv = np.where(lv > R.LOG_VAR_MAX, R.LOG_VAR_MAX, lv).astype(f32)
        sigma = oracle.detmath_eval(abi.DETMATH_EXPF, (f32(0.5) * lv).astype(f32))
    assert_bits(case.want['mu'], np.ascontiguousarray(hs[:, :5, :7, :8]), 'mu')
    assert_bits(case.want['sigma'], sigma, 'sigma')


@pytest.mark.parametrize('lam', R.GAIN_INTERP_LAMBDAS)
def test_gain_interp_oracle_by_bits(lam, oracle):
    case = R.REGIME_CASES['gain_interp-%g' % lam](oracle)
    l = f32(lam)
    with np.errstate(**QUIET):
        a, b = (np.where(g < 0, -g, g) for g in (case.inputs['g_r'], case.inputs['g_t']))
        pa = oracle.detmath_eval(abi.DETMATH_POWF, a, np.full_like(a, l))
        pb = oracle.detmath_eval(abi.DETMATH_POWF, b, np.full_like(b, f32(1) - l))
        assert_bits(case.want, (pa * pb).astype(f32), 'gain_interp')


def test_downsample_pad_and_reparam_oracle_by_bits(oracle):
    with np.errstate(**QUIET):
        for case, (ch0, nch) in zip(R.downsample2x_regime_cases(oracle, 17), ((1, 2), (0, 6), (5, 1))):
            x = case.inputs['x'][:, :4, :6, ch0:ch0 + nch]
            top = (f32(0.5) * x[:, 0::2, 0::2] + f32(0.5) * x[:, 0::2, 1::2]).astype(f32)
            bot = (f32(0.5) * x[:, 1::2, 0::2] + f32(0.5) * x[:, 1::2, 1::2]).astype(f32)
            assert_bits(case.want, np.transpose((f32(0.5) * top + f32(0.5) * bot).astype(f32), (0, 3, 1, 2)), 'downsample2x')
        case = R.REGIME_CASES['pad_channels'](oracle)
        x = case.inputs['x']
        assert_bits(case.want, np.concatenate([x, np.zeros(x.shape[:3] + (5,), f32)], axis=-1), 'pad_channels')
        case = R.REGIME_CASES['gdn_reparam'](oracle)
        bb, gb, ped = R.GDN_BOUNDS
        for nm, src, bound in (('be', case.inputs['beta'], bb), ('ge', case.inputs['gamma'], gb)):
            v = np.where(src > bound, src, bound).astype(f32)  # (a NaN takes the bound)
            assert_bits(case.want[nm], ((v * v).astype(f32) - ped).astype(f32), nm)


# ---- entropy model ---------------------------------------------------------------------------------------------------------------
def cdf_quant_restated(cdf, k):
    """a cdf is taken as a value of [0, 1]: beyond it the nearer end, a NaN 0; then (int)rint(cdf * 65023) + k, wrapping"""
    with np.errstate(**QUIET):
        c = np.where(cdf > 0, cdf, f32(0))
        c = np.where(c < 1, c, f32(1)).astype(f32)
        r = np.rint((c * f32(65023.0)).astype(f32))
    assert ((r >= 0) & (r <= 65023)).all()
    return ((r.astype(np.int64) + k) & 0xFFFF).astype(np.uint16)


def rows_restated(oracle, sigma_pos):
    k = np.arange(abi.LP)
    t = (k.astype(f32) - f32(256.5)).astype(f32)
    tt, ss = np.broadcast_arrays(t[None, :], sigma_pos[:, None])
    cdf = oracle.detmath_eval(abi.DETMATH_LAPLACE_CDF, np.ascontiguousarray(tt), np.ascontiguousarray(ss))
    rows = np.zeros((sigma_pos.size, abi.CDF_ROW), np.uint16)
    rows[:, :abi.LP] = cdf_quant_restated(cdf, k[None, :])
    return rows


@pytest.mark.parametrize('name', R.SIGMA_SETS)
def test_entropy_rows_oracle_by_bits(name, oracle):
    case = R.REGIME_CASES['sigma-' + name](oracle)
    rows = rows_restated(oracle, case.per_pos)
    np.testing.assert_array_equal(case.want['rows'], rows)
    np.testing.assert_array_equal(case.want['win'], rows[:, abi.CDF_WIN0:abi.CDF_WIN0 + abi.CDF_WIN])
    q, maps = case.inputs['q'], R.ENTROPY_MAPS
    sym = q.reshape(-1, q.shape[-1])[:, maps].T.reshape(-1).astype(np.int64) + 256
    lo = rows[np.arange(sym.size), sym].astype(np.uint32)
    hi = np.where(sym == 512, 0, rows[np.arange(sym.size), np.minimum(sym + 1, 513)]).astype(np.uint32)
    np.testing.assert_array_equal(case.want['bounds'], lo | (hi << 16))
    # the range decoder's rare-path layout of the row function returns the row's entry, for every value of the set
    bad, first = oracle.laplace_tail_mismatches(case.special)
    assert bad == 0, (bad, first)


def test_rows_of_the_sigmas_the_header_names(oracle):
    """include/aivc_hip.h: a NaN sigma gives the row k, sigma = 0 a point mass, +inf the row 32512 + k, -0.0 a row that does not increase"""
    sig = np.array([np.nan, 0.0, np.inf, -0.0], f32).reshape(1, 1, 4, 1)
    rows = oracle.laplace_cdf_rows(sig, [0])[:, :513].astype(np.int64)
    k = np.arange(513)
    np.testing.assert_array_equal(rows[0], k)
    np.testing.assert_array_equal(rows[1], np.where(k <= 256, k, (65023 + k) & 0xFFFF))
    np.testing.assert_array_equal(rows[2], 32512 + k)
    np.testing.assert_array_equal(rows[3], np.where(k <= 256, (65023 + k) & 0xFFFF, k))


# ---- rate estimates --------------------------------------------------------------------------------------------------------------
def rate_sum_restated(terms):
    """lane j adds its elements j, j + L, ... in order; then lanes[j] += lanes[j + s] for s = L / 2 ... 1"""
    lanes = np.zeros(abi.RATE_LANES, np.float64)
    with np.errstate(**QUIET):
        for i in range(0, terms.size, abi.RATE_LANES):
            part = terms[i:i + abi.RATE_LANES]
            lanes[:part.size] = lanes[:part.size] + part
        s = abi.RATE_LANES // 2
        while s >= 1:
            lanes[:s] = lanes[:s] + lanes[s:2 * s]
            s //= 2
    return lanes[0]


def test_rate_estimates_oracle_by_bits(oracle):
    case = R.REGIME_CASES['rate'](oracle)
    d, want = case.inputs, case.want
    y, mu, sigma = d['y'], d['mu'], d['sigma']
    cdf_of = lambda t: oracle.detmath_eval(abi.DETMATH_LAPLACE_CDF, t, sigma)
    with np.errstate(**QUIET):
        for nm, m in (('p_mu', mu), ('p_zero', np.zeros_like(mu))):
            up, dn = ((y + f32(0.5)).astype(f32) - m).astype(f32), ((y - f32(0.5)).astype(f32) - m).astype(f32)
            assert_bits(want[nm], (cdf_of(up) - cdf_of(dn)).astype(f32), nm)
        whole = (y >= -256) & (y <= 256) & (np.rint(y) == y)
        k = np.where(whole, y, 0).astype(np.int64)
        ch = np.arange(y.shape[1]).reshape(1, -1, 1, 1)
        p_z = np.where(whole, d['cdf'][ch, k + 257] - d['cdf'][ch, k + 256], f32(np.nan)).astype(f32)
        assert_bits(want['p_z'], p_z, 'p_z')
        for nm, p in (('rate_p', d['p']), ('rate_f', d['p_fin'])):
            lo, hi = f32(R.RATE_P_MIN), f32(R.RATE_P_MAX)
            c = np.where(p < lo, lo, np.where(p > hi, hi, p)).astype(f32)  # (a NaN stays)
            safe = np.where(np.isnan(c), f32(1), c)
            rate = (-(oracle.detmath_eval(abi.DETMATH_LOG, safe.astype(np.float64)) * 1.4426950408889634)).astype(f32)
            rate = np.where(np.isnan(c), c, rate).astype(f32)
            assert_bits(want[nm], rate, nm)
            total = R.total_bits(rate_sum_restated(rate.reshape(-1).astype(np.float64)))
            got = R.total_bits(oracle.rate_bits(p, R.RATE_P_MIN, R.RATE_P_MAX)[1])
            assert got == total, (nm, got, total)
        b = d['bnd'].view(np.uint32)
        lo, hi16 = (b & 0xFFFF).astype(np.int64), (b >> 16).astype(np.int64)
        hi = np.where(hi16 == 0, 0x10000, hi16)
        ok = hi > lo
        terms = np.where(ok, 16.0 - oracle.detmath_eval(abi.DETMATH_LOG, np.where(ok, hi - lo, 1).astype(np.float64)) * 1.4426950408889634, 16.0)
        assert R.total_bits(oracle.bounds_rate(b)) == R.total_bits(rate_sum_restated(terms))
