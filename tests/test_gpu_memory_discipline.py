"""Every device entry point of aivc_amd.ops under the guard-zone and poison harness of tests/guarded.py (read its docstring first:
what an arena is, why there are two fills, what the method cannot see).

Each case runs twice, once per fill.  Its inputs go in through guarded(...): they sit flush against 1 MiB of poison on both
sides.  The call runs inside guard_ops(fill): every output and scratch buffer ops allocates is an arena too, and its untouched
payload is poison.  The result is compared with the CPU oracle exactly as the plain test of that operation compares it (bit
exact; 1e-12 for ssim_means and sq_err; the reference-run fixture and its stated bounds for the warp modes; the bf16x3 mode, which
has no oracle, against its own unguarded run).  Then the guards are checked and the two runs are compared byte for byte.  So a
store outside an output, an output element that is not written and a read outside an input that reaches the result each fail a case.

A case is stated once, in tests/conv_cases.py and tests/op_cases.py: tables, inputs, the ops call, the oracle's result and the
comparison.  The plain tests place its inputs as ordinary tensors; here the placer is guarded(...), and what this file adds is its
choice of cases (edge shapes flush against a guard), the guard-specific assertions, and for the conv tests which kernel variant
took the launch (ops.PROFILE).

ops.range_encode's inputs stay plain tensors (see tests/guarded.py); its outputs are guarded."""
import numpy as np
import pytest
import torch

from aivc_amd import abi
from conv_cases import (BF16X3_CASES, CONV_CASES, CONV_IMAGES_CASES, FUSED_GDN_CASES, FUSED_TAIL_CASES, GDN_RESIDENT_CASES, POLY_CASES,
                        TC_CASES, THIN_WALK_CASES, THIN_WALK_GRIDS, WINO_CASES, bf16x3_case, conv_case, conv_images_cases, fused_gdn_case,
                        fused_tail_case, gdn_resident_case, mfma_tile_case, pack_images_cases, thin_walk_case, wino_case, wino_weights_case)
from guarded import both_fills, guarded, guarded_empty
from op_cases import (AUX, FRAME_BATCH_CASES, FRAME_SIZES, RANGE_DECODE_CASES, WARP_SHAPES, T, bounds_rate_case, cdf_case, detmath_case, downsample2x_cases,
                      eq, frame_batch_case, frame_sources, frame_to_yuv420_case, gain_interp_case, latent_ops_case, metrics_case, on,
                      pad_channels_case, profiled, range_coder_case, range_coder_pmf_case, range_encode_case, rate_estimates_case,
                      stream_bytes, warp_blend_case, warp_blend_sources, warp_case, warp_modes_case, yuv420_to_444_case, yuv_planes)
from op_regimes import REGIME_CASES
from warp_modes_cases import CASES as WARP_CASES, case_key

pytestmark = pytest.mark.gpu

ALGOS = [abi.ALGO_DIRECT, abi.ALGO_AUTO, abi.ALGO_MFMA]
MODE_DIGIT = {abi.MODE_CONV: 0, abi.MODE_TCONV: 1, abi.MODE_GDN: 2, abi.MODE_IGDN: 2}
TILES = (0, 1, 2, 3, 5, 6)


def G(dev, fill):
    """the placer of this file: every input an arena"""
    return lambda a: guarded(a, dev, fill)


def run_guarded(case, dev, codes=None, **kw):
    """the case under both fills, compared with its expected result each time; codes: the conv variants the launch must take
    (a list, or a predicate on the list)"""
    from aivc_amd import ops

    def run(fill):
        if codes is None:
            return case.check(case.run(ops, G(dev, fill), **kw))
        got, took = profiled(lambda: case.run(ops, G(dev, fill), **kw))
        assert codes(took) if callable(codes) else took == codes, took
        return case.check(got)
    return both_fills(run)


def poisoned(t, fill):
    """every byte of t still holds the fill"""
    return bool((t.contiguous().view(-1).view(torch.uint8) == fill).all())


# ---- conv family -----------------------------------------------------------------------------------------------------------------
def _route(mode, k, ci, co, algo):
    """the kernel family the dispatch rule of csrc/api.hip gives a plain launch of these cases"""
    if algo == abi.ALGO_DIRECT:
        return 'direct'
    if algo == abi.ALGO_MFMA:
        return 'mfma'
    if mode in (abi.MODE_GDN, abi.MODE_IGDN) and ci in (64, 128):
        return 'resident'
    if mode == abi.MODE_TCONV and co in (3, 6) and k in (3, 5) and ci % 8 == 0 and 16 <= ci <= 128:
        return 'thin'
    return 'direct' if co < 16 and ci * k * k < 256 else 'mfma'


def _on_route(route, mode):
    def ok(codes):
        if len(codes) != 1:
            return False
        if route == 'direct':
            return codes[0] == 0
        if route == 'resident':
            return codes[0] == 400
        if route == 'thin':
            return codes[0] in (1, 2)
        return codes[0] // 10 == 10 + MODE_DIGIT[mode] and codes[0] % 10 in TILES
    return ok


@pytest.mark.parametrize('idx', range(len(CONV_CASES)))
def test_conv_family(idx, oracle, cuda):
    mode, k, _, _, ci, co = CONV_CASES[idx][:6]
    case = conv_case(oracle, CONV_CASES[idx], 1000 + idx)
    for algo in ALGOS:
        run_guarded(case, cuda, _on_route(_route(mode, k, ci, co, algo), mode), algo=algo)


@pytest.mark.parametrize('idx', range(len(FUSED_GDN_CASES)))
def test_fused_gdn(idx, oracle, cuda):
    mode, co = FUSED_GDN_CASES[idx][0], FUSED_GDN_CASES[idx][5]
    if co in (32, 64, 128):  # 150 + 10 * mode + tile: the fused epilogue in one launch
        codes = lambda c: len(c) == 1 and c[0] // 10 == 15 + MODE_DIGIT[mode] and c[0] % 10 in TILES
    else:
        codes = lambda c: len(c) == 2 and all(v < 150 for v in c)
    run_guarded(fused_gdn_case(oracle, FUSED_GDN_CASES[idx], 2000 + idx), cuda, codes)


@pytest.mark.parametrize('idx', range(len(FUSED_TAIL_CASES)))
def test_fused_tail(idx, oracle, cuda):
    from aivc_amd import ops
    _, _, ci, cm, ct = FUSED_TAIL_CASES[idx][:5]
    case = fused_tail_case(oracle, FUSED_TAIL_CASES[idx], 3000 + idx)
    assert ops.PRECISION == abi.PREC_FP32_WINO and not ops.WINO_ANY_SIZE
    if cm == 64 and ct == 128 and ci % 32 == 0:
        codes = [190]
    elif case.covered:
        codes = lambda c: len(c) == 2 and c[0] == 301 and c[1] not in ops._WINO_VARIANTS
    else:
        codes = lambda c: len(c) == 2 and 190 not in c and not set(c) & set(ops._WINO_VARIANTS)
    run_guarded(case, cuda, codes)


@pytest.mark.parametrize('case', [c for c in GDN_RESIDENT_CASES if c[1] * c[2] * c[3] <= 4096])
def test_gdn_resident(case, oracle, cuda):
    """stand-alone (I)GDN with gamma resident in registers: variant 400"""
    run_guarded(gdn_resident_case(oracle, case), cuda, [400])


@pytest.mark.parametrize('grid', THIN_WALK_GRIDS)
@pytest.mark.parametrize('co,k,ci,h,w', THIN_WALK_CASES)
def test_thin_layer_tile_walk(grid, co, k, ci, h, w, oracle, cuda, monkeypatch):
    """few persistent groups walking several tiles each over 3 images (AIVC_THIN_GRID_MAX): the 16x16x4 MFMA kernel, variant 2"""
    monkeypatch.setenv('AIVC_THIN_GRID_MAX', str(grid))
    run_guarded(thin_walk_case(oracle, (co, k, ci, h, w), grid * 100 + co), cuda, [2])


@pytest.fixture()
def fp32w_any_size(oracle):
    from aivc_amd import ops
    prev_h, prev_o = ops.set_precision('fp32w'), oracle.set_precision('fp32w')
    ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = True
    yield
    ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = False
    ops.set_precision(prev_h)
    oracle.set_precision(prev_o)


def _edge_shape(n, h, w):
    """the shapes of the Winograd case lists that put a partial 2 x 2 tile on the last row or column of a small image: odd in
    both dimensions (a single pixel included); the lists hold such shapes with n = 1, 2, 3 and 5"""
    return h % 2 == 1 and w % 2 == 1 and h * w <= 300


WINO_GUARDED = ([(301, c) for c in WINO_CASES if _edge_shape(*c[:3])] +
                [(302, c[:8] + (False, c[8])) for c in POLY_CASES if _edge_shape(*c[:3])] +
                [(303, c[:8] + (False, c[8])) for c in TC_CASES if _edge_shape(*c[:3])])
assert {v for v, _ in WINO_GUARDED} == {301, 302, 303}
assert all(any(v == code and c[0] >= 2 for v, c in WINO_GUARDED) and any(v == code and c[1:3] == (1, 1) for v, c in WINO_GUARDED)
           for code in (301, 302, 303))  # n >= 2 and 1 x 1 on every kernel


@pytest.mark.parametrize('variant,case', WINO_GUARDED)
def test_winograd(variant, case, oracle, cuda, fp32w_any_size):
    run_guarded(wino_case(oracle, variant, case, variant * 100 + case[0] * 10 + case[1]), cuda, [variant])


@pytest.mark.parametrize('c_in', [8, 32])
@pytest.mark.parametrize('form', ['3x3', 'poly5', 'tconv5'])
def test_winograd_weight_transforms(form, c_in, oracle, cuda):
    from aivc_amd import ops
    case = wino_weights_case(oracle, form, c_in)

    def run(fill):
        u = case.run(ops, G(cuda, fill))
        assert hasattr(u, '_guard') and u.numel() == case.want.size
        return case.check(u)
    both_fills(run)


@pytest.mark.parametrize('case', BF16X3_CASES)
def test_bf16x3_mode(case, cuda):
    """The precision mode has no oracle (its bits are its own): the unguarded run of the same launch stands in, the weights
    split ahead of the launch and by the K loop give the same bits (csrc/conv_bf16x3.hip), and the two fills must agree."""
    from aivc_amd import ops
    v_ahead, v_loop = case[9:]
    c = bf16x3_case(case, 4000 + case[5] + case[1])
    prev, prev_split = ops.set_precision('bf16x3'), ops.PRESPLIT_WEIGHTS
    try:
        c.want = c.run(ops, on(cuda)).cpu().numpy()
        assert np.isfinite(c.want).all()
        for ahead, variant in ((True, v_ahead), (False, v_loop)):
            ops.PRESPLIT_WEIGHTS = ahead
            run_guarded(c, cuda, [variant])
    finally:
        ops.PRESPLIT_WEIGHTS = prev_split
        ops.set_precision(prev)


@pytest.mark.parametrize('tile,c_in', [(t, ci) for ci in (32, 12) for t in TILES if t != 2 or ci % 32 == 0])
def test_every_mfma_tile(tile, c_in, oracle, cuda, monkeypatch):
    """AIVC_FORCE_TILE: 0 = 128x128, 1 = 64x64, 2 = 256x64, 3 = 128x32, 5 = 64x128, 6 = 128x64 on M = 2 * 9 * 13 = 234 rows and
    72 output channels (multiples of no tile side): partial tiles along both; c_in 32 takes the LDS-DMA K loop, 12 the generic
    loader (which the 256-row tile is not instantiated for)"""
    monkeypatch.setenv('AIVC_FORCE_TILE', str(tile))
    run_guarded(mfma_tile_case(oracle, 5000 + tile + c_in, c_in), cuda, [100 + tile], algo=abi.ALGO_MFMA)


# ---- conv_images and pack_images -------------------------------------------------------------------------------------------------
IMAGE_SIZES = [c for c in CONV_IMAGES_CASES if c[0] % 2 and c[1] % 2]  # odd h and w: ceil-sized chroma planes flush against their guard
assert [c[:2] for c in IMAGE_SIZES] == [(9, 13), (35, 131)]


@pytest.mark.parametrize('h,w,n', IMAGE_SIZES)
@pytest.mark.parametrize('use_gdn', [True, False])
def test_conv_images(h, w, n, use_gdn, oracle, cuda, monkeypatch):
    """aivc_conv_images (variant 191) on 1 / 2 / 3 images: 8-bit 4:2:0 planes, float sources of 3 and 4 channels, a None part"""
    from aivc_amd import ops
    monkeypatch.setattr(ops, '_CONV_IMAGES_MAX', 3)
    for case in conv_images_cases(oracle, h, w, n, use_gdn, ('a', 'f', ('f3',), 'ab', ('a', 'f3'), 'aba', ('f', 'a', None))):
        run_guarded(case, cuda, [191])


@pytest.mark.parametrize('h,w,n', IMAGE_SIZES)
def test_pack_images(h, w, n, oracle, cuda):
    for case in pack_images_cases(oracle, h, w, n, ('a', ('f3',), ('a', None), ('a', 'b', None), 'af', 'aba', (None, 'f3', 'b'))):
        run_guarded(case, cuda)


# ---- pixel operations ------------------------------------------------------------------------------------------------------------
PLANE_SIZES = [(1, 1), (9, 13), (6, 1028)]
assert set(PLANE_SIZES) < set(FRAME_SIZES)


@pytest.mark.parametrize('h,w', PLANE_SIZES)
@pytest.mark.parametrize('u8', [True, False])
def test_yuv420_to_444(h, w, u8, oracle, cuda):
    """every stored layout: c_store 3 / 4 / 8, c_off 0 / 4, into a fresh tensor and into the caller's (whose other channels stay)"""
    from aivc_amd import ops
    planes = yuv_planes(h * 10 + w, h, w)
    for c_store, c_off in ((3, 0), (4, 0), (8, 0), (8, 4)):
        for own_out in (False, True):
            case = yuv420_to_444_case(oracle, planes, u8, c_store, c_off, own_out)

            def run(fill):
                got = case.run(ops, G(cuda, fill))
                assert hasattr(got, '_guard')
                return case.check(got)
            both_fills(run)


@pytest.mark.parametrize('h,w', PLANE_SIZES + [(10, 14)])
def test_frame_to_yuv420(h, w, oracle, cuda):
    """4 stored channels with margins (scalar path) and the 3-channel even-pitch hand-over of the codec (vector path when the
    frame sides are even), with and without the skip frame, floats and bytes or bytes alone"""
    x, skip, x3 = frame_sources(5 + h + w, h, w)
    for src in (x, x3):
        for sk in (None, skip):
            for want_float in (True, False):
                run_guarded(frame_to_yuv420_case(oracle, src, h, w, sk, want_float), cuda)


@pytest.mark.parametrize('h,w,s', WARP_SHAPES + [(1, 1, 1.0)])
def test_warp(h, w, s, oracle, cuda):
    run_guarded(warp_case(oracle, 6 + h, h, w, s), cuda)


@pytest.mark.parametrize('s,mode,pad,ac', WARP_CASES, ids=[case_key(*c) for c in WARP_CASES])
def test_warp_modes(s, mode, pad, ac, cuda, golden):
    """every sampling mode against the reference-run fixture, with the bounds and the left-out pixels of tests/test_gpu_warp_modes.py"""
    run_guarded(warp_modes_case(golden('warp_modes'), s, mode, pad, ac), cuda)


@pytest.mark.parametrize('h,w,s', WARP_SHAPES)
@pytest.mark.parametrize('ft', [1, 2])
@pytest.mark.parametrize('general', [False, True])
def test_warp_blend(h, w, s, ft, general, oracle, cuda):
    """both frame types on the 16-byte fast path (4 / 4 / 8 channels) and the general kernel (3 / 3 / 7), with and without the
    auxiliary outputs"""
    sources = warp_blend_sources(60 + h, h, w, s)
    for want_aux in (True, False):
        run_guarded(warp_blend_case(oracle, sources, h, w, ft, general, want_aux), cuda)


@pytest.mark.parametrize('rows', [(0, 4), (4, 5), (9, 4), (0, 13), (12, 1)])
@pytest.mark.parametrize('ft', [1, 2])
@pytest.mark.parametrize('general', [False, True])
def test_warp_blend_rows(rows, ft, general, oracle, cuda):
    """a first, a middle and a last band of a 13-row frame (and the whole frame, and one row): the band of the MOFNet output in,
    whole reference frames in, the band's rows out -- equal to the oracle's band and to the rows of the oracle's whole frame"""
    from aivc_amd import ops
    case = warp_blend_case(oracle, warp_blend_sources(70, 13, 11, 4.0), 13, 11, ft, general, rows=rows)

    def run(fill):
        g = case.check(case.run(ops, G(cuda, fill)))
        assert all(g[kk].shape[1] == rows[1] for kk in AUX)
        return g
    both_fills(run)


@pytest.mark.parametrize('h,w', [(6, 8), (7, 9), (6, 9), (7, 8), (2, 2), (3, 67)])
def test_downsample2x(h, w, oracle, cuda):
    """2x2 means of a channel range that does not start at 0, planar output; an odd side drops its last row / column"""
    for case in downsample2x_cases(oracle, h * 100 + w, h, w):
        run_guarded(case, cuda)


@pytest.mark.parametrize('lam', [0.0, 1.0, 0.3])
@pytest.mark.parametrize('n', [1, 13, 192])
def test_gain_interp(lam, n, oracle, cuda):
    run_guarded(gain_interp_case(oracle, n, n, lam), cuda)


@pytest.mark.parametrize('c_in,c_out', [(3, 4), (6, 8), (13, 16)])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (1, 3, 129)])
def test_pad_channels(c_in, c_out, shape, oracle, cuda):
    run_guarded(pad_channels_case(oracle, c_in, shape, c_in, c_out), cuda)


def test_latent_ops(oracle, cuda):
    """hyper_params, channel_gain, quantize_center with and without y_hat / mu / gain, dequantize, gdn_reparam"""
    run_guarded(latent_ops_case(oracle, 7), cuda)


# ---- entropy model and rate ------------------------------------------------------------------------------------------------------
def test_cdf_tables_and_single_frame_kernels(oracle, cuda):
    """balle_cdf_table with and without the float table; laplace_cdf_rows / laplace_cdf_windows into fresh tensors and into
    the caller's at a row offset (the rows before and behind still hold the fill); laplace_bounds, table_bounds, nonzero_flags"""
    from aivc_amd import ops
    case = cdf_case(oracle, 8, (1, 5, 7, 8))
    maps, npos, want, off = case.maps, case.npos, case.want, 3

    def run(fill):
        d = case.place(G(cuda, fill))
        out = case.check(case.call(ops, d))
        own = guarded_empty((off + npos + 2, abi.CDF_ROW), torch.int16, cuda, fill)
        assert ops.laplace_cdf_rows(d['sig'], maps, out=own, row_off=off) is own
        eq(own[off:off + npos], want['rows'])
        assert poisoned(own[:off], fill) and poisoned(own[off + npos:], fill)
        out['rows_own'] = own[off:off + npos]
        own_w = guarded_empty((off + npos + 2, abi.CDF_WIN), torch.int16, cuda, fill)
        own_s = guarded_empty((off + npos + 2,), torch.float32, cuda, fill)
        ops.laplace_cdf_windows(d['sig'], maps, out=(own_w, own_s), row_off=off)
        eq(own_w[off:off + npos], want['win']), eq(own_s[off:off + npos], want['sp'])
        assert all(poisoned(t[:off], fill) and poisoned(t[off + npos:], fill) for t in (own_w, own_s))
        out['win_own'], out['sp_own'] = own_w[off:off + npos], own_s[off:off + npos]
        return out
    both_fills(run)


@pytest.mark.parametrize('shape,maps', FRAME_BATCH_CASES)
def test_frame_batch_entropy_kernels(shape, maps, oracle, cuda):
    """the _batch forms on ragged per-frame map lists with a frame that codes nothing; c % 8 != 0 in the second shape"""
    from aivc_amd import ops
    case = frame_batch_case(oracle, 21 + shape[3], shape, maps)
    total = case.total

    def run(fill):
        win = guarded_empty((total + 3, abi.CDF_WIN), torch.int16, cuda, fill)
        sp = guarded_empty((total + 3,), torch.float32, cuda, fill)
        r = case.check(case.run(ops, G(cuda, fill), out=(win, sp)))
        assert hasattr(r['tab'][0], '_guard')
        assert poisoned(win[total:], fill) and poisoned(sp[total:], fill)
        out = {k: v for k, v in r.items() if k not in ('offs', 'tab')}  # (the device table's padding follows the fill)
        out['b'], out['win'], out['sp'] = r['b'][:total], win[:total], sp[:total]
        return out
    both_fills(run)


def test_frames_that_code_nothing(oracle, cuda):
    """a batch in which no frame has a coded map: no launch, nothing written"""
    from aivc_amd import ops
    sig = np.full((2, 3, 4, 8), 1.0, np.float32)
    q = np.zeros((2, 3, 4, 8), np.int16)

    def run(fill):
        b, offs = ops.laplace_bounds_batch(guarded(sig, cuda, fill), guarded(q, cuda, fill), [[], []])
        win = guarded_empty((2, abi.CDF_WIN), torch.int16, cuda, fill)
        sp = guarded_empty((2,), torch.float32, cuda, fill)
        offs2, _ = ops.laplace_cdf_windows_batch(guarded(sig, cuda, fill), [[], []], (win, sp))
        assert offs == offs2 == [0, 0]
        assert poisoned(b, fill) and poisoned(win, fill) and poisoned(sp, fill)
        return offs
    both_fills(run)


def test_range_encode(oracle, cuda):
    """plain inputs (the product's back-to-back detection runs on _base / storage_offset as ever), guarded outputs: separate
    tensors (concatenated), slices of one tensor (taken as they sit), more than 64 streams (two launches), ragged lengths"""
    from aivc_amd import ops
    case = range_encode_case(oracle, 77, [1, 7, 8, 9, 63, 64, 65, 500], 62, 400, straddle=False)
    separate = case.place(on(cuda))['streams']
    one = T(np.concatenate(case.inputs['streams']), cuda)
    cuts = np.concatenate([[0], np.cumsum(case.lens)])
    slices = [one[cuts[i]:cuts[i + 1]] for i in range(len(case.lens))]
    for bounds_list in (separate, slices, separate[:1]):
        def run(fill):
            out, ln, offs = case.check(case.call(ops, None, bounds=bounds_list))
            assert hasattr(out, '_guard') and hasattr(ln, '_guard')
            return ln, stream_bytes(out, ln, offs)
        both_fills(run)


@pytest.mark.parametrize('n_sym,scale', RANGE_DECODE_CASES)
def test_range_decode(n_sym, scale, oracle, cuda):
    """payload (staged through ops' own device buffer, now an arena) and CDF rows guarded; full rows and windows of whole maps,
    two streams side by side into a flat output"""
    run_guarded(range_coder_case(oracle, n_sym, scale, trim=False, windows=True), cuda, encode=False)


def test_range_decode_pmf_tables(oracle, cuda):
    run_guarded(range_coder_pmf_case(oracle, 11), cuda, encode=False)


@pytest.mark.parametrize('n', [0, 1, 1000, 16385])
def test_bounds_rate(n, oracle, cuda):
    from aivc_amd import ops
    case = bounds_rate_case(oracle, 11 + n, n)

    def run(fill):
        d = case.place(G(cuda, fill))
        got = case.check(case.call(ops, d))
        own = guarded_empty((3,), torch.float64, cuda, fill)  # `out`: a 1-element view to fill, its neighbours untouched
        ops.bounds_rate(d['b'], out=own[1:2])
        assert float(own[1].cpu()) == case.want and poisoned(own[:1], fill) and poisoned(own[2:], fill)
        return got, own[1:2]
    both_fills(run)


@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (2, 5, 7, 9), (1, 4, 3, 130)])
def test_rate_estimates(shape, oracle, cuda):
    """laplace_prob with and without mu, table_prob, rate_bits"""
    run_guarded(rate_estimates_case(oracle, shape[-1], shape), cuda)


# ---- the regimes of tests/op_regimes.py ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case_id', sorted(REGIME_CASES))
def test_op_regimes(case_id, oracle, cuda):
    """every builder of tests/op_regimes.py once more: non-finite flows, pixels, latents and sigmas next to the guards"""
    run_guarded(REGIME_CASES[case_id](oracle), cuda)


# ---- deterministic transcendentals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 63, 4097])
def test_detmath_eval(n, oracle, cuda):
    """every function id of aivc_detmath_eval: one element, less than a wavefront, more than a block's stride"""
    from detmath_cases import sample
    for fn in range(abi.DETMATH_COUNT):
        run_guarded(detmath_case(oracle, fn, *sample(fn, n, 100 * fn + n)), cuda)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,ws', [(2, 2, 1), (5, 7, 5), (37, 53, 11), (64, 129, 6)])
def test_metrics(h, w, ws, cuda):
    """ssim_means (its workspace, sized by aivc_metrics_workspace, is an arena too), pool2x2 with both edges, sq_err; the
    tolerances of tests/test_gpu_metrics.py"""
    from oracle import oracle
    run_guarded(metrics_case(oracle, h, w, ws), cuda)


def test_ops_is_left_as_it_was():
    from aivc_amd import ops
    assert ops.torch is torch and ops.PROFILE is None
