"""Every device entry point of aivc_amd.ops under the guard-zone and poison harness of tests/guarded.py (read its docstring first:
what an arena is, why there are two fills, what the method cannot see).

Each case runs twice, once per fill.  Its inputs go in through guarded(...): they sit flush against 1 MiB of poison on both
sides.  The call runs inside guard_ops(fill): every output and scratch buffer ops allocates is an arena too, and its untouched
payload is poison.  The result is compared with the CPU oracle exactly as the existing test of that operation compares it (bit
exact; 1e-12 for ssim_means and sq_err; the reference-run fixture and its stated bounds for the warp modes; the bf16x3 mode, which
has no oracle, against its own unguarded run).  Then the guards are checked and the two runs are compared byte for byte.  So a
store outside an output, an output element that is not written and a read outside an input that reaches the result each fail a case.

The case tables are the existing ones (test_gpu_ops.py, test_gpu_winograd.py, test_gpu_gdn_resident.py, warp_modes_cases.py),
imported, and the conv tests assert through ops.PROFILE which kernel variant took the launch.

ops.range_encode's inputs stay plain tensors (see tests/guarded.py); its outputs are guarded."""
import os
import sys

import numpy as np
import pytest
import torch

from aivc_amd import abi

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from guarded import both_fills, guarded, guarded_empty  # noqa: E402
from test_gpu_gdn_resident import CASES as GDN_RESIDENT_CASES  # noqa: E402
from test_gpu_ops import (CONV_CASES, CONV_IMAGES_CASES, FUSED_GDN_CASES, FUSED_TAIL_CASES, THIN_WALK_CASES, THIN_WALK_GRIDS, T,  # noqa: E402
                          eq)
from test_gpu_winograd import CASES as WINO_CASES, POLY_CASES, TC_CASES  # noqa: E402
from warp_modes_cases import BICUBIC_REFERENCE_DEVIATION, CASES as WARP_CASES, case_key, left_out  # noqa: E402

pytestmark = pytest.mark.gpu

ALGOS = [abi.ALGO_DIRECT, abi.ALGO_AUTO, abi.ALGO_MFMA]
MODE_DIGIT = {abi.MODE_CONV: 0, abi.MODE_TCONV: 1, abi.MODE_GDN: 2, abi.MODE_IGDN: 2}
TILES = (0, 1, 2, 3, 5, 6)


def G(a, dev, fill):
    return None if a is None else guarded(a, dev, fill)


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


def _assert_route(codes, route, mode):
    assert len(codes) == 1, codes
    code = codes[0]
    if route == 'direct':
        assert code == 0, codes
    elif route == 'resident':
        assert code == 400, codes
    elif route == 'thin':
        assert code in (1, 2), codes
    else:
        assert code // 10 == 10 + MODE_DIGIT[mode] and code % 10 in TILES, codes


@pytest.mark.parametrize('idx', range(len(CONV_CASES)))
def test_conv_family(idx, oracle, cuda):
    from aivc_amd import ops
    case = CONV_CASES[idx]
    mode, k, s, pad, ci, co, h, w, a1, a2, use_mul, use_res = case
    rng = np.random.default_rng(1000 + idx)
    x = rng.standard_normal((2, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    if mode in (abi.MODE_GDN, abi.MODE_IGDN):
        wt = np.abs(wt) * 0.1
        bias = np.abs(bias) + 0.1
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    mul = rng.standard_normal((2, ho, wo, co), dtype=np.float32) if use_mul else None
    res = rng.standard_normal((2, ho, wo, co), dtype=np.float32) if use_res else None
    ref = oracle.conv2d(x, wt, bias, mode=mode, stride=s, pad=pad, act1=a1, act2=a2, mul=mul, res=res)
    for algo in ALGOS:
        def run(fill):
            got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(bias, cuda, fill), mode=mode, stride=s, pad=pad,
                                                     act1=a1, act2=a2, mul=G(mul, cuda, fill), res=G(res, cuda, fill), algo=algo))
            _assert_route(codes, _route(mode, k, ci, co, algo), mode)
            eq(got, ref)
            return got
        both_fills(run)


@pytest.mark.parametrize('idx', range(len(FUSED_GDN_CASES)))
def test_fused_gdn(idx, oracle, cuda):
    from aivc_amd import ops
    mode, k, s, pad, ci, co, h, w, inv, use_res = FUSED_GDN_CASES[idx]
    rng = np.random.default_rng(2000 + idx)
    x = rng.standard_normal((2, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    beta = (np.abs(rng.standard_normal(co)) + 0.2).astype(np.float32)
    gamma = (np.abs(rng.standard_normal((co, co))) * 0.05).astype(np.float32)
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    res = rng.standard_normal((2, ho, wo, co), dtype=np.float32) if use_res else None
    want = oracle.conv2d(x, wt, bias, mode=mode, stride=s, pad=pad, res=res, gdn=(beta, gamma, inv))
    fusable = co in (32, 64, 128)

    def run(fill):
        got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(bias, cuda, fill), mode=mode, stride=s, pad=pad,
                                                 res=G(res, cuda, fill), gdn=(G(beta, cuda, fill), G(gamma, cuda, fill), inv)))
        if fusable:  # 150 + 10 * mode + tile: the fused epilogue in one launch
            assert len(codes) == 1 and codes[0] // 10 == 15 + MODE_DIGIT[mode] and codes[0] % 10 in TILES, codes
        else:
            assert len(codes) == 2 and all(c < 150 for c in codes), codes
        eq(got, want)
        return got
    both_fills(run)


@pytest.mark.parametrize('idx', range(len(FUSED_TAIL_CASES)))
def test_fused_tail(idx, oracle, cuda):
    from aivc_amd import ops
    k, s, ci, cm, ct, n, h, w, a1, a2, use_res = FUSED_TAIL_CASES[idx]
    rng = np.random.default_rng(3000 + idx)
    x = rng.standard_normal((n, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((cm, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    b1 = rng.standard_normal(cm, dtype=np.float32)
    cm4 = (cm + 3) // 4 * 4
    w3 = np.zeros((ct, 1, 1, cm4), dtype=np.float32)
    w3[..., :cm] = rng.standard_normal((ct, 1, 1, cm), dtype=np.float32) / np.sqrt(cm)
    b3 = rng.standard_normal(ct, dtype=np.float32)
    ho, wo = abi.conv_out_size(abi.MODE_CONV, h, w, k, s, k // 2)
    res = rng.standard_normal((n, ho, wo, ct), dtype=np.float32) if use_res else None
    t = oracle.conv2d(x, wt, b1, stride=s, pad=k // 2, act1=a1)
    if cm4 != cm:
        t = np.concatenate([t, np.zeros(t.shape[:3] + (cm4 - cm,), np.float32)], axis=-1)
    want = oracle.conv2d(t, w3, b3, res=res, act2=a2)
    assert ops.PRECISION == abi.PREC_FP32_WINO and not ops.WINO_ANY_SIZE
    covered = k == 3 and s == 1 and ci % 32 == 0 and cm % 128 == 0 and h * w >= 8000
    fusable = cm == 64 and ct == 128 and ci % 32 == 0

    def run(fill):
        got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(b1, cuda, fill), stride=s, pad=k // 2, act1=a1, act2=a2,
                                                 res=G(res, cuda, fill), tail=(G(w3, cuda, fill), G(b3, cuda, fill))))
        if fusable:
            assert codes == [190], codes
        elif covered:
            assert len(codes) == 2 and codes[0] == 301 and codes[1] not in ops._WINO_VARIANTS, codes
        else:
            assert len(codes) == 2 and 190 not in codes and not set(codes) & set(ops._WINO_VARIANTS), codes
        eq(got, want)
        return got
    both_fills(run)


@pytest.mark.parametrize('case', [c for c in GDN_RESIDENT_CASES if c[1] * c[2] * c[3] <= 4096])
def test_gdn_resident(case, oracle, cuda):
    """stand-alone (I)GDN with gamma resident in registers: variant 400"""
    from aivc_amd import ops
    c, n, h, w, inv, use_res = case
    rng = np.random.default_rng(c * 1000 + n * 100 + h + w + (5 if inv else 0))
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    beta = (np.abs(rng.standard_normal(c)) + 0.2).astype(np.float32)
    gamma = (np.abs(rng.standard_normal((c, c))) * 0.05).astype(np.float32)
    res = rng.standard_normal((n, h, w, c), dtype=np.float32) if use_res else None
    want = oracle.gdn(x, beta, gamma, inverse=inv, res=res)

    def run(fill):
        got, codes = profiled(lambda: ops.gdn(G(x, cuda, fill), G(beta, cuda, fill), G(gamma, cuda, fill), inverse=inv, res=G(res, cuda, fill)))
        assert codes == [400], codes
        eq(got, want)
        return got
    both_fills(run)


@pytest.mark.parametrize('grid', THIN_WALK_GRIDS)
@pytest.mark.parametrize('co,k,ci,h,w', THIN_WALK_CASES)
def test_thin_layer_tile_walk(grid, co, k, ci, h, w, oracle, cuda, monkeypatch):
    """few persistent groups walking several tiles each over 3 images (AIVC_THIN_GRID_MAX): the 16x16x4 MFMA kernel, variant 2"""
    from aivc_amd import ops
    monkeypatch.setenv('AIVC_THIN_GRID_MAX', str(grid))
    rng = np.random.default_rng(grid * 100 + co)
    x = rng.standard_normal((3, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    ref = oracle.conv2d(x, wt, bias, mode=abi.MODE_TCONV, stride=2, pad=0, act1=abi.ACT_LEAKY)

    def run(fill):
        got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(bias, cuda, fill), mode=abi.MODE_TCONV, stride=2, pad=0,
                                                 act1=abi.ACT_LEAKY))
        assert codes == [2], codes
        eq(got, ref)
        return got
    both_fills(run)


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
    from aivc_amd import ops
    n, h, w, ci, co, a1, a2, has_b, has_m, has_r = case
    k, s, pad, mode = {301: (3, 1, 1, abi.MODE_CONV), 302: (5, 2, 2, abi.MODE_CONV), 303: (5, 2, 0, abi.MODE_TCONV)}[variant]
    rng = np.random.default_rng(variant * 100 + n * 10 + h)
    x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
    wt = (rng.standard_normal((co, k, k, ci)) / np.sqrt(k * k * ci / (4 if mode == abi.MODE_TCONV else 1))).astype(np.float32)
    b = (rng.standard_normal(co) * 0.1).astype(np.float32) if has_b else None
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    m = rng.standard_normal((n, ho, wo, co)).astype(np.float32) if has_m else None
    r = rng.standard_normal((n, ho, wo, co)).astype(np.float32) if has_r else None
    want = oracle.conv2d(x, wt, b, mode=mode, stride=s, pad=pad, act1=a1, act2=a2, mul=m, res=r)

    def run(fill):
        got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(b, cuda, fill), mode=mode, stride=s, pad=pad, act1=a1,
                                                 act2=a2, mul=G(m, cuda, fill), res=G(r, cuda, fill)))
        assert codes == [variant], codes
        eq(got, want)
        return got
    both_fills(run)


@pytest.mark.parametrize('c_in', [8, 32])
@pytest.mark.parametrize('form', ['3x3', 'poly5', 'tconv5'])
def test_winograd_weight_transforms(form, c_in, oracle, cuda):
    from aivc_amd import ops
    k = 3 if form == '3x3' else 5
    wt = (np.random.default_rng(100 + c_in + k).standard_normal((64, k, k, c_in)) * 3).astype(np.float32)
    want = np.asarray(oracle.winograd_weights(wt, transposed=form == 'tconv5')).ravel()

    def run(fill):
        u = ops.winograd_weights(G(wt, cuda, fill), transposed=form == 'tconv5')
        assert hasattr(u, '_guard') and u.numel() == want.size
        eq(u, want)
        return u
    both_fills(run)


BF16X3_CASES = [  # mode, k, stride, pad, c_in, c_out, h, w, fused gdn (0 / 1 / 2), variant with the weights split ahead, in the K loop
    (abi.MODE_CONV, 3, 1, 1, 64, 128, 9, 11, 0, 1100, 1100),
    (abi.MODE_CONV, 5, 2, 2, 128, 64, 13, 15, 0, 1106, 1102),
    (abi.MODE_TCONV, 5, 2, 0, 128, 128, 5, 7, 2, 1165, 1160),
]


@pytest.mark.parametrize('case', BF16X3_CASES)
def test_bf16x3_mode(case, cuda):
    """The precision mode has no oracle (its bits are its own): the unguarded run of the same launch stands in, the weights
    split ahead of the launch and by the K loop give the same bits (csrc/conv_bf16x3.hip), and the two fills must agree."""
    from aivc_amd import ops
    mode, k, s, pad, ci, co, h, w, gdn, v_ahead, v_loop = case
    rng = np.random.default_rng(4000 + co + k)
    x = rng.standard_normal((2, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    b = rng.standard_normal(co, dtype=np.float32)
    beta = (np.abs(rng.standard_normal(co)) + 0.5).astype(np.float32)
    gamma = (np.abs(rng.standard_normal((co, co))) * 0.02).astype(np.float32)
    prev, prev_split = ops.set_precision('bf16x3'), ops.PRESPLIT_WEIGHTS
    try:
        g = None if not gdn else (T(beta, cuda), T(gamma, cuda), gdn == 2)
        plain = ops.conv2d(T(x, cuda), T(wt, cuda), T(b, cuda), mode=mode, stride=s, pad=pad, gdn=g).cpu().numpy()
        assert np.isfinite(plain).all()
        for ahead, variant in ((True, v_ahead), (False, v_loop)):
            ops.PRESPLIT_WEIGHTS = ahead

            def run(fill):
                gg = None if not gdn else (G(beta, cuda, fill), G(gamma, cuda, fill), gdn == 2)
                got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(b, cuda, fill), mode=mode, stride=s, pad=pad, gdn=gg))
                assert codes == [variant], codes
                eq(got, plain)
                return got
            both_fills(run)
    finally:
        ops.PRESPLIT_WEIGHTS = prev_split
        ops.set_precision(prev)


@pytest.mark.parametrize('tile,c_in', [(t, ci) for ci in (32, 12) for t in TILES if t != 2 or ci % 32 == 0])
def test_every_mfma_tile(tile, c_in, oracle, cuda, monkeypatch):
    """AIVC_FORCE_TILE: 0 = 128x128, 1 = 64x64, 2 = 256x64, 3 = 128x32, 5 = 64x128, 6 = 128x64 on M = 2 * 9 * 13 = 234 rows and
    72 output channels (multiples of no tile side): partial tiles along both; c_in 32 takes the LDS-DMA K loop, 12 the generic
    loader (which the 256-row tile is not instantiated for)"""
    from aivc_amd import ops
    monkeypatch.setenv('AIVC_FORCE_TILE', str(tile))
    rng = np.random.default_rng(5000 + tile + c_in)
    x = rng.standard_normal((2, 9, 13, c_in), dtype=np.float32)
    wt = (rng.standard_normal((72, 3, 3, c_in), dtype=np.float32) / np.sqrt(9 * c_in)).astype(np.float32)
    b = rng.standard_normal(72, dtype=np.float32)
    res = rng.standard_normal((2, 9, 13, 72), dtype=np.float32)
    want = oracle.conv2d(x, wt, b, stride=1, pad=1, act1=abi.ACT_LEAKY, res=res)

    def run(fill):
        got, codes = profiled(lambda: ops.conv2d(G(x, cuda, fill), G(wt, cuda, fill), G(b, cuda, fill), stride=1, pad=1, act1=abi.ACT_LEAKY,
                                                 res=G(res, cuda, fill), algo=abi.ALGO_MFMA))
        assert codes == [100 + tile], codes
        eq(got, want)
        return got
    both_fills(run)


# ---- conv_images and pack_images -------------------------------------------------------------------------------------------------
def _image_parts(rng, n, h, w):
    hc, wc = (h + 1) // 2, (w + 1) // 2

    def planes():
        return {'y': rng.integers(0, 256, (n, h, w), dtype=np.uint8), 'u': rng.integers(0, 256, (n, hc, wc), dtype=np.uint8),
                'v': rng.integers(0, 256, (n, hc, wc), dtype=np.uint8)}
    a, b = planes(), planes()
    f4 = rng.standard_normal((n, h, w, 4)).astype(np.float32)
    f4[..., 3] = 0.0
    f3 = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    return a, b, f3, f4


def _guard_parts(parts, dev, fill):
    return [{k: guarded(p[k], dev, fill) for k in 'yuv'} if isinstance(p, dict) else G(p, dev, fill) for p in parts]


IMAGE_SIZES = [c for c in CONV_IMAGES_CASES if c[0] % 2 and c[1] % 2]  # odd h and w: ceil-sized chroma planes flush against their guard
assert [c[:2] for c in IMAGE_SIZES] == [(9, 13), (35, 131)]


@pytest.mark.parametrize('h,w,n', IMAGE_SIZES)
@pytest.mark.parametrize('use_gdn', [True, False])
def test_conv_images(h, w, n, use_gdn, oracle, cuda, monkeypatch):
    """aivc_conv_images (variant 191) on 1 / 2 / 3 images: 8-bit 4:2:0 planes, float sources of 3 and 4 channels, a None part"""
    from aivc_amd import ops
    monkeypatch.setattr(ops, '_CONV_IMAGES_MAX', 3)
    rng = np.random.default_rng(h * 1000 + w + (7 if use_gdn else 0))
    a, b, f3, f4 = _image_parts(rng, n, h, w)
    for parts_np in ([a], [f4], [f3], [a, b], [a, f3], [a, b, a], [f4, a, None]):
        ni = len(parts_np)
        wt = np.zeros((64, 5, 5, 4 * ni), np.float32)
        for i in range(ni):
            wt[..., 4 * i:4 * i + 3] = rng.standard_normal((64, 5, 5, 3)).astype(np.float32) / np.sqrt(75 * ni)
        bias = rng.standard_normal(64, dtype=np.float32)
        g = None
        if use_gdn:
            g = ((np.abs(rng.standard_normal(64)) + 0.2).astype(np.float32), (np.abs(rng.standard_normal((64, 64))) * 0.05).astype(np.float32), False)
        act1 = 0 if use_gdn else abi.ACT_LEAKY
        want = oracle.conv2d(oracle.pack_images(parts_np, h, w), wt, bias, stride=2, pad=2, act1=act1, gdn=g)

        def run(fill):
            stack = ops.ImageStack(_guard_parts(parts_np, cuda, fill), h, w, cuda)
            gt = None if g is None else (G(g[0], cuda, fill), G(g[1], cuda, fill), False)
            got, codes = profiled(lambda: ops.conv2d(stack, G(wt, cuda, fill), G(bias, cuda, fill), stride=2, pad=2, act1=act1, gdn=gt))
            assert codes == [191] and stack._packed is None, codes
            eq(got, want)
            return got
        both_fills(run)


@pytest.mark.parametrize('h,w,n', IMAGE_SIZES)
def test_pack_images(h, w, n, oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(h * 1000 + w)
    a, b, f3, f4 = _image_parts(rng, n, h, w)
    for parts_np in ([a], [f3], [a, None], [a, b, None], [a, f4], [a, b, a], [None, f3, b]):
        want = oracle.pack_images(parts_np, h, w)

        def run(fill):
            got = ops.pack_images(_guard_parts(parts_np, cuda, fill), h, w, cuda)
            eq(got, want)
            return got
        both_fills(run)


# ---- pixel operations ------------------------------------------------------------------------------------------------------------
PLANE_SIZES = [(1, 1), (9, 13), (6, 1028)]


@pytest.mark.parametrize('h,w', PLANE_SIZES)
@pytest.mark.parametrize('u8', [True, False])
def test_yuv420_to_444(h, w, u8, oracle, cuda):
    """every stored layout: c_store 3 / 4 / 8, c_off 0 / 4, into a fresh tensor and into the caller's (whose other channels stay)"""
    from aivc_amd import ops
    rng = np.random.default_rng(h * 10 + w)
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y, u, v = (rng.integers(0, 256, (2, hh, ww), dtype=np.uint8) for hh, ww in ((h, w), (hc, wc), (hc, wc)))
    if not u8:
        y, u, v = (a.astype(np.float32) / np.float32(255) for a in (y, u, v))
    orc = oracle.yuv420u8_to_444 if u8 else oracle.yuv420_to_444
    for c_store, c_off in ((3, 0), (4, 0), (8, 0), (8, 4)):
        for own_out in (False, True):
            base = np.full((2, h, w, c_store), 7.0, np.float32) if own_out else np.zeros((2, h, w, c_store), np.float32)
            want = orc(y, u, v, c_store=c_store, c_off=c_off, out=base.copy())
            if c_store >= c_off + 4:
                want[..., c_off + 3] = 0.0  # (the image's zero pad channel: ops asks the kernel to write it)
            untouched = [c for c in range(c_store) if not c_off <= c < c_off + 4]
            assert np.array_equal(want[..., untouched], base[..., untouched])

            def run(fill):
                out = G(base, cuda, fill) if own_out else None
                got = ops.yuv420_to_444(G(y, cuda, fill), G(u, cuda, fill), G(v, cuda, fill), c_store=c_store, c_off=c_off, out=out)
                assert out is None or got is out
                assert hasattr(got, '_guard')
                eq(got, want)
                return got
            both_fills(run)


@pytest.mark.parametrize('h,w', PLANE_SIZES + [(10, 14)])
def test_frame_to_yuv420(h, w, oracle, cuda):
    """4 stored channels with margins (scalar path) and the 3-channel even-pitch hand-over of the codec (vector path when the
    frame sides are even), with and without the skip frame, floats and bytes or bytes alone"""
    from aivc_amd import ops
    rng = np.random.default_rng(5 + h + w)
    x = (rng.standard_normal((2, h + 3, w + 2, 4), dtype=np.float32) * 0.4 + 0.5).astype(np.float32)
    skip = (rng.standard_normal((2, h, w, 4), dtype=np.float32) * 0.1).astype(np.float32)
    x3 = np.ascontiguousarray(x[:, :, :w + 2 - (w & 1), :3])
    for src in (x, x3):
        for sk in (None, skip):
            rf, rb = oracle.frame_to_yuv420(src, h, w, skip=sk)
            for want_float in (True, False):
                def run(fill):
                    gf, gb = ops.frame_to_yuv420(G(src, cuda, fill), h, w, skip=G(sk, cuda, fill), want_float=want_float)
                    for a, b in zip(gb, rb):
                        eq(a, b)
                    if want_float:
                        for a, b in zip(gf, rf):
                            eq(a, b)
                    else:
                        assert gf == (None, None, None)
                    return gf, gb
                both_fills(run)


@pytest.mark.parametrize('h,w,s', [(9, 13, 3.0), (8, 8, 30.0), (5, 1, 2.0), (1, 1, 1.0)])
def test_warp(h, w, s, oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(6 + h)
    x = rng.standard_normal((2, h, w, 4), dtype=np.float32)
    flow = (rng.standard_normal((2, h, w, 2), dtype=np.float32) * s).astype(np.float32)
    want = oracle.warp(x, flow)

    def run(fill):
        got = ops.warp(G(x, cuda, fill), G(flow, cuda, fill))
        eq(got, want)
        return got
    both_fills(run)


BICUBIC_ATOL = 4 * BICUBIC_REFERENCE_DEVIATION  # (the bound of tests/test_gpu_warp_modes.py, derived there)


@pytest.mark.parametrize('s,mode,pad,ac', WARP_CASES, ids=[case_key(*c) for c in WARP_CASES])
def test_warp_modes(s, mode, pad, ac, cuda, golden):
    """every sampling mode against the reference-run fixture, with the bounds and the left-out pixels of tests/test_gpu_warp_modes.py"""
    from aivc_amd import ops
    g = golden('warp_modes')
    x = np.ascontiguousarray(np.transpose(g['x_%d' % s], (0, 2, 3, 1)))
    flow = np.ascontiguousarray(np.transpose(g['flow_%d' % s], (0, 2, 3, 1)))
    want = g['y_' + case_key(s, mode, pad, ac)]
    keep = np.broadcast_to(~left_out(g, s, mode, pad, ac)[:, None], want.shape)
    gone = np.broadcast_to((g['m_' + case_key(s, mode, pad, ac)] < 0.9998)[:, None], want.shape)

    def run(fill):
        y = ops.warp(G(x, cuda, fill), G(flow, cuda, fill), mode, pad, ac)
        got = np.transpose(y.cpu().numpy(), (0, 3, 1, 2))
        if mode == 'bicubic':
            np.testing.assert_allclose(got[keep], want[keep], rtol=0, atol=BICUBIC_ATOL)
        else:
            np.testing.assert_allclose(got[keep], want[keep], rtol=1e-5, atol=2e-6)
        if (mode, pad, ac) != ('bilinear', 'border', True):  # (the codec's mode has no mask)
            assert (got[gone] == 0).all()
        return y
    both_fills(run)


def _warp_blend_inputs(h, w, s, seed):
    rng = np.random.default_rng(seed)
    mof = rng.standard_normal((2, h + 2, w + 1, 8), dtype=np.float32)
    mof[..., 2:6] *= np.float32(s)
    return mof, rng.random((2, h, w, 4), dtype=np.float32), rng.random((2, h, w, 4), dtype=np.float32)


AUX = ('pred', 'skip', 'x_warp', 'alpha', 'beta')


@pytest.mark.parametrize('h,w,s', [(9, 13, 3.0), (8, 8, 30.0), (5, 1, 2.0)])
@pytest.mark.parametrize('ft', [1, 2])
@pytest.mark.parametrize('general', [False, True])
def test_warp_blend(h, w, s, ft, general, oracle, cuda):
    """both frame types on the 16-byte fast path (4 / 4 / 8 channels) and the general kernel (3 / 3 / 7), with and without the
    auxiliary outputs"""
    from aivc_amd import ops
    mof, prev, nxt = _warp_blend_inputs(h, w, s, 60 + h)
    co = 4
    if general:
        mof, prev, nxt, co = np.ascontiguousarray(mof[..., :7]), prev[..., :3].copy(), nxt[..., :3].copy(), 3
    want = oracle.warp_blend(mof, prev, nxt, h, w, ft, co=co)
    for want_aux in (True, False):
        def run(fill):
            g = ops.warp_blend(G(mof, cuda, fill), G(prev, cuda, fill), G(nxt, cuda, fill), h, w, ft, co=co, want_aux=want_aux)
            for kk in AUX if want_aux else AUX[:2]:
                eq(g[kk], want[kk])
            assert want_aux or all(g[kk] is None for kk in AUX[2:])
            return g
        both_fills(run)


@pytest.mark.parametrize('rows', [(0, 4), (4, 5), (9, 4), (0, 13), (12, 1)])
@pytest.mark.parametrize('ft', [1, 2])
@pytest.mark.parametrize('general', [False, True])
def test_warp_blend_rows(rows, ft, general, oracle, cuda):
    """a first, a middle and a last band of a 13-row frame (and the whole frame, and one row): the band of the MOFNet output in,
    whole reference frames in, the band's rows out -- equal to the oracle's band and to the rows of the oracle's whole frame"""
    from aivc_amd import ops
    h, w = 13, 11
    row0, nr = rows
    mof, prev, nxt = _warp_blend_inputs(h, w, 4.0, 70)
    co = 4
    if general:
        mof, prev, nxt, co = np.ascontiguousarray(mof[..., :7]), prev[..., :3].copy(), nxt[..., :3].copy(), 3
    band = np.ascontiguousarray(mof[:, row0:row0 + nr])
    want = oracle.warp_blend(band, prev, nxt, h, w, ft, co=co, rows=rows)
    whole = oracle.warp_blend(mof, prev, nxt, h, w, ft, co=co)
    for kk in AUX:
        np.testing.assert_array_equal(want[kk], whole[kk][:, row0:row0 + nr])

    def run(fill):
        g = ops.warp_blend(G(band, cuda, fill), G(prev, cuda, fill), G(nxt, cuda, fill), h, w, ft, co=co, want_aux=True, rows=rows)
        for kk in AUX:
            assert g[kk].shape[1] == nr
            eq(g[kk], want[kk])
        return g
    both_fills(run)


@pytest.mark.parametrize('h,w', [(6, 8), (7, 9), (6, 9), (7, 8), (2, 2), (3, 67)])
def test_downsample2x(h, w, oracle, cuda):
    """2x2 means of a channel range that does not start at 0, planar output; an odd side drops its last row / column"""
    from aivc_amd import ops
    rng = np.random.default_rng(h * 100 + w)
    x = rng.standard_normal((2, h, w, 6), dtype=np.float32)
    for ch0, nch in ((1, 2), (3, 3), (0, 6), (5, 1)):
        want = oracle.downsample2x(x, ch0, nch)
        assert want.shape == (2, nch, h // 2, w // 2)

        def run(fill):
            got = ops.downsample2x(G(x, cuda, fill), ch0, nch)
            eq(got, want)
            return got
        both_fills(run)


@pytest.mark.parametrize('lam', [0.0, 1.0, 0.3])
@pytest.mark.parametrize('n', [1, 13, 192])
def test_gain_interp(lam, n, oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(n)
    g_r, g_t = (np.exp(rng.standard_normal(n)).astype(np.float32) for _ in range(2))
    want = oracle.gain_interp(g_r, g_t, lam)

    def run(fill):
        got = ops.gain_interp(G(g_r, cuda, fill), G(g_t, cuda, fill), lam)
        eq(got, want)
        return got
    both_fills(run)


@pytest.mark.parametrize('c_in,c_out', [(3, 4), (6, 8), (13, 16)])
@pytest.mark.parametrize('shape', [(1, 1, 1), (2, 5, 7), (1, 3, 129)])
def test_pad_channels(c_in, c_out, shape, oracle, cuda):
    from aivc_amd import ops
    x = np.random.default_rng(c_in).standard_normal(shape + (c_in,), dtype=np.float32)
    want = oracle.pad_channels(x, c_out)
    assert want.shape == shape + (c_out,) and np.array_equal(want[..., :c_in], x) and not want[..., c_in:].any()

    def run(fill):
        got = ops.pad_channels(G(x, cuda, fill), c_out)
        eq(got, want)
        return got
    both_fills(run)


def test_latent_ops(oracle, cuda):
    """hyper_params, channel_gain, quantize_center with and without y_hat / mu / gain, dequantize, gdn_reparam"""
    from aivc_amd import ops
    rng = np.random.default_rng(7)
    hs = (rng.standard_normal((1, 6, 9, 16), dtype=np.float32) * 8).astype(np.float32)
    hs[0, 0, 0, 8], hs[0, 0, 1, 8] = -30, 30
    mu, sg = oracle.hyper_params(hs, 8, 5, 7)
    y = (rng.standard_normal((1, 5, 7, 8), dtype=np.float32) * 20).astype(np.float32)
    y[0, 0, 0, :4] = [0.5, 1.5, 2.5, -0.5]
    y[0, 0, 1, :2] = [400, -400]
    gain = rng.standard_normal(8).astype(np.float32)
    want_gain = oracle.channel_gain(y, gain)
    q, yh = oracle.quantize_center(y, mu, gain)
    q0, yh0 = oracle.quantize_center(y)
    want_deq, want_deq0 = oracle.dequantize(q, mu, gain), oracle.dequantize(q0)
    beta = np.abs(rng.standard_normal(8)).astype(np.float32)
    gamma = (rng.standard_normal((8, 8)) * 0.1).astype(np.float32)
    be, ge = oracle.gdn_reparam(beta, gamma, 1e-3, 2 ** -18, 2 ** -36)

    def run(fill):
        d = lambda a: G(a, cuda, fill)
        out = {}
        out['mu'], out['sigma'] = ops.hyper_params(d(hs), 8, 5, 7)
        eq(out['mu'], mu), eq(out['sigma'], sg)
        out['gain'] = ops.channel_gain(d(y), d(gain))
        eq(out['gain'], want_gain)
        out['gain_none'] = ops.channel_gain(d(y), None)
        eq(out['gain_none'], oracle.channel_gain(y, None))
        out['q'], out['yh'] = ops.quantize_center(d(y), d(mu), d(gain))
        eq(out['q'], q), eq(out['yh'], yh)
        out['q0'], out['yh0'] = ops.quantize_center(d(y))
        eq(out['q0'], q0), eq(out['yh0'], yh0)
        out['q_only'], none = ops.quantize_center(d(y), d(mu), d(gain), want_yhat=False)
        assert none is None
        eq(out['q_only'], q)
        out['deq'] = ops.dequantize(d(q), d(mu), d(gain))
        eq(out['deq'], want_deq)
        out['deq0'] = ops.dequantize(d(q0))
        eq(out['deq0'], want_deq0)
        out['be'], out['ge'] = ops.gdn_reparam(d(beta), d(gamma), 1e-3, 2 ** -18, 2 ** -36)
        eq(out['be'], be), eq(out['ge'], ge)
        return out
    both_fills(run)


# ---- entropy model and rate ------------------------------------------------------------------------------------------------------
def _i16(a):
    return np.ascontiguousarray(a).view(np.int16)


def test_cdf_tables_and_single_frame_kernels(oracle, cuda):
    """balle_cdf_table with and without the float table; laplace_cdf_rows / laplace_cdf_windows into fresh tensors and into
    the caller's at a row offset (the rows before and behind still hold the fill); laplace_bounds, table_bounds, nonzero_flags"""
    from aivc_amd import ops
    rng = np.random.default_rng(8)
    params = (rng.standard_normal((6, abi.BALLE_PARAMS)) * 1.2).astype(np.float32)
    table, cdf = oracle.balle_cdf_table(params)
    sig = np.exp(rng.uniform(np.log(1e-4), np.log(148.4), (1, 5, 7, 8))).astype(np.float32)
    sig[0, 0, 0, 0], sig[0, 0, 0, 1] = 1e-4, 148.41316
    maps = [0, 2, 3, 7]
    npos = len(maps) * 35
    rows = oracle.laplace_cdf_rows(sig, maps)
    win, sp = oracle.laplace_cdf_windows(sig, maps)
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig), -256, 255).astype(np.int16)
    want_b = oracle.laplace_bounds(sig, q, maps)
    qz = rng.integers(-5, 6, (1, 3, 4, 6)).astype(np.int16)
    want_tb = oracle.table_bounds(table, qz)
    qb = np.clip(np.rint(rng.laplace(0, 1, (5, 6, 7, 8)) * 3), -256, 255).astype(np.int16)
    for i, dead in enumerate(([], [0], [1, 7], list(range(8)), [3])):
        qb[i][..., dead] = 0
    want_flags = np.array([[1 if k in oracle.nonzero_maps(qb[i:i + 1]) else 0 for k in range(8)] for i in range(5)], np.uint8)
    off = 3

    def run(fill):
        d = lambda a: G(a, cuda, fill)
        out = {}
        out['t'], out['c'] = ops.balle_cdf_table(d(params), want_float=True)
        eq(out['t'], table), eq(out['c'], cdf)
        out['t_only'] = ops.balle_cdf_table(d(params))
        eq(out['t_only'], table)
        out['rows'] = ops.laplace_cdf_rows(d(sig), maps)
        eq(out['rows'], rows)
        own = guarded_empty((off + npos + 2, abi.CDF_ROW), torch.int16, cuda, fill)
        assert ops.laplace_cdf_rows(d(sig), maps, out=own, row_off=off) is own
        eq(own[off:off + npos], rows)
        assert poisoned(own[:off], fill) and poisoned(own[off + npos:], fill)
        out['rows_own'] = own[off:off + npos]
        out['win'], out['sp'] = ops.laplace_cdf_windows(d(sig), maps)
        eq(out['win'], win), eq(out['sp'], sp)
        own_w = guarded_empty((off + npos + 2, abi.CDF_WIN), torch.int16, cuda, fill)
        own_s = guarded_empty((off + npos + 2,), torch.float32, cuda, fill)
        ops.laplace_cdf_windows(d(sig), maps, out=(own_w, own_s), row_off=off)
        eq(own_w[off:off + npos], win), eq(own_s[off:off + npos], sp)
        assert all(poisoned(t[:off], fill) and poisoned(t[off + npos:], fill) for t in (own_w, own_s))
        out['win_own'], out['sp_own'] = own_w[off:off + npos], own_s[off:off + npos]
        out['bounds'] = ops.laplace_bounds(d(sig), d(q), maps)
        eq(out['bounds'], want_b)
        out['tbounds'] = ops.table_bounds(d(_i16(table)), d(qz))
        eq(out['tbounds'], want_tb)
        out['flags'] = ops.nonzero_flags(d(qb))
        eq(out['flags'], want_flags)
        return out
    both_fills(run)


@pytest.mark.parametrize('shape,maps', [((5, 7, 9, 16), [[0, 3, 15], [], [1], list(range(16)), [2, 14]]),
                                        ((4, 5, 6, 12), [list(range(12)), [], [0, 11], [5]])])
def test_frame_batch_entropy_kernels(shape, maps, oracle, cuda):
    """the _batch forms on ragged per-frame map lists with a frame that codes nothing; c % 8 != 0 in the second shape"""
    from aivc_amd import ops
    n, h, w, c = shape
    npix = h * w
    rng = np.random.default_rng(21 + c)
    sig = (np.abs(rng.standard_normal(shape)) * 2 + 0.05).astype(np.float32)
    q = np.clip(np.rint(rng.standard_normal(shape) * sig), -256, 256).astype(np.int16)
    table = rng.integers(0, 65535, (c, abi.CDF_ROW)).astype(np.uint16)
    total = sum(len(m) for m in maps) * npix
    want_b = [oracle.laplace_bounds(sig[f:f + 1], q[f:f + 1], m) if m else None for f, m in enumerate(maps)]
    want_w = [oracle.laplace_cdf_windows(sig[f:f + 1], m) if m else None for f, m in enumerate(maps)]
    want_tb = np.stack([oracle.table_bounds(table, q[f:f + 1]) for f in range(n)])
    sym = np.concatenate([(q[f].reshape(npix, c)[:, m].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16) for f, m in enumerate(maps) if m])
    want_q = np.zeros_like(q)
    for f, m in enumerate(maps):
        want_q[f][..., m] = q[f][..., m]

    def run(fill):
        d = lambda a: G(a, cuda, fill)
        out = {}
        out['b'], offs = ops.laplace_bounds_batch(d(sig), d(q), maps)
        win = guarded_empty((total + 3, abi.CDF_WIN), torch.int16, cuda, fill)
        sp = guarded_empty((total + 3,), torch.float32, cuda, fill)
        offs2, tab = ops.laplace_cdf_windows_batch(d(sig), maps, (win, sp))
        assert offs2 == offs and hasattr(tab[0], '_guard')
        for f, m in enumerate(maps):
            if m:
                sl = slice(offs[f], offs[f] + len(m) * npix)
                eq(out['b'][sl], want_b[f])
                eq(win[sl], want_w[f][0]), eq(sp[sl], want_w[f][1])
        assert poisoned(win[total:], fill) and poisoned(sp[total:], fill)
        out['b'] = out['b'][:total]
        out['win'], out['sp'] = win[:total], sp[:total]
        out['tb'] = ops.table_bounds_batch(d(_i16(table)), d(q))
        eq(out['tb'], want_tb)
        out['q'] = ops.scatter_symbols_batch(d(_i16(sym)), maps, n, npix, c, table=tab)
        eq(out['q'].view(n, h, w, c), want_q)
        out['q2'] = ops.scatter_symbols_batch(d(_i16(sym)), maps, n, npix, c)  # (its own device table)
        eq(out['q2'].view(n, h, w, c), want_q)
        for f, m in enumerate(maps):
            if m:
                s1 = (q[f].reshape(npix, c)[:, m].T.reshape(-1).astype(np.int32) + 256).astype(np.uint16)
                out['q1_%d' % f] = ops.scatter_symbols(d(_i16(s1)), npix, c, m)
                eq(out['q1_%d' % f].view(h, w, c), want_q[f])
        return out
    both_fills(run)


def test_frames_that_code_nothing(oracle, cuda):
    """a batch in which no frame has a coded map: no launch, nothing written"""
    from aivc_amd import ops
    sig = np.full((2, 3, 4, 8), 1.0, np.float32)
    q = np.zeros((2, 3, 4, 8), np.int16)

    def run(fill):
        b, offs = ops.laplace_bounds_batch(G(sig, cuda, fill), G(q, cuda, fill), [[], []])
        win = guarded_empty((2, abi.CDF_WIN), torch.int16, cuda, fill)
        sp = guarded_empty((2,), torch.float32, cuda, fill)
        offs2, _ = ops.laplace_cdf_windows_batch(G(sig, cuda, fill), [[], []], (win, sp))
        assert offs == offs2 == [0, 0]
        assert poisoned(b, fill) and poisoned(win, fill) and poisoned(sp, fill)
        return offs
    both_fills(run)


@pytest.mark.parametrize('kernel', ['lanes', 'wave'])
def test_range_encode(kernel, oracle, cuda, monkeypatch):
    """plain inputs (the product's back-to-back detection runs on _base / storage_offset as ever), guarded outputs: separate
    tensors (concatenated), slices of one tensor (taken as they sit), more than 64 streams (two launches), ragged lengths"""
    from aivc_amd import ops
    monkeypatch.setenv('AIVC_RC_ENCODE', kernel)
    rng = np.random.default_rng(77)
    lens = [1, 7, 8, 9, 63, 64, 65, 500] + [int(v) for v in rng.integers(1, 400, 62)]
    streams = []
    for nsym in lens:
        sig = np.clip(np.exp(rng.uniform(np.log(0.05), np.log(40.0), (1, 1, nsym, 1))), 1e-4, 148.4).astype(np.float32)
        q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig / np.sqrt(2)), -256, 255).astype(np.int16)
        streams.append(oracle.laplace_bounds(sig, q, [0]))
    want = [oracle.range_encode(b) for b in streams]
    separate = [T(b.view(np.int32), cuda) for b in streams]
    one = T(np.concatenate(streams).view(np.int32), cuda)
    cuts = np.concatenate([[0], np.cumsum(lens)])
    slices = [one[cuts[i]:cuts[i + 1]] for i in range(len(lens))]
    for bounds_list in (separate, slices, separate[:1]):
        def run(fill):
            out, ln, offs = ops.range_encode(bounds_list)
            assert hasattr(out, '_guard') and hasattr(ln, '_guard')
            out_h, ln_h = out.cpu().numpy(), ln.cpu().numpy()
            got = [out_h[off:off + int(m)].tobytes() for (off, cap), m in zip(offs, ln_h)]
            assert got == want[:len(bounds_list)]
            return ln, got
        both_fills(run)


@pytest.mark.parametrize('n_sym,scale', [(1, 1.0), (65, 5.0), (1000, 0.05), (5000, 40.0)])
def test_range_decode(n_sym, scale, oracle, cuda):
    """payload (staged through ops' own device buffer, now an arena) and CDF rows guarded; full rows, pmf tables and windows"""
    from aivc_amd import ops
    rng = np.random.default_rng(n_sym)
    c = 4
    npix = (n_sym + c - 1) // c
    sig = np.clip(np.exp(rng.uniform(np.log(0.05), np.log(4.0), (1, 1, npix, c))) * scale, 1e-4, 148.4).astype(np.float32)
    q = np.clip(np.rint(rng.laplace(0, 1, sig.shape) * sig / np.sqrt(2)), -256, 255).astype(np.int16)
    maps = list(range(c))
    payload = oracle.range_encode(oracle.laplace_bounds(sig, q, maps))
    rows = oracle.laplace_cdf_rows(sig, maps)
    win, sp = oracle.laplace_cdf_windows(sig, maps)
    n_all = npix * c
    want, want_bits = oracle.range_decode(payload, rows, n_all, want_bits=True)

    def run(fill):
        d = lambda a: G(a, cuda, fill)
        out = {}
        (out['sym'],), out['bits'] = ops.range_decode([payload], d(_i16(rows)), [0], [n_all], [0], want_bits=True)
        eq(out['sym'], want)
        assert int(out['bits'].cpu()[0]) == want_bits
        (out['sym_w'],), out['bits_w'] = ops.range_decode([payload], d(_i16(win)), [0], [n_all], [0], sigma_pos=d(sp), want_bits=True)
        eq(out['sym_w'], want)
        assert int(out['bits_w'].cpu()[0]) == want_bits
        # two streams side by side, the second from its own row offset, flat output
        out['flat'] = ops.range_decode([payload, payload], d(_i16(np.concatenate([rows, rows]))), [0, n_all], [n_all, n_all], [0, 0], flat=True)
        eq(out['flat'], np.concatenate([want, want]))
        return out
    both_fills(run)


def test_range_decode_pmf_tables(oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(11)
    params = (rng.standard_normal((5, abi.BALLE_PARAMS)) * 0.8).astype(np.float32)
    table, _ = oracle.balle_cdf_table(params)
    qz = rng.integers(-3, 4, (1, 6, 7, 5)).astype(np.int16)
    payload = oracle.range_encode(oracle.table_bounds(table, qz))
    want = oracle.range_decode(payload, table, qz.size, plane=42)

    def run(fill):
        sym = ops.range_decode([payload], G(_i16(table), cuda, fill), [0], [qz.size], [42])[0]
        eq(sym, want)
        back = ops.scatter_symbols(sym, 42, 5, list(range(5)))
        eq(back, qz.reshape(42, 5))
        return sym, back
    both_fills(run)


@pytest.mark.parametrize('n', [0, 1, 1000, 16385])
def test_bounds_rate(n, oracle, cuda):
    from aivc_amd import ops
    rng = np.random.default_rng(11 + n)
    lo = rng.integers(0, 0xFFFF, n)
    hi = lo + 1 + (rng.integers(0, 0x10000, n) % (0x10000 - lo))
    b = (lo | ((hi & 0xFFFF) << 16)).astype(np.uint32)
    want = oracle.bounds_rate(b)

    def run(fill):
        got = ops.bounds_rate(G(b.view(np.int32), cuda, fill))
        assert float(got.cpu()) == want
        own = guarded_empty((3,), torch.float64, cuda, fill)  # `out`: a 1-element view to fill, its neighbours untouched
        ops.bounds_rate(G(b.view(np.int32), cuda, fill), out=own[1:2])
        assert float(own[1].cpu()) == want and poisoned(own[:1], fill) and poisoned(own[2:], fill)
        return got, own[1:2]
    both_fills(run)


@pytest.mark.parametrize('shape', [(1, 3, 1, 1), (2, 5, 7, 9), (1, 4, 3, 130)])
def test_rate_estimates(shape, oracle, cuda):
    """laplace_prob with and without mu, table_prob, rate_bits"""
    from aivc_amd import ops
    rng = np.random.default_rng(shape[-1])
    b, c, h, w = shape
    y = np.rint(rng.standard_normal(shape) * 6).astype(np.float32)
    mu = rng.standard_normal(shape).astype(np.float32)
    sigma = np.exp(rng.uniform(-3, 3, shape)).astype(np.float32)
    params = (rng.standard_normal((c, abi.BALLE_PARAMS)) * 0.8).astype(np.float32)
    _, cdf = oracle.balle_cdf_table(params)
    p_mu, p_zero = oracle.laplace_prob(y, mu, sigma), oracle.laplace_prob(y, None, sigma)
    p_z = oracle.table_prob(y, cdf)
    rate, total = oracle.rate_bits(p_zero, 2.0 ** -16, 1.0)

    def run(fill):
        d = lambda a: G(a, cuda, fill)
        out = {'p_mu': ops.laplace_prob(d(y), d(mu), d(sigma)), 'p_zero': ops.laplace_prob(d(y), None, d(sigma)),
               'p_z': ops.table_prob(d(y), d(cdf))}
        eq(out['p_mu'], p_mu), eq(out['p_zero'], p_zero), eq(out['p_z'], p_z)
        out['rate'], out['total'] = ops.rate_bits(d(p_zero), 2.0 ** -16, 1.0)
        eq(out['rate'], rate)
        assert float(out['total'].cpu()) == total
        return out
    both_fills(run)


# ---- metrics ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('h,w,ws', [(2, 2, 1), (5, 7, 5), (37, 53, 11), (64, 129, 6)])
def test_metrics(h, w, ws, cuda):
    """ssim_means (its workspace, sized by aivc_metrics_workspace, is an arena too), pool2x2 with both edges, sq_err; the
    tolerances of tests/test_gpu_metrics.py"""
    from aivc_amd import ops
    from oracle import metrics, oracle
    rng = np.random.default_rng(h * 100 + w)
    a = rng.uniform(0, 255, (3, h, w))
    b = np.clip(a + rng.normal(0, 9, a.shape), 0, 255)
    win = metrics.window_clic(ws, ws * 1.5 / 11)
    c1, c2 = (0.01 * 255) ** 2, (0.03 * 255) ** 2
    want_ssim = oracle.ssim_means(a, b, win, c1, c2)
    want_pool = [oracle.pool2x2(a, edge) for edge in (0, 1)]
    se_ref = oracle.sq_err(a, b)[0]
    ia, ib = np.rint(a), np.rint(b)

    def run(fill):
        d = lambda t: G(t, cuda, fill)
        out = {'ssim': ops.ssim_means(d(a), d(b), win, c1, c2)}
        np.testing.assert_allclose(out['ssim'].cpu().numpy(), want_ssim, rtol=0, atol=1e-12)
        for edge in (0, 1):
            out['pool%d' % edge] = ops.pool2x2(d(a), edge)
            np.testing.assert_array_equal(out['pool%d' % edge].cpu().numpy(), want_pool[edge])
        out['se'] = ops.sq_err(d(a), d(b))
        assert abs(out['se'].item() - se_ref) <= 1e-12 * se_ref
        out['se_int'] = ops.sq_err(d(ia), d(ib))  # integer-valued planes: the sum of squares is exact in fp64
        assert out['se_int'].item() == oracle.sq_err(ia, ib)[0]
        return out
    both_fills(run)


def test_ops_is_left_as_it_was():
    from aivc_amd import ops
    assert ops.torch is torch and ops.PROFILE is None
