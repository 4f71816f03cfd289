"""Row bands under version 2 of the arithmetic contract (the default, Winograd F(2x2, 3x3) chains) on the CPU: a caller can
turn bands on there (FrameCodec._banded), and a chain of layers that takes every Winograd form -- 3x3 stride 1, 5x5 stride 2
in polyphase form, transposed 5x5 -- gives on every rank of R thread ranks the whole map's bits in its valid rows, with
the ORACLE's conv as the per-slab kernel and the product's per-launch decision (ops.slab_contract) applied to it.  The GPU
twin (HIP kernels, whole codec, real processes): tests/test_gpu_bands_winograd.py."""
import ctypes
import threading
import types

import numpy as np
import pytest
import torch

from aivc_amd import abi, ops
from aivc_amd.bands import Band, BandCtx, ThreadComm
from aivc_amd.codec import FrameCodec


# ---- FrameCodec._banded: opt-in under version 2 --------------------------------------------------------------------
def _shard(**kw):
    return types.SimpleNamespace(R=4, **kw)


@pytest.fixture
def fp32w(monkeypatch):
    monkeypatch.setattr(ops, 'PRECISION', abi.PREC_FP32_WINO)
    monkeypatch.delenv('AIVC_BAND_LEVELS', raising=False)
    return monkeypatch


def test_banded_is_off_by_default_in_version_2(fp32w):
    assert FrameCodec._banded(_shard(), 1, 1080, 1920) is False
    assert FrameCodec._banded(_shard(band_levels=None), 1, 1080, 1920) is False


def test_banded_on_with_the_environment_in_version_2(fp32w):
    fp32w.setenv('AIVC_BAND_LEVELS', '1')
    assert FrameCodec._banded(_shard(), 1, 1080, 1920) is True
    fp32w.setenv('AIVC_BAND_LEVELS', '0')
    assert FrameCodec._banded(_shard(), 1, 1080, 1920) is False
    assert FrameCodec._banded(_shard(band_levels=True), 1, 1080, 1920) is False  # the environment wins, as in version 1


def test_banded_on_with_the_shard_switch_in_version_2(fp32w):
    assert FrameCodec._banded(_shard(band_levels=True), 1, 1080, 1920) is True
    assert FrameCodec._banded(_shard(band_levels=False), 1, 1080, 1920) is False
    assert FrameCodec._banded(_shard(band_levels=True), 4, 1080, 1920) is False  # a level as wide as the group: frame sharding


def test_banded_automatic_rule_unchanged_in_version_1(monkeypatch):
    monkeypatch.setattr(ops, 'PRECISION', abi.PREC_FP32)
    monkeypatch.delenv('AIVC_BAND_LEVELS', raising=False)
    assert FrameCodec._banded(_shard(), 1, 1080, 1920) is True
    assert FrameCodec._banded(types.SimpleNamespace(R=2), 1, 1080, 1920) is False


# ---- a Winograd chain through BandCtx ------------------------------------------------------------------------------
_LOCK = threading.Lock()
_A = 1 << 20  # stand-in pointers: aivc_conv2d_variant reads the shape, never the memory


def _params(x, w, mode, stride, pad, flags, res, act1):
    n, h, w_in, c = x.shape
    co, k = w.shape[0], w.shape[1]
    ho, wo = abi.conv_out_size(mode, h, w_in, k, stride, pad)
    return abi.ConvParams(mode, k, stride, pad, n, h, w_in, c, ho, wo, co, act1, 0, abi.ALGO_AUTO, 0, flags,
                          _A, 2 * _A, None, None, 5 * _A if res is not None else None, 6 * _A, None, None)


def _conv(oracle, x, w, mode, stride, pad, res, act1, any_size, frame_h=None):
    """oracle.conv2d in version 2; frame_h: x is a slab of a map of frame_h rows and the launch computes in the version
    (and with the flags) the product's conv2d gives it (ops.slab_contract) -- set on the oracle's module under a lock,
    since the thread ranks share it"""
    flags = abi.CONV_WINO_ANY_SIZE if any_size else 0
    prec = abi.PREC_FP32_WINO
    if frame_h is not None:
        prec, flags = ops.slab_contract(_params(x, w, mode, stride, pad, flags, res, act1), frame_h)
    with _LOCK:
        old = oracle.PRECISION, oracle.WINO_ANY_SIZE
        oracle.PRECISION, oracle.WINO_ANY_SIZE = prec, bool(flags & abi.CONV_WINO_ANY_SIZE)
        try:
            return oracle.conv2d(x, w, None, mode=mode, stride=stride, pad=pad, res=res, act1=act1)
        finally:
            oracle.PRECISION, oracle.WINO_ANY_SIZE = old


def _weights(seed, specs):
    rng = np.random.default_rng(seed)
    return {n: (rng.standard_normal(s) * (1.0 / np.sqrt(np.prod(s[1:])))).astype(np.float32) for n, s in specs.items()}


# layers: (name, input map -- '*': all-gathered first, mode, ksize, stride, pad, residual map)
# (a) every Winograd form live, any size: down to an odd coarsest grid and back up
#   level 2 (x, 32 ch):  s = 1x1 32->128;  t = 3x3 s1 32->128 + s  (301);  d = 1x1 128->32
#   level 1:             e = 5x5 s2 32->128  (302)
#   level 0 (y grid):    f = 3x3 s2 128->128, all-gathered
#   level 1:             u = transposed 5x5 128->64 from the gathered map  (303);  v = 3x3 s1 64->128 on bands  (301)
#   level 2:             o = transposed 5x5 128->64 on bands  (303)
_CHAIN_A = [('s', 'x', abi.MODE_CONV, 1, 1, 0, None), ('t', 'x', abi.MODE_CONV, 3, 1, 1, 's'), ('d', 't', abi.MODE_CONV, 1, 1, 0, None),
            ('e', 'd', abi.MODE_CONV, 5, 2, 2, None), ('f', 'e', abi.MODE_CONV, 3, 2, 1, None), ('u', 'f*', abi.MODE_TCONV, 5, 2, 0, None),
            ('v', 'u', abi.MODE_CONV, 3, 1, 1, None), ('o', 'v', abi.MODE_TCONV, 5, 2, 0, None)]
_SPECS_A = dict(s=(128, 1, 1, 32), t=(128, 3, 3, 32), d=(32, 1, 1, 128), e=(128, 5, 5, 32), f=(128, 3, 3, 128), u=(64, 5, 5, 128),
                v=(128, 3, 3, 64), o=(64, 5, 5, 128))
# (b) a frame just above the 3x3 form's size rule (80 x 100 = AIVC_WINO_MIN_PIXELS): its slabs fall below it and only the
# routing by frame size keeps them on the Winograd chain; the 5x5 stride-2 layer's frame (40 x 50 outputs) is below the rule,
# so its slabs must stay on the tap chain
_CHAIN_B = [('s', 'x', abi.MODE_CONV, 1, 1, 0, None), ('t', 'x', abi.MODE_CONV, 3, 1, 1, 's'), ('d', 't', abi.MODE_CONV, 1, 1, 0, None),
            ('e', 'd', abi.MODE_CONV, 5, 2, 2, None)]
_SPECS_B = dict(s=(128, 1, 1, 32), t=(128, 3, 3, 32), d=(32, 1, 1, 128), e=(128, 5, 5, 32))


def _whole(oracle, chain, wts, x, any_size):
    m = {'x': x}
    for name, src, mode, k, stride, pad, res in chain:
        m[name] = _conv(oracle, m[src.rstrip('*')], wts[name], mode, stride, pad, None if res is None else m[res],
                        abi.ACT_LEAKY, any_size)
    return m


def _banded(oracle, ctx, chain, wts, x, h_y, k_x, any_size):
    """this rank's part -> {layer: (v0, v1, its valid rows)}"""
    ctx.set_frame(h_y, k_x)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    n = lambda t: None if t is None else np.ascontiguousarray(t.numpy())
    H = x.shape[1]
    o0, o1 = ctx.own(k_x, H)
    m = {'x': Band(ctx, T(x[:, o0:o1]), o0, H, k_x, o0, o1)}
    for name, src, mode, k, stride, pad, res in chain:
        xb = m[src.rstrip('*')]
        if src.endswith('*'):
            xb = ctx.full(ctx.gather_full(xb), xb.k)

        def launch(xs, rs, ms, w=wts[name], mode=mode, stride=stride, pad=pad, frame_h=xb.H):
            return T(_conv(oracle, n(xs), w, mode, stride, pad, n(rs), abi.ACT_LEAKY, any_size, frame_h))
        m[name] = ctx.conv(launch, xb, mode, k, stride, pad, wts[name].shape[0], res=None if res is None else m[res])
    return {name: (b.v0, b.v1, b.rows(b.v0, b.v1).numpy().copy()) for name, b in m.items() if name != 'x'}


def _run_ranks(R, fn):
    shared = ThreadComm.Shared(R)
    out, err = [None] * R, []

    def work(r):
        try:
            out[r] = fn(BandCtx(ThreadComm(shared, r), torch.device('cpu')))
        except BaseException as e:  # noqa: BLE001 -- a dead rank must not leave the others at the barrier
            err.append(e)
            shared.barrier.abort()
    ts = [threading.Thread(target=work, args=(r,)) for r in range(R)]
    [t.start() for t in ts]
    [t.join() for t in ts]
    if err:
        raise next((e for e in err if not isinstance(e, threading.BrokenBarrierError)), err[0])
    return out


def _check(oracle, chain, specs, x, h_y, k_x, R, any_size, seed):
    wts = _weights(seed, specs)
    want = _whole(oracle, chain, wts, x, any_size)
    res = _run_ranks(R, lambda ctx: _banded(oracle, ctx, chain, wts, x, h_y, k_x, any_size))
    for name, *_ in chain:
        H = want[name].shape[1]
        covered = 0
        for r, got in enumerate(res):
            v0, v1, rows = got[name]
            np.testing.assert_array_equal(rows, want[name][:, v0:v1], err_msg='layer %s, rank %d of %d' % (name, r, R))
            covered += v1 - v0
        assert covered == H, (name, covered, H)


def _variant(x_shape, w_shape, mode, stride, pad, flags=0, res=False):
    """aivc_conv2d_variant in version 2 for a launch of these shapes"""
    from aivc_amd import _lib
    n, h, w_in, c = x_shape
    ho, wo = abi.conv_out_size(mode, h, w_in, w_shape[1], stride, pad)
    p = abi.ConvParams(mode, w_shape[1], stride, pad, n, h, w_in, c, ho, wo, w_shape[0], abi.ACT_LEAKY, 0, abi.ALGO_AUTO, 0, flags,
                       _A, 2 * _A, None, None, 5 * _A if res else None, 6 * _A, None, None)
    p.precision = abi.PREC_FP32_WINO
    return _lib.load()['aivc_conv2d_variant'](ctypes.byref(p))


@pytest.mark.parametrize('R', [2, 3, 4, 5])
def test_winograd_chain_any_size_bands_equal_whole_map(R, oracle):
    """(a): 3x3 stride 1 with a residual, 5x5 stride 2, transposed 5x5 from a gathered map and from bands, an odd coarsest
    grid -- all in version 2 (AIVC_CONV_WINO_ANY_SIZE): every slab starts on the frame's tile grid"""
    h_y, W = 7, 12
    H = 4 * h_y - 1
    x = np.random.default_rng(R).standard_normal((1, H, W, 32)).astype(np.float32)
    # every Winograd form is live in this chain
    assert _variant((1, H, W, 32), _SPECS_A['t'], abi.MODE_CONV, 1, 1, abi.CONV_WINO_ANY_SIZE, True) == 301
    assert _variant((1, H, W, 32), _SPECS_A['e'], abi.MODE_CONV, 2, 2, abi.CONV_WINO_ANY_SIZE) == 302
    assert _variant((1, 7, W // 4, 128), _SPECS_A['u'], abi.MODE_TCONV, 2, 0, abi.CONV_WINO_ANY_SIZE) == 303
    _check(oracle, _CHAIN_A, _SPECS_A, x, h_y, 2, R, True, seed=10 + R)


@pytest.mark.parametrize('R', [2, 3, 5])
def test_winograd_chain_routed_by_frame_size(R, oracle):
    """(b): 80 x 100 frame, no any-size flag -- the frame's 3x3 launches take the Winograd chain, a slab's own size would not"""
    H, W = 80, 100
    assert H * W == abi.WINO_MIN_PIXELS
    assert _variant((1, H, W, 32), _SPECS_B['t'], abi.MODE_CONV, 1, 1, 0, True) == 301
    assert _variant((1, H // R + 2, W, 32), _SPECS_B['t'], abi.MODE_CONV, 1, 1, 0, True) != 301  # a slab alone: tap chain
    assert _variant((1, H, W, 32), _SPECS_B['e'], abi.MODE_CONV, 2, 2) != 302  # 40 x 50 outputs: below the rule
    x = np.random.default_rng(100 + R).standard_normal((1, H, W, 32)).astype(np.float32)
    _check(oracle, _CHAIN_B, _SPECS_B, x, H // 2, 1, R, False, seed=20 + R)


def test_slab_contract_follows_the_frame():
    """ops.slab_contract: the whole map's routing decides, on the slab's own params"""
    def p_of(h, ci, co, k, stride, pad, mode=abi.MODE_CONV, flags=0):
        ho, wo = abi.conv_out_size(mode, h, 100, k, stride, pad)
        return abi.ConvParams(mode, k, stride, pad, 1, h, 100, ci, ho, wo, co, 0, 0, abi.ALGO_AUTO, 0, flags,
                              _A, 2 * _A, 3 * _A, None, None, 6 * _A, None, None)
    assert ops.slab_contract(p_of(12, 32, 128, 3, 1, 1), 80) == (abi.PREC_FP32_WINO, abi.CONV_WINO_ANY_SIZE)  # frame covered
    assert ops.slab_contract(p_of(12, 32, 128, 3, 1, 1), 40) == (abi.PREC_FP32, 0)  # frame below the rule: version 1
    assert ops.slab_contract(p_of(12, 32, 64, 3, 1, 1), 800) == (abi.PREC_FP32, 0)  # a shape version 2 does not cover
    assert ops.slab_contract(p_of(12, 32, 128, 5, 2, 2), 400) == (abi.PREC_FP32_WINO, abi.CONV_WINO_ANY_SIZE)  # 200 x 50 outputs
    assert ops.slab_contract(p_of(12, 128, 64, 5, 2, 0, abi.MODE_TCONV), 400) == (abi.PREC_FP32_WINO, abi.CONV_WINO_ANY_SIZE)
    assert ops.slab_contract(p_of(12, 128, 64, 5, 2, 0, abi.MODE_TCONV), 300) == (abi.PREC_FP32, 0)  # 30000 input pixels
    assert ops.slab_contract(p_of(12, 32, 128, 3, 1, 1, flags=abi.CONV_SPARSE4), 40) == (abi.PREC_FP32, abi.CONV_SPARSE4)
    # a covered frame with a fused gdn has no code (the map's launch splits): the slab's must split too
    p = p_of(12, 32, 128, 3, 1, 1)
    p.gdn, p.gdn_beta, p.gdn_gamma = 1, 7 * _A, 8 * _A
    assert ops.slab_contract(p, 80) == (abi.PREC_FP32_WINO, abi.CONV_WINO_ANY_SIZE)
    p.precision, p.flags = ops.slab_contract(p, 80)
    from aivc_amd import _lib
    assert _lib.load()['aivc_conv2d_variant'](ctypes.byref(p)) < 0
