"""The conv family's part of tests/op_cases.py (read its docstring first): the case tables of tests/test_gpu_ops.py,
test_gpu_winograd*.py (with their shared fixture and helpers), test_gpu_gdn_resident.py, test_gpu_large_batches.py and tests/test_gpu_memory_discipline.py and one builder
per kind of launch; the fp64 layer evaluation with torch that several modules compare against.  Every
builder's call passes keyword arguments on to ops.conv2d / ops.gdn (algo=...).  Not a test module."""
import numpy as np
import pytest

from aivc_amd import abi
from numeric_regimes import assert_bits, row_facts
from op_cases import Case, on, profiled

CONV_CASES = [
    # mode, k, stride, pad, cin, cout, h, w, act1, act2, mul, res
    (abi.MODE_CONV, 5, 2, 2, 4, 8, 17, 23, 0, 0, False, False),
    (abi.MODE_CONV, 3, 1, 1, 8, 8, 9, 11, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_CONV, 3, 2, 1, 12, 16, 10, 14, abi.ACT_RELU, 0, False, False),
    (abi.MODE_CONV, 1, 2, 0, 8, 8, 9, 13, 0, 0, False, False),
    (abi.MODE_CONV, 1, 1, 0, 8, 8, 6, 10, abi.ACT_SIGMOID, 0, True, True),
    (abi.MODE_CONV, 3, 1, 1, 8, 8, 7, 9, 0, abi.ACT_RELU, False, True),
    (abi.MODE_TCONV, 5, 2, 0, 8, 6, 7, 9, 0, 0, False, False),
    (abi.MODE_TCONV, 3, 2, 0, 8, 8, 5, 6, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_TCONV, 5, 2, 0, 64, 3, 6, 5, 0, 0, False, False),
    (abi.MODE_GDN, 1, 1, 0, 8, 8, 5, 7, 0, 0, False, False),
    (abi.MODE_IGDN, 1, 1, 0, 16, 16, 5, 7, 0, 0, False, True),
    (abi.MODE_CONV, 5, 2, 2, 64, 128, 33, 47, 0, 0, False, False),
    (abi.MODE_CONV, 3, 1, 1, 128, 128, 19, 21, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_CONV, 3, 2, 1, 128, 128, 40, 44, abi.ACT_LEAKY, 0, False, False),
    (abi.MODE_CONV, 5, 2, 2, 12, 64, 47, 61, 0, 0, False, False),
    (abi.MODE_CONV, 5, 2, 2, 128, 64, 30, 34, 0, 0, False, False),
    (abi.MODE_CONV, 1, 1, 0, 128, 64, 23, 29, abi.ACT_LEAKY, 0, False, False),
    (abi.MODE_CONV, 1, 2, 0, 128, 128, 31, 29, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 128, 128, 17, 19, 0, 0, False, False),
    (abi.MODE_TCONV, 3, 2, 0, 128, 128, 17, 19, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_TCONV, 5, 2, 0, 128, 64, 33, 35, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 32, 128, 9, 11, abi.ACT_LEAKY, 0, False, False),
    (abi.MODE_GDN, 1, 1, 0, 128, 128, 33, 31, 0, 0, False, False),
    (abi.MODE_IGDN, 1, 1, 0, 64, 64, 33, 31, 0, 0, False, True),
    (abi.MODE_CONV, 3, 1, 1, 128, 192, 9, 11, 0, 0, False, False),
    (abi.MODE_CONV, 3, 1, 1, 64, 256, 20, 20, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 64, 6, 37, 41, 0, 0, False, False),
    (abi.MODE_TCONV, 3, 2, 0, 64, 3, 17, 33, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_TCONV, 5, 2, 0, 128, 3, 9, 19, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 16, 6, 16, 16, 0, abi.ACT_RELU, False, True),
    # thin outputs on the 16x16x4 MFMA kernel: partial tiles in x and y, several tiles, gate + residual
    (abi.MODE_TCONV, 5, 2, 0, 64, 3, 19, 70, abi.ACT_LEAKY, 0, True, False),
    (abi.MODE_TCONV, 3, 2, 0, 32, 6, 9, 40, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 48, 6, 8, 33, 0, abi.ACT_LEAKY, True, True),
    (abi.MODE_TCONV, 3, 2, 0, 96, 3, 1, 1, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 64, 6, 6, 10, abi.ACT_SIGMOID, 0, False, False),  # falls back to the VALU kernel
    (abi.MODE_TCONV, 5, 2, 0, 64, 3, 7, 70, abi.ACT_RELU, 0, False, False),     # lean epilogue, relu (+0.0 for negatives)
    (abi.MODE_TCONV, 5, 2, 0, 32, 6, 5, 33, abi.ACT_LEAKY, 0, False, False),
    # LDS-DMA K loop corner cases: a reduction of ONE K-tile (1x1, c_in 32), of an odd number (3x3 x 32 = 9), two
    # tiles; transposed with image-border zero fill on every tile; c_out beyond the tile width; rows beyond M
    (abi.MODE_CONV, 1, 1, 0, 32, 64, 9, 13, 0, 0, False, False),
    (abi.MODE_CONV, 3, 1, 1, 32, 32, 11, 7, abi.ACT_LEAKY, 0, False, True),
    (abi.MODE_CONV, 1, 2, 0, 64, 128, 5, 3, 0, abi.ACT_RELU, False, True),
    (abi.MODE_TCONV, 3, 2, 0, 32, 64, 7, 9, 0, 0, False, False),
    (abi.MODE_TCONV, 5, 2, 0, 64, 128, 1, 3, abi.ACT_LEAKY, 0, False, False),
    (abi.MODE_CONV, 5, 2, 2, 96, 160, 13, 9, 0, 0, False, False),
    # a 13th entry states the bias: sigmoid pre-activations (bias + a conv output of unit scale) on both sides of -103.97 / -88.72 /
    # -87.34 and of their mirror images, where fp32 exp(-v) underflows, overflows or is subnormal and the quotient 1 / (1 + e) is
    # subnormal or 0, instead of within +-5 (tests/test_gpu_detmath.py says why); conv_case asserts that they are reached
    (abi.MODE_CONV, 1, 1, 0, 8, 8, 6, 10, abi.ACT_SIGMOID, 0, True, True, (-110.0, -104.0, -88.0, -40.0, 40.0, 88.0, 104.0, 110.0)),
]

# The register-staged K loop's own users, on every tile each is instantiated for (AIVC_FORCE_TILE ids; 2 = 256x64 exists for
# c_in % 32 == 0 only): the (I)GDN mode with and without whole K tiles, transposed conv with c_in % 32 != 0.  Two images of
# 9 x 13: M = 234 rows, a partial last tile for every BM.
STAGED_CASES = [
    # row as in CONV_CASES, tiles
    ((abi.MODE_GDN, 1, 1, 0, 64, 64, 9, 13, 0, 0, False, False), (0, 1, 2, 3, 5, 6)),
    ((abi.MODE_IGDN, 1, 1, 0, 64, 64, 9, 13, 0, 0, False, True), (0, 1, 2, 3, 5, 6)),
    ((abi.MODE_GDN, 1, 1, 0, 36, 36, 9, 13, 0, 0, False, True), (0, 1, 3, 5, 6)),
    ((abi.MODE_IGDN, 1, 1, 0, 36, 36, 9, 13, 0, 0, False, False), (0, 1, 3, 5, 6)),
    ((abi.MODE_TCONV, 3, 2, 0, 8, 64, 9, 13, abi.ACT_LEAKY, 0, False, True), (0, 1, 3, 5, 6)),
    ((abi.MODE_TCONV, 5, 2, 0, 8, 64, 9, 13, 0, 0, False, False), (0, 1, 3, 5, 6)),
    ((abi.MODE_TCONV, 3, 2, 0, 12, 128, 9, 13, 0, 0, False, False), (0, 1, 3, 5, 6)),
    ((abi.MODE_TCONV, 5, 2, 0, 12, 128, 9, 13, 0, abi.ACT_RELU, False, True), (0, 1, 3, 5, 6)),
]
# ... and with a fused (I)GDN (rows as in FUSED_GDN_CASES): the tiles whose BN is c_out
STAGED_FUSED_GDN_CASES = [
    ((abi.MODE_TCONV, 5, 2, 0, 8, 64, 9, 13, True, False), (1, 6)),
    ((abi.MODE_TCONV, 3, 2, 0, 12, 128, 9, 13, False, True), (0, 5)),
]

THIN_WALK_GRIDS = [1, 3, 7]
THIN_WALK_CASES = [(3, 5, 64, 21, 100), (6, 5, 64, 9, 70), (3, 3, 16, 13, 65)]  # co, k, ci, h, w

FUSED_GDN_CASES = [
    # mode, k, stride, pad, cin, cout, h, w, inverse, res
    (abi.MODE_CONV, 5, 2, 2, 12, 64, 31, 45, False, False),
    (abi.MODE_CONV, 5, 2, 2, 64, 128, 33, 29, False, False),
    (abi.MODE_CONV, 3, 1, 1, 128, 128, 17, 19, False, True),
    (abi.MODE_CONV, 3, 1, 1, 128, 128, 17, 19, True, True),
    (abi.MODE_TCONV, 5, 2, 0, 128, 128, 9, 11, True, False),
    (abi.MODE_TCONV, 5, 2, 0, 128, 64, 23, 21, True, False),
    (abi.MODE_CONV, 3, 1, 1, 32, 32, 9, 9, False, False),
    (abi.MODE_CONV, 3, 1, 1, 8, 8, 9, 9, False, True),      # not fusable: two launches
]

FUSED_TAIL_CASES = [
    # k, stride, cin, c_mid, c_tail, n, h, w, act1, act2, res
    (3, 1, 64, 64, 128, 2, 16, 32, abi.ACT_LEAKY, abi.ACT_LEAKY, True),   # whole 128-pixel tiles (the bottleneck block)
    (3, 1, 64, 64, 128, 2, 17, 19, abi.ACT_LEAKY, abi.ACT_LEAKY, True),   # ragged last tile
    (3, 1, 64, 64, 128, 1, 9, 5, abi.ACT_RELU, abi.ACT_NONE, True),       # a single partial tile
    (3, 1, 64, 64, 128, 2, 13, 21, abi.ACT_NONE, abi.ACT_RELU, False),
    (5, 2, 32, 64, 128, 2, 31, 27, abi.ACT_LEAKY, abi.ACT_NONE, False),
    (1, 1, 128, 64, 128, 3, 11, 23, abi.ACT_RELU, abi.ACT_LEAKY, True),
    (3, 1, 64, 64, 64, 2, 9, 9, abi.ACT_LEAKY, abi.ACT_LEAKY, True),      # not fusable (tail width): two launches
    (3, 1, 8, 12, 24, 2, 9, 9, abi.ACT_LEAKY, abi.ACT_LEAKY, True),       # not fusable (narrow): two launches
    (3, 1, 12, 6, 12, 1, 7, 9, abi.ACT_LEAKY, abi.ACT_LEAKY, True),       # intermediate width not a multiple of 4
    # an attention block 128 wide (bench.py --widths n=256) at 96 x 96 >= AIVC_WINO_MIN_PIXELS, size rule in force: under fp32w the
    # 3x3 is covered, the library declines the fused request, the two launches take 301 then the 1x1
    (3, 1, 128, 128, 256, 1, 96, 96, abi.ACT_LEAKY, abi.ACT_LEAKY, True),
]

CONV_IMAGES_CASES = [(9, 13, 2), (16, 128, 1), (35, 131, 2), (64, 64, 3)]  # h, w, n

GDN_RESIDENT_CASES = [
    # c, n, h, w, inverse, res
    (128, 1, 8, 8, False, False),      # one whole tile
    (128, 1, 5, 7, False, False),      # one partial tile (35 of 64 rows)
    (128, 2, 33, 31, False, True),     # 2046 pixels: 31 whole tiles + 62 rows
    (128, 2, 33, 31, True, False),
    (128, 1, 9, 13, True, True),
    (64, 1, 33, 31, False, False),
    (64, 2, 17, 19, True, True),
    (64, 1, 3, 5, False, True),
    (128, 3, 136, 120, False, False),  # 765 tiles: more than the 512 persistent workgroups of a 256-CU part
    (128, 3, 136, 120, True, True),
]

# the attention gate x + trunk * sigmoid(conv1x1(a)): whole 64-row tiles take the inlined-sigmoid epilogue, ragged ones the general
# one; the last row scales the conv's weights (pre-activations far beyond +-5: see the last row of CONV_CASES)
ATTENTION_GATE_CASES = [(2, 16, 32, 128, 1.0), (1, 9, 11, 128, 1.0), (2, 8, 8, 64, 1.0), (1, 9, 11, 128, 40.0)]  # n, h, w, c, weight scale


def _dressed(dress, rng, inputs, row):
    """the drawn inputs, or what the regime `dress` (tests/numeric_regimes.py) makes of them"""
    return inputs if dress is None else dress(rng, inputs, row)


def _reached(dress, row, inputs, want, chain):
    """{} or, having asserted that the oracle's result proves the regime reached, the facts a dressed case carries"""
    if dress is None:
        return {}
    with np.errstate(all='ignore'):
        dress.reach(row, inputs, want, chain)
    return {'regime': dress, 'row': row}


def attention_gate_case(oracle, n, h, w, c, scale, dress=None):
    rng = np.random.default_rng(n * 100 + h)
    a = rng.standard_normal((n, h, w, c), dtype=np.float32)
    wt = (rng.standard_normal((c, 1, 1, c), dtype=np.float32) / np.sqrt(c)).astype(np.float32) * np.float32(scale)
    b = rng.standard_normal(c, dtype=np.float32)
    trunk = rng.standard_normal((n, h, w, c), dtype=np.float32)
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    row = row_facts(act1=abi.ACT_SIGMOID)
    i = _dressed(dress, rng, {'x': a, 'w': wt, 'bias': b, 'mul': trunk, 'res': x}, row)
    pre = oracle.conv2d(i['x'], i['w'], i['bias'])
    want = oracle.conv2d(i['x'], i['w'], i['bias'], act1=abi.ACT_SIGMOID, mul=i['mul'], res=i['res'])
    return Case(i, _conv_call(('mul', 'res'), act1=abi.ACT_SIGMOID), want, pre_activation=pre,
                **_reached(dress, row, i, want, lambda: pre))


WINO_CASES = [  # n, h, w, c_in, c_out, act1, act2, bias, mul, res
    (1, 8, 8, 32, 128, 0, 0, True, False, False),
    (2, 7, 9, 32, 128, 1, 0, True, False, False),      # odd sizes: half-filled last tile row / column
    (3, 13, 21, 64, 128, 0, 2, True, False, True),     # residual + relu
    (1, 17, 30, 128, 128, 1, 0, True, False, True),    # leaky then residual (ChengResBlock)
    (5, 5, 3, 128, 128, 0, 1, False, True, True),      # no bias, gate multiplicand, tiny images: a tile spans images
    (1, 1, 1, 32, 128, 0, 0, True, False, False),      # a single pixel
    (2, 34, 60, 128, 128, 0, 0, True, False, False),
    (1, 9, 40, 64, 256, 2, 0, True, False, False),     # c_out 256: four 64-channel blocks
    (1, 68, 120, 128, 128, 0, 0, True, False, True),   # the 1/16-resolution shape of 1080p
    (2, 33, 50, 64, 128, 1, 0, True, False, True),     # interior blocks (lean epilogue) + right-edge / bottom-edge blocks
    (1, 47, 64, 32, 128, 0, 1, True, False, False),    # leaky after the (absent) residual
    (1, 32, 48, 32, 256, 2, 0, False, False, False),   # relu, no bias
]

# the 5x5 stride-2 layers in polyphase form (ABI 17: four stride-1 3x3 convolutions of the input's phases, 49 multiplications per
# 2x2 outputs instead of 100; include/aivc_hip.h, aivc_winograd_covers)
POLY_CASES = [  # n, h, w, c_in, c_out, act1, act2, bias, res
    (1, 8, 8, 32, 128, 0, 0, True, False),
    (2, 15, 17, 64, 128, 1, 0, True, False),     # odd input sizes: the last phase row / column clamps into the other phase's samples
    (1, 33, 47, 64, 128, 0, 2, True, True),
    (1, 64, 96, 64, 128, 0, 0, True, False),     # 32 x 48 outputs: 2 x 3 blocks
    (3, 9, 7, 32, 256, 2, 0, False, False),      # four 64-channel blocks, tiny images
    (1, 136, 240, 64, 128, 0, 0, True, True),    # 68 x 120 outputs: right-edge column, bottom block row mostly outside
    (1, 7, 5, 128, 128, 0, 1, True, True),
    (1, 1, 1, 32, 128, 0, 0, True, False),       # a single pixel: every tap clamps onto it
    (2, 34, 62, 64, 128, 1, 0, True, True),
]

# the transposed 5x5 stride-2 layers class by class (ABI 17: each output parity class a stride-1 3x3 correlation of the
# zero-extended input, 49 multiplications per 2x2 grid pixels instead of 100)
TC_CASES = [  # n, h, w, c_in, c_out, act1, act2, bias, res
    (1, 8, 8, 32, 64, 0, 0, True, False),
    (2, 7, 9, 64, 64, 1, 0, True, False),        # odd sizes: half-filled last tile row / column, zero extension on every side
    (1, 17, 30, 128, 64, 0, 0, True, True),
    (1, 33, 50, 128, 128, 0, 2, True, True),     # c_out 128: two channel blocks per class; interior + edge blocks
    (3, 5, 3, 32, 128, 0, 0, False, False),      # tiny images: a block spans nothing but border
    (1, 68, 120, 128, 64, 0, 0, True, False),    # the 1/16-resolution shape of 1080p: right-edge column
    (1, 1, 1, 32, 64, 0, 0, True, False),
    (2, 34, 60, 64, 128, 2, 0, True, True),
]

WINO_FORMS = {301: (3, 1, 1, abi.MODE_CONV), 302: (5, 2, 2, abi.MODE_CONV), 303: (5, 2, 0, abi.MODE_TCONV)}  # variant: k, stride, pad, mode

BF16X3_CASES = [  # mode, k, stride, pad, c_in, c_out, h, w, fused gdn (0 / 1 / 2), variant with the weights split ahead, in the K loop
    (abi.MODE_CONV, 3, 1, 1, 64, 128, 9, 11, 0, 1100, 1100),
    (abi.MODE_CONV, 5, 2, 2, 128, 64, 13, 15, 0, 1106, 1102),
    (abi.MODE_TCONV, 5, 2, 0, 128, 128, 5, 7, 2, 1165, 1160),
]


def _conv_call(names, **fixed):
    """ops.conv2d(x, w, bias, ...) from the placed inputs: those in `names` as the keyword arguments of their name"""
    def call(ops, d, **kw):
        return ops.conv2d(d['x'], d['w'], d['bias'], **fixed, **{nm: d[nm] for nm in names}, **kw)
    return call


def conv_case(oracle, row, seed, n=2, dress=None):
    """a row of CONV_CASES: bias, two activations, gate multiplicand, residual; the GDN modes with positive gamma and beta"""
    mode, k, s, pad, ci, co, h, w, a1, a2, use_mul, use_res = row[:12]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    if len(row) > 12:
        bias = np.array(row[12], np.float32)
        assert bias.shape == (co,)
    if mode in (abi.MODE_GDN, abi.MODE_IGDN):
        wt = np.abs(wt) * 0.1
        bias = np.abs(bias) + 0.1
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    mul = rng.standard_normal((n, ho, wo, co), dtype=np.float32) if use_mul else None
    res = rng.standard_normal((n, ho, wo, co), dtype=np.float32) if use_res else None
    fixed = dict(mode=mode, stride=s, pad=pad, act1=a1, act2=a2)
    facts = {}
    rf = row_facts(mode, k, s, pad, a1, a2)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': bias, 'mul': mul, 'res': res}, rf)
    x, wt, bias, mul, res = (i[nm] for nm in ('x', 'w', 'bias', 'mul', 'res'))
    if len(row) > 12 and dress is None:  # the range the row exists for, whatever the seed
        pre = facts['pre_activation'] = oracle.conv2d(x, wt, bias, mode=mode, stride=s, pad=pad)
        for lo, hi in ((-np.inf, -103.98), (-103.97, -88.73), (-88.72, -87.34), (87.34, 88.72), (88.73, 103.97), (103.98, np.inf)):
            assert ((pre > lo) & (pre < hi)).any(), (lo, hi, float(pre.min()), float(pre.max()))
    with np.errstate(all='ignore'):
        want = oracle.conv2d(x, wt, bias, mul=mul, res=res, **fixed)

    def chain(inverse=False):  # (inverse: the GDN mode's normaliser through its inverse form)
        return oracle.conv2d(x, wt, bias, mode=abi.MODE_IGDN if inverse else mode, stride=s, pad=pad)
    return Case(i, _conv_call(('mul', 'res'), **fixed), want, **facts, **_reached(dress, rf, i, want, chain))


def thin_walk_case(oracle, row, seed, with_bias=True, dress=None):
    """a row of THIN_WALK_CASES over 3 images: the transposed thin output layer, leaky, with or without its bias (drawn either way)"""
    co, k, ci, h, w = row
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    if not with_bias:
        bias = None
    fixed = dict(mode=abi.MODE_TCONV, stride=2, pad=0, act1=abi.ACT_LEAKY)
    rf = row_facts(abi.MODE_TCONV, k, 2, 0, abi.ACT_LEAKY)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': bias}, rf)
    with np.errstate(all='ignore'):
        want = oracle.conv2d(i['x'], i['w'], i['bias'], **fixed)
    return Case(i, _conv_call((), **fixed), want,
                **_reached(dress, rf, i, want, lambda: oracle.conv2d(i['x'], i['w'], i['bias'], mode=abi.MODE_TCONV, stride=2)))


def _gdn_params(rng, co, floor=0.2, scale=0.05):
    return (np.abs(rng.standard_normal(co)) + floor).astype(np.float32), (np.abs(rng.standard_normal((co, co))) * scale).astype(np.float32)


def fused_gdn_case(oracle, row, seed, dress=None):
    """a row of FUSED_GDN_CASES: conv + (I)GDN (+ residual) in one request; want: the oracle's fused evaluation"""
    mode, k, s, pad, ci, co, h, w, inv, use_res = row
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    bias = rng.standard_normal(co, dtype=np.float32)
    beta, gamma = _gdn_params(rng, co)
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    res = rng.standard_normal((2, ho, wo, co), dtype=np.float32) if use_res else None
    fixed = dict(mode=mode, stride=s, pad=pad)
    rf = row_facts(mode, k, s, pad, fused_gdn=inv)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': bias, 'beta': beta, 'gamma': gamma, 'res': res}, rf)
    with np.errstate(all='ignore'):
        want = oracle.conv2d(i['x'], i['w'], i['bias'], res=i['res'], gdn=(beta, gamma, inv), **fixed)
    return Case(i, lambda ops, d, **kw: ops.conv2d(d['x'], d['w'], d['bias'], res=d['res'], gdn=(d['beta'], d['gamma'], inv), **fixed, **kw),
                want, **_reached(dress, rf, i, want, lambda: oracle.conv2d(i['x'], i['w'], i['bias'], gdn=(beta, gamma, inv), **fixed)))


def fused_tail_case(oracle, row, seed, dress=None):
    """a row of FUSED_TAIL_CASES: conv + activation + 1x1 conv (+ residual, activation) in one request; want: the oracle's two
    convolutions, the intermediate zero padded to a multiple of 4 channels as the tail's weights are.  covered: version 2 of the
    contract runs the 3x3 on the Winograd chain (size rule in force) and the library declines the fusion."""
    k, s, ci, cm, ct, n, h, w, a1, a2, use_res = row
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((cm, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    b1 = rng.standard_normal(cm, dtype=np.float32)
    cm4 = (cm + 3) // 4 * 4
    w3 = np.zeros((ct, 1, 1, cm4), dtype=np.float32)
    w3[..., :cm] = rng.standard_normal((ct, 1, 1, cm), dtype=np.float32) / np.sqrt(cm)
    b3 = rng.standard_normal(ct, dtype=np.float32)
    ho, wo = abi.conv_out_size(abi.MODE_CONV, h, w, k, s, k // 2)
    res = rng.standard_normal((n, ho, wo, ct), dtype=np.float32) if use_res else None
    rf = row_facts(abi.MODE_CONV, k, s, k // 2, a1, a2, tail=True)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': b1, 'w3': w3, 'b3': b3, 'res': res}, rf)
    with np.errstate(all='ignore'):
        t = oracle.conv2d(i['x'], i['w'], i['bias'], stride=s, pad=k // 2, act1=a1)
    if cm4 != cm:
        t = np.concatenate([t, np.zeros(t.shape[:3] + (cm4 - cm,), np.float32)], axis=-1)
    fixed = dict(stride=s, pad=k // 2, act1=a1, act2=a2)
    with np.errstate(all='ignore'):
        want = oracle.conv2d(t, i['w3'], i['b3'], res=i['res'], act2=a2)
    return Case(i, lambda ops, d, **kw: ops.conv2d(d['x'], d['w'], d['bias'], res=d['res'], tail=(d['w3'], d['b3']), **fixed, **kw),
                want, fixed=fixed, covered=k == 3 and s == 1 and ci % 32 == 0 and cm % 128 == 0 and h * w >= 8000,
                **_reached(dress, rf, i, want, lambda: oracle.conv2d(t, i['w3'], i['b3'])))


def gdn_resident_case(oracle, row, with_oracle=True, dress=None):
    """a row of GDN_RESIDENT_CASES: the stand-alone (I)GDN; want is None where the test leaves the CPU oracle out (large sizes)"""
    c, n, h, w, inv, use_res = row
    rng = np.random.default_rng(c * 1000 + n * 100 + h + w + (5 if inv else 0))
    x = rng.standard_normal((n, h, w, c), dtype=np.float32)
    beta, gamma = _gdn_params(rng, c)
    res = rng.standard_normal((n, h, w, c), dtype=np.float32) if use_res else None
    rf = row_facts(abi.MODE_IGDN if inv else abi.MODE_GDN)
    i = _dressed(dress, rng, {'x': x, 'beta': beta, 'gamma': gamma, 'res': res}, rf)
    with np.errstate(all='ignore'):
        want = oracle.gdn(i['x'], beta, gamma, inverse=inv, res=i['res']) if with_oracle else None
    return Case(i, lambda ops, d, **kw: ops.gdn(d['x'], d['beta'], d['gamma'], inverse=inv, res=d['res'], **kw), want,
                **_reached(dress, rf, i, want, lambda inverse=False: oracle.gdn(i['x'], beta, gamma, inverse=inv or inverse)))


def wino_case(oracle, variant, row, seed, dress=None):
    """a row of WINO_CASES (variant 301), POLY_CASES (302) or TC_CASES (303, weights scaled for its 4 classes); the 5x5 tables have
    no gate multiplicand.  Needs version 2 of the contract with the size rule lifted on both sides (the tests' fixture)."""
    n, h, w, ci, co, a1, a2, has_b, has_m, has_r = row if len(row) == 10 else row[:8] + (False, row[8])
    k, s, pad, mode = WINO_FORMS[variant]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, h, w, ci)).astype(np.float32)
    wt = (rng.standard_normal((co, k, k, ci)) / np.sqrt(k * k * ci / (4 if mode == abi.MODE_TCONV else 1))).astype(np.float32)
    b = (rng.standard_normal(co) * 0.1).astype(np.float32) if has_b else None
    ho, wo = abi.conv_out_size(mode, h, w, k, s, pad)
    m = rng.standard_normal((n, ho, wo, co)).astype(np.float32) if has_m else None
    r = rng.standard_normal((n, ho, wo, co)).astype(np.float32) if has_r else None
    fixed = dict(mode=mode, stride=s, pad=pad, act1=a1, act2=a2)
    rf = row_facts(mode, k, s, pad, a1, a2, variant=variant)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': b, 'mul': m, 'res': r}, rf)
    with np.errstate(all='ignore'):
        want = oracle.conv2d(i['x'], i['w'], i['bias'], mul=i['mul'], res=i['res'], **fixed)
    return Case(i, _conv_call(('mul', 'res'), **fixed), want,
                **_reached(dress, rf, i, want, lambda: oracle.conv2d(i['x'], i['w'], i['bias'], mode=mode, stride=s, pad=pad)))


@pytest.fixture()
def fp32w(oracle):
    """version 2 of the contract with the size rule lifted, on the device side and in the oracle (a test module imports it)"""
    from aivc_amd import ops
    prev_h, prev_o = ops.set_precision('fp32w'), oracle.set_precision('fp32w')
    ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = True  # the kernel on shapes the oracle checks in seconds
    yield
    ops.WINO_ANY_SIZE = oracle.WINO_ANY_SIZE = False
    ops.set_precision(prev_h)
    oracle.set_precision(prev_o)


def wino_blocks(variant, row, n=None):
    """length of the kernel's block list (conv2d_wino) for n images (default: the row's): 16 x 16 grid pixels x 64 output channels
    (x 4 classes, transposed form).  The grid is the output's; transposed form: the input's"""
    h, w, co = row[1], row[2], row[4]
    gh, gw = ((h + 1) // 2, (w + 1) // 2) if variant == 302 else (h, w)
    return (row[0] if n is None else n) * ((gh + 15) // 16) * ((gw + 15) // 16) * (co // 64) * (4 if variant == 303 else 1)


def wino_three_launches(variant, c, cuda):
    """three launches in a row on the same buffers: the variant code and the oracle's bits, every time"""
    from aivc_amd import ops
    d = c.place(on(cuda))
    for launch in range(3):
        got, variants = profiled(lambda: c.call(ops, d))
        assert variants == [variant], (launch, variants)
        assert_bits(got.cpu().numpy(), c.want, 'launch %d' % launch)


def wino_weights_case(oracle, form, c_in):
    """the U image of a [64, k, k, c_in] weight in the form '3x3', 'poly5' or 'tconv5', flat"""
    k = 3 if form == '3x3' else 5
    wt = (np.random.default_rng(100 + c_in + k).standard_normal((64, k, k, c_in)) * 3).astype(np.float32)
    tr = form == 'tconv5'
    want = np.asarray(oracle.winograd_weights(wt, transposed=tr)).ravel()
    assert want.size == 64 * 16 * c_in * (1 if form == '3x3' else 4)
    return Case({'w': wt}, lambda ops, d: ops.winograd_weights(d['w'], transposed=tr), want)


def bf16x3_case(row, seed):
    """a row of BF16X3_CASES.  The precision mode has no oracle (its bits are its own): want is for the test to set, from a run
    of the same launch that it trusts"""
    mode, k, s, pad, ci, co, h, w, gdn = row[:9]
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, h, w, ci), dtype=np.float32)
    wt = (rng.standard_normal((co, k, k, ci), dtype=np.float32) / np.sqrt(k * k * ci)).astype(np.float32)
    b = rng.standard_normal(co, dtype=np.float32)
    beta, gamma = _gdn_params(rng, co, 0.5, 0.02)

    def call(ops, d):
        g = (d['beta'], d['gamma'], gdn == 2) if gdn else None
        return ops.conv2d(d['x'], d['w'], d['bias'], mode=mode, stride=s, pad=pad, gdn=g)
    return Case({'x': x, 'w': wt, 'bias': b, 'beta': beta, 'gamma': gamma}, call, None)


def mfma_tile_case(oracle, seed, c_in, dress=None):
    """M = 2 * 9 * 13 = 234 rows and 72 output channels (multiples of no tile side): partial tiles along both; 3x3, leaky, residual"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((2, 9, 13, c_in), dtype=np.float32)
    wt = (rng.standard_normal((72, 3, 3, c_in), dtype=np.float32) / np.sqrt(9 * c_in)).astype(np.float32)
    b = rng.standard_normal(72, dtype=np.float32)
    res = rng.standard_normal((2, 9, 13, 72), dtype=np.float32)
    fixed = dict(stride=1, pad=1, act1=abi.ACT_LEAKY)
    rf = row_facts(abi.MODE_CONV, 3, 1, 1, abi.ACT_LEAKY)
    i = _dressed(dress, rng, {'x': x, 'w': wt, 'bias': b, 'res': res}, rf)
    with np.errstate(all='ignore'):
        want = oracle.conv2d(i['x'], i['w'], i['bias'], res=i['res'], **fixed)
    return Case(i, _conv_call(('res',), **fixed), want,
                **_reached(dress, rf, i, want, lambda: oracle.conv2d(i['x'], i['w'], i['bias'], stride=1, pad=1)))


# ---- conv_images and pack_images -------------------------------------------------------------------------------------------------
def _image_sources(rng, n, h, w, zero_pad, with_f3):
    """'a', 'b': 8-bit 4:2:0 planes; 'f': a float source of 4 channels (the pad channel zero or not); 'f3': one of 3, drawn last"""
    hc, wc = (h + 1) // 2, (w + 1) // 2

    def planes():
        return {'y': rng.integers(0, 256, (n, h, w), dtype=np.uint8), 'u': rng.integers(0, 256, (n, hc, wc), dtype=np.uint8),
                'v': rng.integers(0, 256, (n, hc, wc), dtype=np.uint8)}
    src = {'a': planes(), 'b': planes(), 'f': rng.standard_normal((n, h, w, 4)).astype(np.float32), None: None}
    if zero_pad:
        src['f'][..., 3] = 0.0
    if with_f3:
        src['f3'] = rng.standard_normal((n, h, w, 3)).astype(np.float32)
    return src


def conv_images_cases(oracle, h, w, n, use_gdn, part_lists, dress=None):
    """the first analysis layer (5x5 stride 2 -> 64, GDN or leaky) on every list of image sources in part_lists (names of
    _image_sources), weights drawn per list from one stream: call(ops, d) runs it from an ops.ImageStack, which the fused kernel
    must take (no packed tensor); call(ops, d, packed=True) is the pack + conv pair it replaces"""
    rng = np.random.default_rng(h * 1000 + w + (7 if use_gdn else 0))
    src = _image_sources(rng, n, h, w, True, any('f3' in pl for pl in part_lists))
    act1 = 0 if use_gdn else abi.ACT_LEAKY
    cases = []
    for pl in part_lists:
        parts = [src[nm] for nm in pl]
        ni = len(parts)
        wt = np.zeros((64, 5, 5, 4 * ni), np.float32)
        for i in range(ni):
            wt[..., 4 * i:4 * i + 3] = rng.standard_normal((64, 5, 5, 3)).astype(np.float32) / np.sqrt(75 * ni)
        bias = rng.standard_normal(64, dtype=np.float32)
        beta, gamma = _gdn_params(rng, 64) if use_gdn else (None, None)

        def call(ops, d, packed=False):
            dev = d['w'].device
            stack = ops.pack_images(d['parts'], h, w, dev) if packed else ops.ImageStack(d['parts'], h, w, dev)
            got = ops.conv2d(stack, d['w'], d['bias'], stride=2, pad=2, act1=act1, gdn=(d['beta'], d['gamma'], False) if use_gdn else None)
            assert packed or stack._packed is None, 'the fused kernel must have taken this layer (no packed tensor)'
            return got
        rf = row_facts(abi.MODE_CONV, 5, 2, 2, act1, fused_gdn=False if use_gdn else None,
                       plane_cols=[4 * j + ch for j, p in enumerate(parts) if isinstance(p, dict) for ch in range(3)])
        i = _dressed(dress, rng, {'parts': parts, 'w': wt, 'bias': bias, 'beta': beta, 'gamma': gamma}, rf)
        gdn = (beta, gamma, False) if use_gdn else None
        with np.errstate(all='ignore'):
            packed = oracle.pack_images(i['parts'], h, w)
            want = oracle.conv2d(packed, i['w'], i['bias'], stride=2, pad=2, act1=act1, gdn=gdn)
        cases.append(Case(i, call, want, act1=act1,
                          **_reached(dress, rf, i, want, lambda: oracle.conv2d(packed, i['w'], i['bias'], stride=2, pad=2, gdn=gdn))))
    return cases


def pack_images_cases(oracle, h, w, n, part_lists):
    """ops.pack_images on every list of image sources in part_lists"""
    src = _image_sources(np.random.default_rng(h * 1000 + w), n, h, w, False, any('f3' in pl for pl in part_lists))

    def call(ops, d):
        first = next(t for t in d['parts'] if t is not None)
        return ops.pack_images(d['parts'], h, w, (first['y'] if isinstance(first, dict) else first).device)
    return [Case({'parts': parts}, call, oracle.pack_images(parts, h, w)) for parts in ([src[nm] for nm in pl] for pl in part_lists)]


# ---- fp64 evaluations with torch (tests/test_oracle_winograd.py, test_gpu_precision.py, test_gpu_large_batches.py) ---------------
def torch_fp64(mode, x, w, b, stride, pad, k):
    """fp64 evaluation of the layer on the CPU (NHWC numpy in, NHWC torch out): conv with replicate padding, or ConvTranspose2d k,
    s 2, pad (1 + k) / 2 - 1, output_padding 1 (src/layers/misc/custom_conv_layers.py:129-253); w is OHWI"""
    import torch
    import torch.nn.functional as F
    xt = torch.from_numpy(np.ascontiguousarray(x)).double().permute(0, 3, 1, 2)
    wt = torch.from_numpy(np.ascontiguousarray(w)).double()
    bt = None if b is None else torch.from_numpy(np.ascontiguousarray(b)).double()
    if mode == abi.MODE_CONV:
        xp = F.pad(xt, (pad, pad, pad, pad), mode='replicate') if pad else xt
        y = F.conv2d(xp, wt.permute(0, 3, 1, 2), bt, stride=stride)
    else:
        y = F.conv_transpose2d(xt, wt.permute(3, 0, 1, 2), bt, stride=2, padding=int((1 + k) / 2 - 1), output_padding=1)
    return y.permute(0, 2, 3, 1).contiguous()


def gdn_fp64(x, beta, gamma, inverse):
    """x / sqrt(beta + gamma @ x^2) per pixel (inverse: x * sqrt(...)), fp64 torch tensors, channels last"""
    import torch
    nrm = torch.sqrt(beta + (x * x) @ gamma.t())
    return x * nrm if inverse else x / nrm


# ---- batches whose tensors contain byte 2^31 and byte 2^32 (tests/test_gpu_large_batches.py) ---------------------------------------
class Large:
    """One layer of the default model at 1080p on a batch just large enough that the tensors named in the module's table cross the
    marks.  kind: 'conv' (ops.conv2d on a float tensor), 'gdn' (ops.gdn) or 'images' (one 8-bit 4:2:0 source as an ops.ImageStack)."""

    def __init__(self, name, variants, kind, n, h, w, ci, co, mode=abi.MODE_CONV, k=1, stride=1, pad=0, act1=0, act2=0, mul=False,
                 res=False, gdn=None, precision=None):
        self.name, self.variants, self.kind, self.n, self.h, self.w, self.ci, self.co = name, variants, kind, n, h, w, ci, co
        self.mode, self.k, self.stride, self.pad, self.act1, self.act2, self.mul, self.res = mode, k, stride, pad, act1, act2, mul, res
        self.gdn, self.precision = gdn, precision  # gdn: None, False (GDN) or True (inverse): fused for 'conv' / 'images', the op of 'gdn'
        self.ho, self.wo = abi.conv_out_size(mode, h, w, k, stride, pad)

    def __repr__(self):
        return self.name


_L, _T = abi.ACT_LEAKY, abi.MODE_TCONV
LARGE_CASES = [
    Large('301-conv3-128-leaky-res', [301], 'conv', 66, 270, 480, 128, 128, k=3, stride=1, pad=1, act1=_L, res=True),
    Large('302-conv5s2-64to128', [302], 'conv', 66, 540, 960, 64, 128, k=5, stride=2, pad=2),
    Large('303-tconv5-128to64-res', [303], 'conv', 66, 270, 480, 128, 64, mode=_T, k=5, stride=2, res=True),
    Large('400-gdn128-res', [400], 'gdn', 66, 270, 480, 128, 128, mode=abi.MODE_GDN, res=True, gdn=False),
    Large('400-igdn128-res', [400], 'gdn', 66, 270, 480, 128, 128, mode=abi.MODE_IGDN, res=True, gdn=True),
    Large('400-gdn64', [400], 'gdn', 34, 540, 960, 64, 64, mode=abi.MODE_GDN, gdn=False),
    Large('2-tconv5-64to3-leaky-lean', [2], 'conv', 34, 540, 960, 64, 3, mode=_T, k=5, stride=2, act1=_L),
    Large('2-tconv5-64to6-mul-res-act2', [2], 'conv', 34, 540, 960, 64, 6, mode=_T, k=5, stride=2, act2=_L, mul=True, res=True),
    Large('1-tconv5-128to3', [1], 'conv', 18, 540, 960, 128, 3, mode=_T, k=5, stride=2),
    Large('191-images-conv5s2-gdn', [191], 'images', 34, 1080, 1920, 4, 64, k=5, stride=2, pad=2, gdn=False),
    # the version-1 pair of tests/test_gpu_fullsize_kernels.py::test_batch_beyond_4gb_goes_out_as_sub_batches
    Large('155-conv5s2-64to128-gdn-fp32', [155], 'conv', 34, 540, 960, 64, 128, k=5, stride=2, pad=2, gdn=False, precision='fp32'),
    Large('113-tconv3-64to32-leaky-fp32', [113], 'conv', 34, 540, 960, 64, 32, mode=_T, k=3, stride=2, act1=_L, precision='fp32'),
]
LARGE_CHUNK = 8     # images per small launch: every tensor of a chunk stays below 2^31 bytes
LARGE_WINDOW = 24   # output pixels per side of an fp64 window
LARGE_MARKS = (1 << 31, 1 << 32)


def large_tensors(c, dev, seed):
    """the case's operands, drawn ON THE DEVICE: weights scaled 1 / sqrt(k k c_in), positive GDN parameters, output-shaped gate
    multiplicand / residual where the case has them"""
    import torch
    g = torch.Generator(device=dev).manual_seed(seed)

    def randn(*shape):
        return torch.randn(shape, device=dev, generator=g)
    d = {}
    if c.kind == 'images':
        hc, wc = (c.h + 1) // 2, (c.w + 1) // 2
        d['planes'] = {nm: torch.randint(0, 256, (c.n, hh, ww), device=dev, generator=g, dtype=torch.uint8)
                       for nm, hh, ww in (('y', c.h, c.w), ('u', hc, wc), ('v', hc, wc))}
        d['w'] = torch.zeros((c.co, c.k, c.k, 4), device=dev)
        d['w'][..., :3] = randn(c.co, c.k, c.k, 3) / (c.k * c.k * 3) ** 0.5
    else:
        d['x'] = randn(c.n, c.h, c.w, c.ci)
    if c.kind == 'conv':
        d['w'] = randn(c.co, c.k, c.k, c.ci) / (c.k * c.k * c.ci) ** 0.5
    if c.kind != 'gdn':
        d['bias'] = randn(c.co)
    if c.gdn is not None:
        d['beta'] = torch.rand(c.co, device=dev, generator=g) + 0.5
        d['gamma'] = torch.rand((c.co, c.co), device=dev, generator=g) * 0.01
    for nm in ('mul', 'res'):
        if getattr(c, nm):
            d[nm] = randn(c.n, c.ho, c.wo, c.co)
    return d


def large_launch(ops, c, d, lo, hi):
    """the case's launch on images lo .. hi - 1 (contiguous slices of the operands) -> (output, variant codes)"""
    mul, res = (d[nm][lo:hi] if nm in d else None for nm in ('mul', 'res'))
    if c.kind == 'gdn':
        return profiled(lambda: ops.gdn(d['x'][lo:hi], d['beta'], d['gamma'], inverse=c.gdn, res=res))
    fused = None if c.gdn is None else (d['beta'], d['gamma'], c.gdn)
    kw = dict(mode=c.mode, stride=c.stride, pad=c.pad, act1=c.act1, act2=c.act2, mul=mul, res=res, gdn=fused)
    if c.kind == 'images':
        stack = ops.ImageStack([{nm: t[lo:hi] for nm, t in d['planes'].items()}], c.h, c.w, d['w'].device)
        y, codes = profiled(lambda: ops.conv2d(stack, d['w'], d['bias'], **kw))
        assert stack._packed is None, 'the fused kernel must have taken this layer (no packed tensor)'
        return y, codes
    return profiled(lambda: ops.conv2d(d['x'][lo:hi], d['w'], d['bias'], **kw))


def _mark_pixels(c, d):
    """[(tensor name, mark, image, output row, output column)]: where byte 2^31 / 2^32 of each float tensor of the case lies, as the
    output pixel that reads (input) or is (output, gate, residual) the pixel holding that byte"""
    out = []
    for nm in ('x', 'y', 'mul', 'res'):
        if nm == 'x' and 'x' not in d or nm in ('mul', 'res') and nm not in d:
            continue
        hh, ww, cc = (c.h, c.w, c.ci) if nm == 'x' else (c.ho, c.wo, c.co)
        for mark in LARGE_MARKS:
            if c.n * hh * ww * cc * 4 <= mark:
                continue
            img, off = divmod(mark, hh * ww * cc * 4)
            py, px = divmod(off // (cc * 4), ww)
            if nm == 'x' and c.mode == abi.MODE_TCONV:
                py, px = 2 * py, 2 * px
            elif nm == 'x':
                py, px = min(py // c.stride, c.ho - 1), min(px // c.stride, c.wo - 1)
            out.append((nm, mark, img, py, px))
    return out


def large_windows(c, d):
    """-> (marks, [(image, row, column)]): origins (even) of the LARGE_WINDOW-square output windows the fp64 comparison takes.
    Images: those holding a mark, the one before each, image 0 and the last; per image the top-left corner, the window against the
    bottom-right corner and one around a mark pixel (its own where it holds one, else the case's first)"""
    marks = _mark_pixels(c, d)
    s = LARGE_WINDOW

    def around(py, px):
        return min(max(py - s // 2, 0) & ~1, c.ho - s), min(max(px - s // 2, 0) & ~1, c.wo - s)
    images = sorted({0, c.n - 1} | {i for m in marks for i in (m[2] - 1, m[2]) if i >= 0})
    wins = []
    for img in images:
        own = [m for m in marks if m[2] == img] or marks[:1]
        spots = [(0, 0), (c.ho - s, c.wo - s)] + [around(m[3], m[4]) for m in own]
        wins += [(img,) + sp for sp in dict.fromkeys(spots)]
    return marks, wins


def large_window_fp64(c, d, img, oy0, ox0):
    """the layer on one output window, in fp64 on the CPU: the input window with its halo is gathered from the device; where it
    touches the image's border that border is kept (replicate padding / zero extension are the layer's own), inside the image the
    halo is real pixels.  -> numpy [LARGE_WINDOW, LARGE_WINDOW, c_out]"""
    import torch
    import torch.nn.functional as F
    s = LARGE_WINDOW
    cpu64 = lambda t: t.detach().cpu().double()  # noqa: E731
    gdn = None if c.gdn is None else (cpu64(d['beta']), cpu64(d['gamma']))
    if c.kind == 'gdn':
        v = gdn_fp64(cpu64(d['x'][img, oy0:oy0 + s, ox0:ox0 + s]), gdn[0], gdn[1], c.gdn)
    else:
        tc = c.mode == abi.MODE_TCONV
        # rows / columns of the input the window reads, before clipping to the image
        lo = [(o // 2 - 1) if tc else (o * c.stride - c.pad) for o in (oy0, ox0)]
        hi = [((o + s + 1) // 2) if tc else ((o + s - 1) * c.stride - c.pad + c.k - 1) for o in (oy0, ox0)]
        r0, c0, r1, c1 = max(lo[0], 0), max(lo[1], 0), min(hi[0], c.h - 1), min(hi[1], c.w - 1)
        if c.kind == 'images':  # 4:2:0 -> 4:4:4 as aivc_pack_images states it: level / 255, chroma by nearest neighbour, a zero 4th channel
            assert r0 % 2 == 0 and c0 % 2 == 0
            pl = d['planes']
            ch = [cpu64(pl[nm][img, r0 // 2:r1 // 2 + 1, c0 // 2:c1 // 2 + 1]).repeat_interleave(2, 0).repeat_interleave(2, 1)
                  [:r1 - r0 + 1, :c1 - c0 + 1] for nm in ('u', 'v')]
            yy = cpu64(pl['y'][img, r0:r1 + 1, c0:c1 + 1])
            patch = torch.stack([yy, ch[0], ch[1], torch.zeros_like(yy)], dim=-1) / 255.0
        else:
            patch = cpu64(d['x'][img, r0:r1 + 1, c0:c1 + 1])
        cut = (c0 - lo[1], hi[1] - c1, r0 - lo[0], hi[0] - r1)  # what the image's border took away: left, right, top, bottom
        pt = patch.permute(2, 0, 1)[None]
        pt = F.pad(pt, cut, mode='constant', value=0.0) if tc else (F.pad(pt, cut, mode='replicate') if any(cut) else pt)
        v = torch_fp64(c.mode, pt.permute(0, 2, 3, 1).numpy(), cpu64(d['w']).numpy(), cpu64(d['bias']).numpy(), c.stride, 0, c.k)[0]
        if tc:  # patch row i is input row lo + i: output row 2 (lo + i) + ..; the window starts 2 rows in, the rest is the halo ring
            v = v[2:2 + s, 2:2 + s]
        assert tuple(v.shape) == (s, s, c.co), (tuple(v.shape), cut)
        if gdn is not None:
            v = gdn_fp64(v, gdn[0], gdn[1], c.gdn)
    act = lambda a, t: torch.where(t > 0, t, t * 0.01) if a == abi.ACT_LEAKY else (t.clamp(min=0.0) if a == abi.ACT_RELU else t)  # noqa: E731
    v = act(c.act1, v)
    if 'mul' in d:
        v = cpu64(d['mul'][img, oy0:oy0 + s, ox0:ox0 + s]) * v
    if 'res' in d:
        v = v + cpu64(d['res'][img, oy0:oy0 + s, ox0:ox0 + s])
    return act(c.act2, v).numpy()
