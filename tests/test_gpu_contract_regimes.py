"""Every kind of conv launch under every numeric regime of tests/numeric_regimes.py, against the CPU oracle BY BITS
(detmath_cases.same_bits: the same pattern, or both NaN; +0 is not -0): subnormal operands and partial sums, chains that
underflow to signed zeros or overflow midway, the IEEE division and square root of the (I)GDN epilogues on subnormal numerators,
the NaN / inf footprint of single non-finite pixels.  tests/test_contract_regimes.py pins the oracle itself in these regimes.

One test id is one launch under one regime: the case is dressed by the regime (its reach condition asserted on the oracle's
result by the builder), the variant code(s) of the launch asserted, every element compared.  The rows are the smallest of
tests/conv_cases.py that still reach each kernel; the oracle's evaluation is shared by the launches of a row (algo, forced tile).
Where include/aivc_hip.h leaves the sign of a zero result open, numeric_regimes.ZERO_SIGN_OPEN names the launch and the regime,
and for those a zero of either sign matches a zero; everything else matches by bits.

The thin output layer's matrix-core kernel (variant 2) multiplies the taps a parity class lacks by a zero weight: under `nonfinite`
that term was inf * 0 = NaN (81 of 31920 outputs NaN where the oracle is finite); the kernel now computes an accumulator that
comes out NaN again by the contract's own chain (csrc/conv_thin.hip, thin_exact_acc), and these rows hold it to that."""
import functools

import pytest

from aivc_amd import abi
from conv_cases import (CONV_CASES, FUSED_GDN_CASES, FUSED_TAIL_CASES, GDN_RESIDENT_CASES, POLY_CASES, STAGED_CASES, STAGED_FUSED_GDN_CASES,
                        TC_CASES, WINO_CASES, attention_gate_case, conv_case, conv_images_cases, fp32w, fused_gdn_case, fused_tail_case,  # noqa: F401
                        gdn_resident_case, thin_walk_case, wino_case)
from numeric_regimes import REGIMES, assert_bits, zero_sign_open
from op_cases import on, profiled

pytestmark = pytest.mark.gpu

_L, _R, _S = abi.ACT_LEAKY, abi.ACT_RELU, abi.ACT_SIGMOID
_C, _T, _G, _I = abi.MODE_CONV, abi.MODE_TCONV, abi.MODE_GDN, abi.MODE_IGDN
D, A, M = abi.ALGO_DIRECT, abi.ALGO_AUTO, abi.ALGO_MFMA
IMAGE_LISTS = ('f', 'af', ('f', 'a', None))


def _row(table, *head):
    """the row of a case table that starts with head (rows are stated once, there)"""
    found = [r for r in table if r[:len(head)] == head]
    assert len(found) >= 1, head
    return found[0]


class Launch:
    """name; builder and its arguments (the regime is passed as dress=); keyword arguments of the call; the variant codes the
    launch must report; environment; `wino`: version 2 with the size rule lifted (the fp32w fixture); `pick`: which of a list of
    cases; n: images of a conv_case row under the nonfinite regime (tiny images: see numeric_regimes)"""

    def __init__(self, name, build, args, codes, kw=None, env=None, wino=False, pick=None, nonfinite_n=None):
        self.name, self.build, self.args, self.codes, self.kw, self.env = name, build, args, codes, kw or {}, env or {}
        self.wino, self.pick, self.nonfinite_n = wino, pick, nonfinite_n

    def __repr__(self):
        return self.name


@functools.lru_cache(maxsize=2)
def _built(build, args, regime, wino, extra):
    """(wino: part of the key -- the oracle's contract version at the time of the call)"""
    return build(*args, dress=regime, **dict(extra))


def case_of(launch, regime, oracle):
    extra = ()
    if launch.nonfinite_n and regime.name == 'nonfinite':
        extra = (('n', launch.nonfinite_n),)
    c = _built(launch.build, (oracle,) + launch.args, regime, launch.wino, extra)
    return c if launch.pick is None else c[launch.pick]


def _conv_launches():
    rows = [
        # row, {algo: code} (the row does not admit an algo that is absent)
        (_row(CONV_CASES, _C, 3, 1, 1, 8, 8, 9, 11), {D: 0, A: 0, M: 103}),               # scalar kernel
        (_row(CONV_CASES, _C, 3, 1, 1, 32, 32, 11, 7), {D: 0, A: 103, M: 103}),           # LDS-DMA loop, nine K tiles
        (_row(CONV_CASES, _C, 1, 1, 0, 32, 64, 9, 13), {D: 0, A: 101, M: 101}),           # ... one K tile
        (_row(CONV_CASES, _C, 5, 2, 2, 12, 64, 47, 61), {D: 0, A: 101, M: 101}),          # c_in % 8 != 0: zero-padded last group
        (_row(CONV_CASES, _C, 3, 2, 1, 128, 128, 40, 44), {D: 0, A: 101, M: 101}),
        (_row(CONV_CASES, _T, 5, 2, 0, 64, 128, 1, 3), {D: 0, A: 111, M: 111}),           # border zero fill on every tile
        (_row(CONV_CASES, _T, 3, 2, 0, 32, 64, 7, 9), {D: 0, A: 111, M: 111}),
        (_row(CONV_CASES, _T, 5, 2, 0, 8, 6, 7, 9), {D: 0, A: 0, M: 113}),                # register-staged loop
        (_row(CONV_CASES, _G, 1, 1, 0, 8, 8, 5, 7), {D: 0, A: 0, M: 123}),                # the (I)GDN mode launches
        (_row(CONV_CASES, _I, 1, 1, 0, 16, 16, 5, 7), {D: 0, A: 123, M: 123}),
        (_row(CONV_CASES, _G, 1, 1, 0, 128, 128, 33, 31), {D: 0, A: 400, M: 125}),
        # the thin output layer: 16x16x4 MFMA kernel, its lean epilogue (relu), the VALU fallback (sigmoid)
        (_row(CONV_CASES, _T, 5, 2, 0, 64, 3, 19, 70), {A: 2}),
        (_row(CONV_CASES, _T, 5, 2, 0, 64, 3, 7, 70), {A: 2}),
        (_row(CONV_CASES, _T, 5, 2, 0, 64, 6, 6, 10, _S), {A: 1}),
    ]
    out = []
    for row, codes in rows:
        name = '%s%dx%ds%d-%dto%d-%dx%d' % (('conv', 'tconv', 'gdn', 'igdn')[row[0]], row[1], row[1], row[2], row[4], row[5], row[6], row[7])
        tiny = row[6] * row[7] < 8
        for algo, code in codes.items():
            out.append(Launch('%s-%s' % (name, {D: 'direct', A: 'auto', M: 'mfma'}[algo]), conv_case, (row, abs(hash(row)) % (2 ** 31)),
                              [code], kw={'algo': algo}, nonfinite_n=6 if tiny else None))
    return out


def _staged_launches():
    out = []
    for row, _ in STAGED_CASES:
        if row[4] in (36, 12):  # c_in without whole K tiles
            digit = {_C: 0, _T: 1, _G: 2, _I: 2}[row[0]]
            for tile in (0, 5):
                out.append(Launch('staged-%s%d-c%d-tile%d' % (('conv', 'tconv', 'gdn', 'igdn')[row[0]], row[1], row[4], tile), conv_case,
                                  (row, abs(hash(row)) % (2 ** 31)), [100 + 10 * digit + tile], kw={'algo': M}, env={'AIVC_FORCE_TILE': str(tile)}))
    for row, tiles in STAGED_FUSED_GDN_CASES:
        out.append(Launch('staged-fused-gdn-tconv%d-c%d-tile%d' % (row[1], row[4], tiles[0]), fused_gdn_case, (row, abs(hash(row)) % (2 ** 31)),
                          [160 + tiles[0]], kw={'algo': M}, env={'AIVC_FORCE_TILE': str(tiles[0])}))
    return out


def _gdn_launches():
    out = []
    for idx, codes in ((2, [155]), (3, [155]), (4, [165]), (5, [161]), (7, [0, 0])):
        row = FUSED_GDN_CASES[idx]
        out.append(Launch('fused-gdn-row%d' % idx, fused_gdn_case, (row, abs(hash(row)) % (2 ** 31)), codes))
    for row in ((128, 1, 5, 7, False, False), (128, 2, 33, 31, True, False), (64, 2, 17, 19, True, True)):
        assert row in GDN_RESIDENT_CASES
        out.append(Launch('gdn-resident-%d-%dx%dx%d%s%s' % (row[:4] + ('-inverse' if row[4] else '', '-res' if row[5] else '')),
                          gdn_resident_case, (row,), [400]))
    return out


def _image_launches():
    out = []
    for (h, w, n) in ((9, 13, 2), (16, 128, 1)):
        for use_gdn in (True, False):
            for pick, pl in enumerate(IMAGE_LISTS):
                for packed in (False, True):
                    out.append(Launch('images-%dx%dx%d-%s-%s-%s' % (n, h, w, 'gdn' if use_gdn else 'leaky', ''.join(p or '0' for p in pl),
                                                                   'packed' if packed else 'fused'),
                                      conv_images_cases, (h, w, n, use_gdn, IMAGE_LISTS),
                                      # (a packed tensor of ONE float image is recognised by conv2d and takes the fused kernel as well)
                                      [(151 if use_gdn else 101) if packed and pl != 'f' else 191],
                                      kw={'packed': packed}, pick=pick))
    return out


def _other_launches():
    out = []
    for grid_bias in (True, False):
        out.append(Launch('thin-walk-grid3-%s' % ('bias' if grid_bias else 'nobias'), thin_walk_case, ((3, 5, 64, 21, 100), 303, grid_bias), [2],
                          env={'AIVC_THIN_GRID_MAX': '3'}))
    for idx in (1, 2):
        row = FUSED_TAIL_CASES[idx]
        out.append(Launch('fused-tail-row%d' % idx, fused_tail_case, (row, abs(hash(row)) % (2 ** 31)), [190]))
    for algo, code in ((D, 0), (A, 101), (M, 101)):
        out.append(Launch('attention-gate-1x9x11x128-%s' % {D: 'direct', A: 'auto', M: 'mfma'}[algo], attention_gate_case, (1, 9, 11, 128, 1.0),
                          [code], kw={'algo': algo}))
    for variant, table, heads in ((301, WINO_CASES, ((2, 7, 9, 32, 128), (5, 5, 3, 128, 128), (2, 33, 50, 64, 128))),
                                  (302, POLY_CASES, ((2, 15, 17, 64, 128), (3, 9, 7, 32, 256))),
                                  (303, TC_CASES, ((2, 7, 9, 64, 64), (3, 5, 3, 32, 128)))):
        for head in heads:
            row = _row(table, *head)
            out.append(Launch('%d-%dx%dx%d-%dto%d' % ((variant,) + head), wino_case, (variant, row, abs(hash(row)) % (2 ** 31)), [variant], wino=True))
    return out


LAUNCHES = _conv_launches() + _staged_launches() + _gdn_launches() + _image_launches() + _other_launches()


@pytest.mark.parametrize('launch', LAUNCHES, ids=repr)  # (varies fastest: the launches of a row follow each other and share its case)
@pytest.mark.parametrize('regime', REGIMES, ids=repr)
def test_launch_under_regime(launch, regime, oracle, cuda, monkeypatch, request):
    from aivc_amd import ops
    if launch.wino:
        request.getfixturevalue('fp32w')
    c = case_of(launch, regime, oracle)
    for k, v in launch.env.items():
        monkeypatch.setenv(k, v)
    if launch.build is conv_images_cases:
        monkeypatch.setattr(ops, '_CONV_IMAGES_MAX', 3)
    got, codes = profiled(lambda: c.run(ops, on(cuda), **launch.kw))
    assert codes == launch.codes, (codes, launch.codes)
    assert_bits(got.cpu().numpy(), c.want, '%r under %r, variant %s' % (launch, regime, codes), sign_of_zero_open=zero_sign_open(codes, regime))
