"""One rate index per intra-period unit (FrameCodec.encode_units / encode_video with a list) and byte budgets per unit
(aivc_amd.rate_control.encode_video_budgeted), on the three-rate model and the three-unit clip of tests/rate_cases.py.

Everything is bit exact.  The yardstick of a unit coded inside a mixed-rate level batch is that unit coded ALONE at its scalar rate
by the CPU oracle (oracle/codec.py, which reads and writes the per-GOP rate byte): the same GOP record, the same reconstructions."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import rate_cases as rcase  # noqa: E402

pytestmark = pytest.mark.gpu

RATES = [0.5, 2.0, 1.25]


@pytest.fixture(scope='module')
def setup(cuda):
    from aivc_amd import synth
    model = rcase.make_model(cuda)
    fc = model.frame_codec()
    frames = synth.to_device_frames(rcase.clip(), cuda)
    return model, fc, frames


@pytest.fixture(scope='module')
def oracle_units(setup):
    """per unit: (GOP record, reconstructions) of the oracle coding that unit alone at RATES[u] (computed once)"""
    from aivc_amd.real_life import cat_binary_files as container
    from oracle import codec as ocodec
    from oracle import spec as ospec
    om = ospec.export_model(setup[0])
    out = []
    for u, r in enumerate(RATES):
        blob, rec = ocodec.encode_video(om, rcase.unit_frames(u), rcase.GOP, idx_rate=r)
        _, _, _, gops = container.unpack_video(blob)
        assert len(gops) == 1
        out.append((gops[0], rec))
    return om, out


def plane(p):
    """a [1, h, w] device plane of the codec, or an [h, w] array of the oracle -> [h, w] array"""
    return p if isinstance(p, np.ndarray) else p[0].cpu().numpy()


def same_planes(dec, ref):
    assert len(dec) == len(ref)
    for d, r in zip(dec, ref):
        for k in 'yuv':
            np.testing.assert_array_equal(plane(d[k]), plane(r[k]))


def count_rows_launches(fn):
    """fn() with a counting wrapper around aivc_amd.ops.call -> (its result, {entry point: launches})"""
    from aivc_amd import ops
    seen = {}
    real = ops.call

    def counting(name, *args):
        seen[name] = seen.get(name, 0) + 1
        return real(name, *args)
    ops.call = counting
    try:
        out = fn()
    finally:
        ops.call = real
    return out, seen


def rows_launches(seen):
    return sum(v for k, v in seen.items() if k.endswith('_rows') and k != 'aivc_warp_blend_rows')


def test_mixed_batch_equals_each_unit_alone(setup, oracle_units, cuda):
    from oracle import codec as ocodec
    _, fc, frames = setup
    om, ref = oracle_units
    with torch.no_grad():
        enc, seen = count_rows_launches(lambda: fc.encode_video(frames, rcase.GOP, idx_rate=RATES))
        blob = fc.assemble_video(enc)
        (dec, _, _, _), seen_dec = count_rows_launches(lambda: fc.decode_video(blob, cuda))
    assert fc.stream_errors() == []
    assert enc['nb_gop'] == 3
    for u, r in enumerate(RATES):
        assert enc['gops'][u] == ref[u][0], 'unit %d' % u
        assert enc['gops'][u][5] == round(r * 16)
        same_planes(enc['recs'][u], ref[u][1])
    # the mixed batches went through the gain-row kernels, in the encoder (gain + quantisation per network) and the decoder
    assert seen.get('aivc_channel_gain_rows', 0) >= 1 and seen.get('aivc_quantize_center_rows', 0) >= 1
    assert seen_dec.get('aivc_dequantize_rows', 0) >= 1
    want = [f for u in range(3) for f in ref[u][1]]
    same_planes(dec, want)
    same_planes(ocodec.decode_video(om, blob), want)


def test_refs_only_gives_the_same_records(setup, oracle_units):
    _, fc, frames = setup
    with torch.no_grad():
        enc = fc.encode_video(frames, rcase.GOP, idx_rate=RATES, recon='refs')
    assert enc['gops'] == [g for g, _ in oracle_units[1]]
    assert any(r is None for unit in enc['recs'] for r in unit)  # (frames nobody references were not reconstructed)


def test_equal_list_is_the_scalar_path(setup, cuda):
    _, fc, frames = setup
    with torch.no_grad():
        scalar, seen_scalar = count_rows_launches(lambda: fc.encode_video(frames, rcase.GOP, idx_rate=1.25))
        listed, seen_list = count_rows_launches(lambda: fc.encode_video(frames, rcase.GOP, idx_rate=[1.25] * 3))
        _, seen_mixed = count_rows_launches(lambda: fc.encode_video(frames, rcase.GOP, idx_rate=RATES))
        _, seen_dec = count_rows_launches(lambda: fc.decode_video(fc.assemble_video(listed), cuda))
    assert listed['gops'] == scalar['gops']
    assert rows_launches(seen_list) == 0 and rows_launches(seen_dec) == 0 and seen_list == seen_scalar
    assert rows_launches(seen_mixed) >= 1


def test_rate_list_is_checked(setup):
    _, fc, frames = setup
    for bad in (0.3, -1 / 16, rcase.NB_RATES - 1 + 1 / 16):
        with pytest.raises(ValueError, match='unit 1'):
            fc.encode_video(frames, rcase.GOP, idx_rate=[0.5, bad, 1.0])
    with pytest.raises(ValueError):
        fc.encode_video(frames, rcase.GOP, idx_rate=[0.5, 1.0])  # three units


@pytest.fixture(scope='module')
def alone(setup):
    """bytes of unit u's GOP record coded alone at a scalar rate (bitstream only), cached"""
    _, fc, frames = setup
    cache = {}

    def size(u, rate):
        if (u, rate) not in cache:
            with torch.no_grad():
                blobs, _, _ = fc.encode_units([frames[u * rcase.UNIT:(u + 1) * rcase.UNIT]], rcase.GOP, rate, recon='refs')
            cache[(u, rate)] = blobs[0]
        return cache[(u, rate)]
    return size


@pytest.fixture(scope='module')
def budgeted(setup):
    from aivc_amd import rate_control
    _, fc, frames = setup
    with torch.no_grad():
        return rate_control.encode_video_budgeted(fc, frames, rcase.GOP, rcase.TARGET_BPP)


def test_budgets(setup, alone, budgeted, cuda):
    from aivc_amd import rate_control
    _, fc, frames = setup
    grid = rate_control.rate_grid(rcase.NB_RATES)
    budgets = rate_control.unit_budgets(rcase.TARGET_BPP, rcase.W, rcase.H, len(frames), rcase.UNIT)
    with torch.no_grad():  # every unit at both ends: two calls
        ends = [fc.encode_video(frames, rcase.GOP, idx_rate=r, recon='refs')['gops'] for r in (grid[0], grid[-1])]
    for u in range(3):
        lean, rich = sorted((len(ends[0][u]), len(ends[1][u])))
        print('unit %d: noise %s, %d B at rate %s, %d B at rate %s, budget %d B' % (u, rcase.NOISE[u], len(ends[0][u]), grid[0],
                                                                                    len(ends[1][u]), grid[-1], budgets[u]))
        assert lean <= budgets[u] < rich  # the premise of the case (tests/rate_cases.py says which noise levels give it)
    enc = budgeted
    assert enc['budgets'] == budgets and len(enc['choices']) == 3
    for u, ch in enumerate(enc['choices']):
        print('unit %d: rate %s, %d B, probes %s' % (u, ch.rate, ch.nbytes, ch.probes))
        assert ch.rate in grid and ch.rate == enc['rates'][u] and not ch.over_budget
        assert len(enc['gops'][u]) == ch.nbytes <= budgets[u]
        assert enc['gops'][u][5] == round(ch.rate * 16)
        assert enc['gops'][u] == alone(u, ch.rate)
        rich_is_last = len(ends[1][u]) > len(ends[0][u])
        neighbour = grid[grid.index(ch.rate) + (1 if rich_is_last else -1)]
        assert len(alone(u, neighbour)) > budgets[u]
        assert len(ch.probes) <= rate_control.max_probe_calls(len(grid))
        for rate, nbytes in ch.probes:
            assert rate in grid and nbytes == len(alone(u, rate)), (u, rate)
    assert len(set(enc['rates'])) >= 2
    with torch.no_grad():
        dec, _, _, _ = fc.decode_video(fc.assemble_video(enc), cuda)
    assert fc.stream_errors() == []
    same_planes(dec, [f for unit in enc['recs'] for f in unit])


def test_a_units_choice_does_not_depend_on_its_peers(setup, budgeted):
    """what a rank of a unit-sharded job does: search its own units only"""
    from aivc_amd import rate_control
    _, fc, frames = setup
    with torch.no_grad():
        one = rate_control.encode_video_budgeted(fc, frames, rcase.GOP, rcase.TARGET_BPP, unit_filter=lambda u: u == 1)
    assert one['gops'][0] is None and one['gops'][2] is None and one['choices'][0] is None
    assert one['choices'][1] == budgeted['choices'][1]
    assert one['gops'][1] == budgeted['gops'][1] and one['rates'] == [None, budgeted['rates'][1], None]
