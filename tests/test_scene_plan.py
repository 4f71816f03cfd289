"""aivc_amd/scene.py without a GPU: the cut rule against a brute-force restatement, the unit layout's properties over every
short clip, the worked layouts of tests/scene_cases.py, the partial decoder's view of a container with those units, the
command-line flags and the C ABI of aivc_pair_sad_u8."""
import ctypes
import itertools
import os
import random
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scene_cases as cases  # noqa: E402

STRUCTURES = ('1_GOP_8', '2_GOP_4', '1_GOP_4', 'LDP_5', '1_GOP_0')


# ---- scene_cuts ----------------------------------------------------------------------------------------------------------------
def brute_cuts(sad, npix, threshold):
    """the rule of DESIGN.md 5.2, frame by frame, on the sums S_1 ... S_{n-1}"""
    n = len(sad) + 1
    S = {t: sad[t - 1] for t in range(1, n)}
    out = []
    for t in range(1, n):
        near = []
        if t - 1 in S:
            near.append(S[t - 1])
        if t + 1 in S:
            near.append(S[t + 1])
        if not near:
            continue
        if 16 * (S[t] - max(near)) >= round(16 * threshold) * npix:
            out.append(t)
    return out


def test_scene_cuts_equal_the_brute_force_rule():
    from aivc_amd.scene import scene_cuts
    rng = random.Random(5)
    seen = 0
    for _ in range(400):
        n = rng.randint(1, 14)
        npix = rng.choice([1, 7, 64 * 48])
        sad = [rng.randint(0, 40 * npix) if rng.random() < 0.7 else rng.randint(0, 255 * npix) for _ in range(n - 1)]
        thr = rng.choice([0.0, 0.0625, 1.0, 10.0, 33.3])
        got = scene_cuts(sad, npix, thr)
        assert got == brute_cuts(sad, npix, thr) and got == sorted(got) and all(1 <= t <= n - 1 for t in got)
        seen += len(got)
    assert seen > 50  # (the series do hold cuts)


def test_scene_cuts_end_rules_and_flash():
    from aivc_amd.scene import scene_cuts
    assert scene_cuts([], 10) == []                      # one frame
    assert scene_cuts([2550], 10) == []                  # two frames: no neighbour at all
    assert scene_cuts([900, 0], 10) == [1]               # t = 1 has the right neighbour only
    assert scene_cuts([0, 900], 10) == [2]               # t = n - 1 the left one only
    assert scene_cuts([50, 900, 50], 10) == [2]
    assert scene_cuts([50, 900, 900, 50], 10) == []      # a one-frame flash: two equal peaks
    assert scene_cuts([50, 900, 899, 50], 10, threshold=0.0) == [2]
    assert scene_cuts([3, 3, 3], 10, threshold=0.0) == [1, 2, 3]  # (threshold 0: a plateau is all cuts; the layout copes)
    with pytest.raises(ValueError):
        scene_cuts([1, 2], 10, threshold=-1.0)
    with pytest.raises(ValueError):
        scene_cuts([1, 2], 0)


def test_scene_cuts_threshold_boundary():
    from aivc_amd.scene import scene_cuts
    npix = 48
    # threshold 10 -> 160 sixteenths: 16 * (S_t - neighbour) >= 160 * 48 iff S_t - neighbour >= 480
    assert scene_cuts([100, 580, 100], npix) == [2]
    assert scene_cuts([100, 579, 100], npix) == []
    assert scene_cuts([100, 580, 101], npix) == []       # the larger neighbour counts
    # a threshold off the grid of sixteenths is rounded to it: 10.03 -> 160, 10.04 -> 161 sixteenths
    assert scene_cuts([100, 580, 100], npix, 10.03) == [2]
    assert scene_cuts([100, 580, 100], npix, 10.04) == []
    assert scene_cuts([100, 583, 100], npix, 10.04) == [2]  # 16 * 483 = 7728 >= 161 * 48 = 7728


@pytest.mark.parametrize('name', ['cut3', 'cut3_odd'])
def test_scene_cuts_of_the_test_clips(name):
    from aivc_amd.scene import cut_scores, scene_cuts
    frames = cases.host_frames(name)
    assert len(frames) == cases.N_FRAMES
    sad = cases.pair_sad_numpy([f['y'] for f in frames])
    npix = frames[0]['y'].size
    assert scene_cuts(sad, npix) == cases.CUTS
    mafd = [s / npix for s in sad]
    others = [v for t, v in enumerate(mafd, 1) if t not in cases.CUTS]
    print(name, 'cuts %.1f %.1f' % (mafd[10], mafd[19]), 'elsewhere %.1f ... %.1f' % (min(others), max(others)))
    if name == 'cut3':
        assert round(mafd[10], 1) == 86.0 and round(mafd[19], 1) == 69.6 and 8.3 <= round(min(others), 1) and round(max(others), 1) <= 10.9
        assert [round(s, 1) for s in cut_scores(sad, npix, cases.CUTS)] == [76.0, 59.1]
    else:
        assert round(mafd[10], 1) == 89.3 and round(mafd[19], 1) == 71.7 and round(max(others), 1) <= 13.2


# ---- plan_units ----------------------------------------------------------------------------------------------------------------
def _cut_subsets(n, rng):
    if n <= 6:
        for k in range(n):
            yield from itertools.combinations(range(1, n), k)
        return
    yield ()
    yield tuple(range(1, n))
    for _ in range(12):
        yield tuple(sorted(rng.sample(range(1, n), rng.randint(1, min(5, n - 1)))))


@pytest.mark.parametrize('gop_name', STRUCTURES)
def test_plan_units_properties(gop_name):
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    from aivc_amd.real_life.header import gop_header_bytes, parse_gop_header
    from aivc_amd.scene import plan_units
    rng = random.Random(11)
    unit = len(generate_gop_struct(gop_name))
    ra = 'GOP' in gop_name and unit > 1
    checked = 0
    for n in range(1, 41):
        uniform = plan_units(n, (), gop_name)
        nb = -(-n // unit)
        assert uniform.names == [gop_name] * nb and uniform.starts == [u * unit for u in range(nb)]  # today's layout
        assert uniform.lengths == [unit] * nb and uniform.real == [min(unit, n - u * unit) for u in range(nb)]
        for cuts in _cut_subsets(n, rng):
            lay = plan_units(n, cuts, gop_name)
            checked += 1
            assert lay.n_frames == n and len(lay) == len(lay.names) == len(lay.starts) == len(lay.lengths) == len(lay.real)
            # the units tile [0, n): back to back from 0, the last one reaches or passes n - 1
            pos = 0
            for u, (s, k, r, name) in enumerate(zip(lay.starts, lay.lengths, lay.real, lay.names)):
                assert s == pos and k == len(generate_gop_struct(name)) and k >= 1
                last = u == len(lay) - 1
                assert r == (k if not last else n - s) and 1 <= r <= k
                if r < k:  # only the last unit may be padded, and only as the configured structure
                    assert last and name == gop_name
                assert parse_gop_header(gop_header_bytes(name, 0.5)) == (name, 0.5)
                pos += k
            assert pos >= n and pos - lay.lengths[-1] < n and lay.padding == pos - n and lay.coded_frames == pos
            if unit > 1:
                assert set(cuts) <= set(lay.starts)  # every cut opens a unit
            else:
                assert lay == uniform
            if not cuts:
                assert lay == uniform
            # locate and position are inverses, over the padded repeats as well
            for t in range(pos):
                u, i = lay.locate(t)
                assert lay.position(u, i) == t and 0 <= i < lay.lengths[u]
            assert lay.keys() == [lay.locate(t) for t in range(pos)]
            with pytest.raises(IndexError):
                lay.locate(pos)
            frames = list(range(n))
            units = lay.units(frames)
            assert [f for un in units for f in un] == frames + [n - 1] * lay.padding
            # the remainder in front of a cut: the stated structures and intra frames
            bounds = [0] + sorted(cuts) + [n] if unit > 1 else [0, n]
            for a, b in zip(bounds, bounds[1:]):
                inside = [u for u, s in enumerate(lay.starts) if a <= s < b]
                whole, left = divmod(b - a, unit)
                assert [lay.names[u] for u in inside[:whole]] == [gop_name] * whole
                rest = [lay.names[u] for u in inside[whole:]]
                if b == n:
                    assert rest == ([gop_name] if left else [])
                    continue
                m = left - 1
                if left == 0:
                    assert rest == []
                elif m == 0:
                    assert rest == ['1_GOP_0']
                elif not ra:
                    assert rest == ['LDP_%d' % m]
                elif m == 1:
                    assert rest == ['LDP_1']
                else:
                    assert sum(cases.i_frames(x) for x in rest) == (1 if m % 2 == 0 else 2)
                    assert rest[1:] == ([] if m % 2 == 0 else ['1_GOP_0'])
                    k, _, s = rest[0].split('_')
                    s, even = int(s), m - m % 2
                    cfg = int(gop_name.split('_')[-1])
                    assert int(k) * s == even and s <= cfg and s & (s - 1) == 0
                    assert all(even % p for p in (2 * s, 4 * s, 8 * s) if p <= cfg)  # the largest such power of two
    assert checked > 400


def test_plan_units_rejects_cuts_outside_the_clip():
    from aivc_amd.scene import plan_units
    for bad in ([0], [10], [-1], [3, 12]):
        with pytest.raises(ValueError):
            plan_units(10, bad, '1_GOP_4')
    with pytest.raises(ValueError):
        plan_units(0, [], '1_GOP_4')
    assert plan_units(10, [3, 3, 7], '1_GOP_4') == plan_units(10, [7, 3], '1_GOP_4')


@pytest.mark.parametrize('clip,gop_name', sorted(cases.LAYOUTS))
def test_worked_layouts(clip, gop_name):
    from aivc_amd.scene import plan_units
    names, real = cases.LAYOUTS[(clip, gop_name)]
    lay = plan_units(cases.N_FRAMES, cases.CUTS, gop_name)
    assert lay.names == names and lay.real == real
    assert lay.padding == {'1_GOP_8': 3, '2_GOP_4': 3, '1_GOP_4': 4}[gop_name]
    assert lay.summary().startswith('%d (' % len(names))


def test_layout_summary_names_in_order_of_first_use():
    from aivc_amd.scene import plan_units
    assert plan_units(cases.N_FRAMES, cases.CUTS, '1_GOP_8').summary() == '4 (3 x 1_GOP_8, 1 x LDP_1)'
    assert plan_units(cases.N_FRAMES, cases.CUTS, '1_GOP_4').summary() == '8 (5 x 1_GOP_4, 2 x 1_GOP_0, 1 x 1_GOP_2)'


def test_partial_plan_reads_the_layout_of_a_container():
    """a container of dummy records under the cut3 / 1_GOP_8 layout's names: the partial decoder finds every absolute frame in
    the unit and at the index the layout gives"""
    from aivc_amd import partial
    from aivc_amd.codec import make_data_dim
    from aivc_amd.func_util.GOP_structure import generate_gop_struct
    from aivc_amd.real_life import cat_binary_files as container
    from aivc_amd.real_life import header as hdr
    from aivc_amd.scene import plan_units
    lay = plan_units(cases.N_FRAMES, cases.CUTS, '1_GOP_8')
    first = 100
    gops = [container.pack_gop(hdr.gop_header_bytes(name, 0), [b'\x00' * 3] * len(generate_gop_struct(name))) for name in lay.names]
    blob = container.pack_video(hdr.video_header_bytes(make_data_dim(48, 64, (3, 4), (1, 1)), len(gops), first,
                                                       first + cases.N_FRAMES - 1), gops)
    for t in (10, 11, 19, 20, 25):
        plan = partial.plan(blob, frames=[first + t])
        assert plan.video.names == lay.names
        u, i = lay.locate(t)
        assert [sorted(w) for w in plan.wanted] == [['frame_%d' % i] if k == u else [] for k in range(len(lay))]
        assert partial.locate(lay.names, first, first + t) == (u, i)
    assert [lay.locate(t) for t in (10, 11, 19, 20, 25)] == [(1, 1), (2, 0), (2, 8), (3, 0), (3, 5)]


# ---- sequence_result_from_rows / budgets by the layout ------------------------------------------------------------------------
def test_sequence_result_names_frames_by_the_layout():
    from aivc_amd.model_mngt.model_management import sequence_result_from_rows
    from aivc_amd.quality import ROW_LEN
    from aivc_amd.scene import plan_units
    lay = plan_units(cases.N_FRAMES, cases.CUTS, '1_GOP_8')
    def row(k):  # sse x 3, alpha / beta / warping sums, ms-ssim x 3, four section sizes, h, w
        r = np.zeros(ROW_LEN)
        r[0:3], r[3:6], r[6:9], r[9:13], r[13], r[14] = 100.0 + k, 10.0, 0.5, 7.0 + k, 48, 64
        return r
    rows = {key: row(k) for k, key in enumerate(lay.keys())}
    seq = sequence_result_from_rows(rows, len(lay), lay, 7, cases.N_FRAMES, 0.0)
    assert list(seq)[:-1] == ['frame_%d' % (7 + t) for t in range(lay.coded_frames)] and list(seq)[-1] == 'sequence'
    # the distortion of the sequence row is the mean over the 26 real frames: the 3 padded repeats of the last unit are left out
    mses = [seq['frame_%d' % (7 + t)]['mse'] for t in range(lay.coded_frames)]
    assert lay.padding == 3 and seq['sequence']['mse'] == pytest.approx(sum(mses[:cases.N_FRAMES]) / cases.N_FRAMES, rel=1e-12)
    # an int unit is the uniform layout, as before
    uni = {(u, i): row(u * 9 + i) for u in range(3) for i in range(9)}
    assert list(sequence_result_from_rows(uni, 3, 9, 0, 23, 0.0))[:-1] == ['frame_%d' % t for t in range(27)]
    with pytest.raises(ValueError):
        sequence_result_from_rows(rows, len(lay) + 1, lay, 7, cases.N_FRAMES, 0.0)


def test_layout_budgets_weigh_the_real_frames():
    from aivc_amd import rate_control
    from aivc_amd.scene import plan_units
    lay = plan_units(cases.N_FRAMES, cases.CUTS, '1_GOP_8')
    assert rate_control.layout_budgets(0.5, 64, 48, lay) == [int(0.5 * 64 * 48 * r // 8) for r in (9, 2, 9, 6)]
    uniform = plan_units(23, (), '1_GOP_8')
    assert rate_control.layout_budgets(0.37, 64, 48, uniform) == rate_control.unit_budgets(0.37, 64, 48, 23, 9)


# ---- flags ---------------------------------------------------------------------------------------------------------------------
def test_encode_flag(monkeypatch, capsys):
    from aivc_amd import encode as enc_cli
    assert enc_cli.parse_args(['-i', 'clip_8x8_1_420.yuv']).scene_cut is None
    assert enc_cli.parse_args(['-i', 'clip_8x8_1_420.yuv', '--scene_cut']).scene_cut == 10.0
    assert enc_cli.parse_args(['--scene_cut', '-i', 'clip_8x8_1_420.yuv']).scene_cut == 10.0
    assert enc_cli.parse_args(['--scene_cut', '7.5']).scene_cut == 7.5
    assert enc_cli.parse_args(['--scene_cut', '0']).scene_cut == 0.0
    with pytest.raises(SystemExit) as e:
        enc_cli.parse_args(['--scene_cut', '-1'])
    assert e.value.code == 2 and '--scene_cut' in capsys.readouterr().err
    seen = {}
    monkeypatch.setattr(enc_cli, 'get_model', lambda name, dev: None)
    monkeypatch.setattr(enc_cli, 'resolve_device', lambda cpu: 'cpu')
    monkeypatch.setattr(enc_cli, 'encode', lambda param: seen.update(param))
    enc_cli.main(['-i', 'clip_8x8_1_420.yuv', '--gop', '1_GOP_4'])
    assert seen['scene_cut'] is None
    enc_cli.main(['-i', 'clip_8x8_1_420.yuv', '--gop', '1_GOP_4', '--scene_cut', '12', '--target_bpp', '0.5', '--digests',
                  '--log_dir', 'x'])
    assert seen['scene_cut'] == 12.0 and seen['target_bpp'] == 0.5 and seen['digests'] is True and seen['working_dir'] == 'x'


def test_help_says_the_default_is_a_convention(capsys):
    from aivc_amd import encode as enc_cli
    with pytest.raises(SystemExit):
        enc_cli.parse_args(['--help'])
    text = ' '.join(capsys.readouterr().out.split())
    assert '--scene_cut [T]' in text and 'not been measured' in text


def test_aivc_flag_reaches_the_encoder(monkeypatch, capsys):
    from aivc_amd import aivc as aivc_cli
    assert aivc_cli.parse_args([]).scene_cut is None
    assert aivc_cli.parse_args(['--scene_cut']).scene_cut == 10.0
    assert aivc_cli.parse_args(['--scene_cut', '4.25']).scene_cut == 4.25
    with pytest.raises(SystemExit) as e:
        aivc_cli.parse_args(['--scene_cut', '-0.5'])
    assert e.value.code == 2 and '--scene_cut' in capsys.readouterr().err
    calls = []
    monkeypatch.setattr(aivc_cli.enc_cli, 'main', lambda argv: calls.append(list(argv)))
    monkeypatch.setattr(aivc_cli.dec_cli, 'main', lambda argv: 0)
    monkeypatch.setattr(aivc_cli.eval_cli, 'main', lambda argv: None)
    aivc_cli.main(['-i', 'clip_8x8_1_420.yuv', '--scene_cut', '4.25'])
    aivc_cli.main(['-i', 'clip_8x8_1_420.yuv'])
    assert '--scene_cut' in calls[0] and float(calls[0][calls[0].index('--scene_cut') + 1]) == 4.25
    assert '--scene_cut' not in calls[1]
    from aivc_amd import encode as enc_cli
    assert enc_cli.parse_args(calls[0]).scene_cut == 4.25


# ---- the C ABI -----------------------------------------------------------------------------------------------------------------
def test_abi_binds_and_library_exports_pair_sad():
    from aivc_amd import abi
    assert abi.ABI_VERSION >= 24 and set(abi.SCENE_PROTOTYPES) == {'aivc_pair_sad_u8'}
    assert not set(abi.SCENE_PROTOTYPES) & set(abi.PROTOTYPES)  # device only: the oracle has no `_ref` twin
    lib_path = os.path.join(ROOT, 'aivc_amd', 'lib', 'libaivc_hip.so')
    if not os.path.exists(lib_path):
        import __graft_entry__ as g
        g.build_hip()
    lib = ctypes.CDLL(lib_path)  # loads without a GPU (no compute call is made)
    assert hasattr(lib, 'aivc_pair_sad_u8')
    lib.aivc_abi_version.restype = ctypes.c_int
    assert lib.aivc_abi_version() == abi.ABI_VERSION
    header = open(os.path.join(ROOT, 'include', 'aivc_hip_scene.h')).read()
    assert 'int aivc_pair_sad_u8(const uint8_t *const *planes, int32_t n, int64_t len, uint64_t *partials, uint64_t *sad,' in header
    assert '#define AIVC_SAD_BLOCKS %d\n' % abi.SAD_BLOCKS in header
    assert '#define AIVC_ABI_VERSION %d\n' % abi.ABI_VERSION in open(os.path.join(ROOT, 'include', 'aivc_hip.h')).read()


def test_pair_sad_argument_errors_without_gpu():
    """error paths return codes before anything is launched (stand-in pointers are never read through)"""
    from aivc_amd import _lib
    sad = _lib.load()['aivc_pair_sad_u8']
    assert sad(None, 0, 4, None, None, None) == 0 and sad(None, 1, 4, None, None, None) == 0  # n <= 1 does nothing
    assert sad(None, 1, -4, None, None, None) == 0
    assert sad(16, -1, 4, 16, 16, None) == -1
    assert sad(None, 2, 4, 16, 16, None) == -1
    assert sad(16, 2, 0, 16, 16, None) == -1 and sad(16, 2, -1, 16, 16, None) == -1
    assert sad(16, 2, 4, None, 16, None) == -1 and sad(16, 2, 4, 16, None, None) == -1
    assert sad(16, 65538, 4, 16, 16, None) == -2  # more pairs than grid.y holds


def test_pair_sad_rejects_cpu_tensors_and_stacks():
    import torch
    from aivc_amd import ops
    from aivc_amd._lib import AivcNativeError
    with pytest.raises(AivcNativeError):
        ops.pair_sad_u8([torch.zeros(8, dtype=torch.uint8), torch.zeros(8, dtype=torch.uint8)])
    with pytest.raises(ValueError):
        ops.pair_sad_u8(torch.zeros(2, 8, dtype=torch.uint8))
