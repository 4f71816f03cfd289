"""Partial decode, the host side (no GPU): the reference closure and the depths of the coding structures, absolute index ->
(unit, frame) on containers of dummy payloads, the plan of a request and of a whole decode, the container index (what it reads, where it stops, what it refuses), the
--frames / --max_level flags and the manifest rows a partial --verify compares.  The decodes themselves are in
tests/test_gpu_partial_decode.py."""
import io
import itertools

import pytest

import partial_cases as pc


# ---- closure and depths ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('gop_name', pc.STRUCTURES)
def test_closure_is_the_fixed_point(gop_name):
    from aivc_amd.func_util.GOP_structure import generate_gop_struct, reference_closure
    gop = generate_gop_struct(gop_name)
    names = sorted(gop, key=lambda f: int(f.split('_')[-1]))
    for f in names:
        assert reference_closure(gop, [f]) == pc.brute_closure(gop, [f]), f
    pairs = list(itertools.combinations(names, 2))
    for pair in pairs[::max(1, len(pairs) // 12)]:
        assert reference_closure(gop, pair) == pc.brute_closure(gop, pair), pair
    assert reference_closure(gop, []) == set()
    assert reference_closure(gop, names) == set(names)
    with pytest.raises(KeyError):
        reference_closure(gop, ['frame_%d' % (len(names) + 3)])


def test_closure_figures():
    from aivc_amd.func_util.GOP_structure import generate_gop_struct, reference_closure
    g8 = generate_gop_struct('1_GOP_8')
    assert [len(reference_closure(g8, [pc.name(i)])) for i in range(9)] == [1, 5, 4, 5, 3, 5, 4, 5, 2]
    g32 = generate_gop_struct('1_GOP_32')
    assert reference_closure(g32, [pc.name(5)]) == {pc.name(i) for i in (0, 4, 5, 6, 8, 16, 32)}


@pytest.mark.parametrize('gop_name,n_levels', [('1_GOP_0', 1), ('LDP_8', 9), ('1_GOP_8', 5), ('2_GOP_4', 5), ('1_GOP_32', 7)])
def test_depths_agree_with_coding_levels(gop_name, n_levels):
    from aivc_amd.func_util.GOP_structure import coding_levels, frame_depths, generate_gop_struct
    gop = generate_gop_struct(gop_name)
    depths = frame_depths(gop)
    levels = coding_levels(gop)
    assert len(levels) == n_levels and set(depths) == set(gop)
    for k, level in enumerate(levels):
        assert all(depths[f] == k for f in level)
    for f, d in gop.items():  # a depth is one more than the deepest reference's
        refs = [depths[r] for r in (d['prev_ref'], d['next_ref']) if r is not None]
        assert depths[f] == (1 + max(refs) if refs else 0)


# ---- absolute index -> (unit, frame of the unit) ---------------------------------------------------------------------
def test_mapping_mixed_structures_and_offset_numbering():
    """LDP_2 (3 frames), 1_GOP_8 (9), LDP_2 (3): 15 frames numbered 100 ... 114"""
    from aivc_amd import partial
    blob, _ = pc.dummy_video(['LDP_2', '1_GOP_8', 'LDP_2'], 100, 15)
    v = partial.indexed_from_blob(blob)
    assert v.names == ['LDP_2', '1_GOP_8', 'LDP_2'] and (v.first, v.last) == (100, 114)
    assert [partial.locate(v.names, v.first, i) for i in (100, 102, 103, 111, 112, 114)] == [(0, 0), (0, 2), (1, 0), (1, 8), (2, 0), (2, 2)]
    assert partial.locate(v.names, v.first, 115) is None
    wanted = partial.select(v.names, v.first, v.last, [102, 108, 114])
    assert wanted == [{pc.name(2)}, {pc.name(5)}, {pc.name(2)}]
    assert partial.closures(v.names, wanted) == [{pc.name(i) for i in (0, 1, 2)}, {pc.name(i) for i in (0, 8, 4, 6, 5)},
                                                 {pc.name(i) for i in (0, 1, 2)}]
    assert partial.selected_indices(v.names, v.first, wanted) == [102, 108, 114]
    # a level: LDP_2 has the depths 0, 1, 2 along its chain; 1_GOP_8 keeps frames 0, 4, 8 at level 2
    assert partial.selected_indices(v.names, v.first, partial.select(v.names, 100, 114, None, 2)) == [100, 101, 102, 103, 107, 111, 112, 113, 114]
    assert partial.selected_indices(v.names, v.first, partial.select(v.names, 100, 114, [101, 104, 107], 2)) == [101, 107]
    assert partial.select(v.names, 100, 114, None, 99) == [{pc.name(i) for i in range(n)} for n in (3, 9, 3)]
    assert partial.coded_frames(v.names, 100, 114) == 15


def test_mapping_padded_last_unit():
    """12 frames of 1_GOP_8: frame 10 is frame 1 of unit 1 and pulls the padded frames 2, 4 and 8 of that unit"""
    from aivc_amd import partial
    blob, _ = pc.dummy_video(['1_GOP_8', '1_GOP_8'], 0, 12)
    v = partial.indexed_from_blob(blob)
    wanted = partial.select(v.names, v.first, v.last, [10])
    assert wanted == [set(), {pc.name(1)}]
    assert partial.closures(v.names, wanted) == [set(), {pc.name(i) for i in (0, 1, 2, 4, 8)}]
    assert partial.coded_frames(v.names, 0, 11) == 18
    # the padded repeats behind idx_last can never be asked for, by index or by level
    with pytest.raises(partial.FrameSelectionError, match='0 ... 11'):
        partial.select(v.names, 0, 11, [12])
    everything = partial.select(v.names, 0, 11, None, 9)
    assert everything[1] == {pc.name(0), pc.name(1), pc.name(2)}


# ---- the plan: what every layer of a decode is handed ------------------------------------------------------------------
def test_plan_of_a_whole_decode_keeps_the_padded_repeats():
    from aivc_amd import partial
    blob, gops = pc.dummy_video(['1_GOP_8', '1_GOP_8'], 0, 12)
    p = partial.plan(partial.indexed_from_blob(blob))
    every = {pc.name(i) for i in range(9)}
    assert p.whole is True and p.need == [every, every] and p.indices == list(range(12))
    assert p.wanted == [every, {pc.name(0), pc.name(1), pc.name(2)}]
    assert p.video.gops == gops and partial.plan(blob) == p  # (bytes are indexed on the way)


def test_plan_of_one_frame_behind_the_padding():
    from aivc_amd import partial
    blob, _ = pc.dummy_video(['1_GOP_8', '1_GOP_8'], 0, 12)
    p = partial.plan(partial.indexed_from_blob(blob), [10])
    assert p.whole is False and p.indices == [10]
    assert p.wanted == [set(), {pc.name(1)}] and p.need == [set(), {pc.name(i) for i in (0, 1, 2, 4, 8)}]
    assert partial.plan(blob, None, 99).whole is False  # (a level is a request, however deep)


def test_plan_with_mixed_structures_and_offset_numbering():
    """the video of test_mapping_mixed_structures_and_offset_numbering: the plan holds what the single functions return"""
    from aivc_amd import partial
    v = partial.indexed_from_blob(pc.dummy_video(['LDP_2', '1_GOP_8', 'LDP_2'], 100, 15)[0])
    for frames, max_level in (([102, 108, 114], None), (None, 2), ([101, 104, 107], 2), (None, None)):
        p = partial.plan(v, frames, max_level)
        wanted = partial.select(v.names, v.first, v.last, frames, max_level)
        assert p.video is v and p.wanted == wanted and p.indices == partial.selected_indices(v.names, v.first, wanted)
        if frames is None and max_level is None:
            assert p.need == [{pc.name(i) for i in range(n)} for n in (3, 9, 3)] and p.indices == list(range(100, 115))
        else:
            assert p.need == partial.closures(v.names, wanted)
    p = partial.plan(v, [102, 108, 114])
    assert p.indices == [102, 108, 114] and p.need == [{pc.name(i) for i in (0, 1, 2)}, {pc.name(i) for i in (0, 8, 4, 6, 5)},
                                                       {pc.name(i) for i in (0, 1, 2)}]
    with pytest.raises(partial.FrameSelectionError, match='100 ... 114'):
        partial.plan(v, [99])
    with pytest.raises(ValueError, match='unit 1: coding structure 1_GOP_8 has no frame_9'):
        partial.closures(v.names, [set(), {pc.name(9)}, None])


@pytest.mark.parametrize('frames,max_level', [([], None), ([18], None), ([-1], None), ([3], -1), (None, -2), ([1, 3, 5], 1)])
def test_requests_outside_the_stream_name_its_range(frames, max_level):
    from aivc_amd import partial
    with pytest.raises(partial.FrameSelectionError, match='0 ... 17'):
        partial.select(['1_GOP_8', '1_GOP_8'], 0, 17, frames, max_level)
    assert issubclass(partial.FrameSelectionError, ValueError)


def test_frame_range_of_the_driver():
    from aivc_amd import partial
    assert list(partial.frame_range((7, 11), 0, 17)) == [7, 8, 9, 10, 11]
    assert list(partial.frame_range((None, 7), 5, 17)) == [5, 6, 7]
    assert list(partial.frame_range((15, None), 0, 17)) == [15, 16, 17]
    assert list(partial.frame_range((None, None), 3, 5)) == [3, 4, 5]
    with pytest.raises(partial.FrameSelectionError, match='5 ... 17'):
        partial.frame_range((None, 2), 5, 17)  # (an end in front of the stream)
    with pytest.raises(partial.FrameSelectionError, match='0 ... 17'):
        partial.frame_range((40, None), 0, 17)


# ---- the container index ----------------------------------------------------------------------------------------------
def test_index_matches_unpack_video():
    from aivc_amd.real_life import cat_binary_files as container
    blob, gops = pc.dummy_video(['LDP_2', '1_GOP_8', '2_GOP_4'], 7, 21)
    data_dim, first, last, units = container.index_video(io.BytesIO(blob))
    ref = container.unpack_video(blob)
    assert (data_dim, first, last) == ref[:3] and len(units) == 3
    assert [blob[o:o + n] for o, n, _, _ in units] == ref[3] == gops
    assert [(g, r) for _, _, g, r in units] == [('LDP_2', 0.0), ('1_GOP_8', 1 / 16), ('2_GOP_4', 2 / 16)]
    f = io.BytesIO(blob)
    assert container.read_units(f, units, [2, 0]) == [gops[0], None, gops[2]]


def test_index_reads_28_bytes_for_one_unit_and_10_more_per_unit():
    from aivc_amd.real_life import cat_binary_files as container
    blob, gops = pc.dummy_video(['1_GOP_8'] * 4, 0, 36)
    for upto, walked in ((None, 4), (0, 1), (2, 3), (9, 4)):
        f = pc.CountingFile(blob)
        units = container.index_video(f, upto=upto)[3]
        assert len(units) == walked and f.nread == 18 + 10 * walked
    for upto_frame, walked in ((0, 1), (8, 1), (9, 2), (35, 4), (99, 4)):
        f = pc.CountingFile(blob)
        units = container.index_video(f, upto_frame=upto_frame)[3]
        assert len(units) == walked and f.nread == 18 + 10 * walked
    # ... and the payload of the chosen units only
    f = pc.CountingFile(blob)
    units = container.index_video(f, upto=1)[3]
    assert container.read_units(f, units, [1]) == [None, gops[1]] and f.nread == 18 + 20 + len(gops[1])


def test_index_of_a_truncated_file():
    from aivc_amd.real_life import cat_binary_files as container
    blob, gops = pc.dummy_video(['1_GOP_8', '1_GOP_8'], 0, 18)
    units = container.index_video(io.BytesIO(blob))[3]
    cut1 = blob[:units[1][0] + units[1][1] // 2]  # in the middle of unit 1
    f = io.BytesIO(cut1)
    got = container.index_video(f, upto=0)
    assert got[3] == units[:1] and container.read_units(f, got[3], [0]) == [gops[0]]
    assert container.index_video(io.BytesIO(cut1), upto_frame=8)[3] == units[:1]
    with pytest.raises(container.ContainerError):
        container.unpack_video(cut1)
    with pytest.raises(container.ContainerError):
        container.index_video(io.BytesIO(cut1))
    with pytest.raises(container.ContainerError):
        container.index_video(io.BytesIO(cut1), upto_frame=9)
    cut0 = blob[:units[0][0] + units[0][1] // 2]  # inside unit 0
    with pytest.raises(container.ContainerError):
        container.index_video(io.BytesIO(cut0), upto=0)
    for short in (blob[:10], blob[:20], blob[:25]):  # inside the video header, the first prefix, the first GOP header
        with pytest.raises(container.ContainerError):
            container.index_video(io.BytesIO(short), upto=0)


def test_the_driver_reads_a_file_once_as_far_as_the_request_reaches(tmp_path):
    from aivc_amd.real_life import cat_binary_files as container
    from aivc_amd.real_life.decode import read_plan
    blob, gops = pc.dummy_video(['1_GOP_8'] * 3, 0, 27)
    (tmp_path / 'v.bin').write_bytes(blob)
    p = read_plan(str(tmp_path / 'v.bin'), None, None)
    assert p.whole and p.video.gops == gops and p.indices == list(range(27))
    p = read_plan(str(tmp_path / 'v.bin'), (10, 12), None)  # the index stops behind unit 1, and unit 0 is not read
    assert not p.whole and p.video.names == ['1_GOP_8'] * 2 and p.video.gops == [None, gops[1]] and p.indices == [10, 11, 12]
    units = container.index_video(io.BytesIO(blob))[3]
    (tmp_path / 'cut.bin').write_bytes(blob[:units[2][0] + units[2][1] // 2])  # cut inside unit 2
    assert read_plan(str(tmp_path / 'cut.bin'), (None, 17), None).video.gops == gops[:2]
    for span, max_level in ((None, None), ((None, 18), None), (None, 1)):
        with pytest.raises(container.ContainerError):
            read_plan(str(tmp_path / 'cut.bin'), span, max_level)


# ---- the scheduler's argument checks (they come before any device work) -------------------------------------------------
def test_wanted_is_refused_with_a_shard_and_with_the_wrong_length():
    from aivc_amd.codec import FrameCodec
    fc = FrameCodec.__new__(FrameCodec)
    with pytest.raises(ValueError, match='wanted'):
        fc.decode_units([b''], None, None, shard=object(), wanted=[None])
    with pytest.raises(ValueError, match='2 selections for 1 units'):
        fc.decode_units([b''], None, None, wanted=[None, None])


def test_level_items_and_batches_take_the_closure():
    from aivc_amd.codec import level_batches, level_items
    from aivc_amd.func_util.GOP_structure import FRAME_B, coding_levels, generate_gop_struct
    gop = generate_gop_struct('1_GOP_8')
    levels = coding_levels(gop)
    need = {0: {pc.name(i) for i in (0, 8, 4, 6, 7)}, 1: {pc.name(i) for i in (0, 8, 4, 2, 1)}}
    assert level_items(gop, levels[3], [0, 1], FRAME_B, need) == [(0, pc.name(6)), (1, pc.name(2))]
    assert level_items(gop, levels[3], [0, 1], FRAME_B) == [(u, pc.name(i)) for u in (0, 1) for i in (2, 6)]
    assert list(level_batches(gop, levels[4], [0, 1], 16, need=need)) == [(FRAME_B, [(0, pc.name(7)), (1, pc.name(1))])]
    assert list(level_batches(gop, levels[4], [0, 1], 16, need={0: set(), 1: set()})) == []


# ---- the flags -----------------------------------------------------------------------------------------------------------
def test_frames_flag_forms():
    from aivc_amd import decode as dec_cli
    assert [dec_cli.parse_args(['--frames', t]).frames for t in ('7:11', '7:', ':11', '7', '0:0')] == \
        [(7, 11), (7, None), (None, 11), (7, 7), (0, 0)]
    a = dec_cli.parse_args(['--frames', '3:4', '--max_level', '2'])
    assert (a.frames, a.max_level) == ((3, 4), 2)
    a = dec_cli.parse_args([])
    assert a.frames is None and a.max_level is None


@pytest.mark.parametrize('argv', [['--frames', 'a:b'], ['--frames', '1:2:3'], ['--frames', ':'], ['--frames', ''], ['--frames', '-1:4'],
                                  ['--frames', '11:7'], ['--frames', '1.5'], ['--max_level', '-1'], ['--max_level', 'x']])
def test_malformed_flags_are_argparse_errors(argv, capsys):
    from aivc_amd import decode as dec_cli
    with pytest.raises(SystemExit) as e:
        dec_cli.parse_args(argv)
    assert e.value.code == 2 and 'usage:' in capsys.readouterr().err


# ---- the manifest rows of a partial --verify ---------------------------------------------------------------------------------
def test_manifest_subset_against_compare():
    from aivc_amd import digests
    rows = {i: tuple('%032x' % (16 * i + c) for c in range(3)) for i in range(10, 20)}
    shown = [12, 13, 17]
    found = {i: rows[i] for i in shown}
    assert digests.compare(rows, found) != []  # the whole manifest against a partial decode: every other frame `differs`
    sub = digests.manifest_subset(rows, shown)
    assert sorted(sub) == shown and digests.compare(sub, found) == []
    found[13] = (rows[13][0], '%032x' % 1, rows[13][2])
    assert digests.compare(sub, found) == ['13_u']
    # a returned frame the manifest does not list differs with all three planes
    found[25] = rows[12]
    assert digests.compare(digests.manifest_subset(rows, shown + [25]), found) == ['13_u', '25_y', '25_u', '25_v']
    assert digests.verify_lines(len(found), ['13_u'])[0] == '[VERIFY] 4 frames, 1 planes differ'
