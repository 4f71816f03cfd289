"""--size / --out_size / --resample through the command lines, against Pillow on the host: a 96 x 64 clip of 10 frames coded at
64 x 48 under 1_GOP_4 (two units) with synthetic weights.  The reference of every comparison is the same command line WITHOUT
the flag, fed with or followed by Image.resize per plane (tests/resize_cases.py: pil_resize_frame).  No tolerance: bytes with ==,
planes with array_equal."""
import contextlib
import io
import os
import socket
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_cases as pc  # noqa: E402
import resize_cases as rc  # noqa: E402
import scene_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SRC, CODED = (96, 64), (64, 48)  # w x h
N, GOP = 10, '1_GOP_4'


@pytest.fixture(scope='module')
def model(cuda):
    from aivc_amd import synth
    from aivc_amd.models import arch
    return synth.make_model(arch.TINY_WIDTHS, seed=7, device=cuda)


@pytest.fixture(scope='module')
def source():
    from aivc_amd import synth
    return synth.synthetic_video(SRC[0], SRC[1], N, seed=11)


def _yuv(tmp, name, frames, size):
    path = str(tmp / ('%s_%dx%d_30_420.yuv' % (name, size[0], size[1])))
    cases.write_yuv(path, frames)
    return path


def _run(cli, model, argv):
    """cli.main(argv) with the tiny model -> (what it returned, what it printed)"""
    mp = pytest.MonkeyPatch()
    buf = io.StringIO()
    try:
        mp.setattr(cli, 'get_model', lambda name, dev: model)
        with contextlib.redirect_stdout(buf):
            out = cli.main(argv)
    finally:
        mp.undo()
    return out, buf.getvalue()


@pytest.fixture(scope='module')
def coded(model, source, tmp_path_factory):
    """the clip as a 96 x 64 file; encode.py --size 64x48 --digests --log_dir on it; and the plain decode of that stream"""
    from aivc_amd import decode as dec_cli
    from aivc_amd import encode as enc_cli
    tmp = tmp_path_factory.mktemp('resize_cli')
    raw, bits = _yuv(tmp, 'clip', source, SRC), str(tmp / 'sized.bin')
    out, text = _run(enc_cli, model, ['-i', raw, '--gop', GOP, '-o', bits, '--size', '%dx%d' % CODED, '--digests',
                                      '--log_dir', str(tmp / 'log')])
    status, _ = _run(dec_cli, model, ['-i', bits, '-o', str(tmp / 'plain.yuv')])
    assert status == 0
    plain = pc.read_planes(tmp / 'plain.yuv', *CODED)
    assert len(plain) == N
    return {'tmp': tmp, 'raw': raw, 'bits': bits, 'out': out, 'text': text, 'plain': plain}


@pytest.mark.parametrize('name', [None, 'lanczos'])
def test_encode_size_writes_the_bytes_of_a_pillow_resized_clip(name, coded, model, source):
    from aivc_amd import encode as enc_cli
    tmp = coded['tmp']
    resized = [rc.pil_resize_frame(fr, CODED[0], CODED[1], name or 'bicubic') for fr in source]
    assert resized[0]['y'].shape == (CODED[1], CODED[0]) and resized[0]['u'].shape == (CODED[1] // 2, CODED[0] // 2)
    ref = str(tmp / ('ref_%s.bin' % name))
    _run(enc_cli, model, ['-i', _yuv(tmp, 'pil_%s' % name, resized, CODED), '--gop', GOP, '-o', ref])
    if name is None:
        got = coded['bits']
    else:
        got = str(tmp / 'lanczos.bin')
        _run(enc_cli, model, ['-i', coded['raw'], '--gop', GOP, '-o', got, '--size', '%dx%d' % CODED, '--resample', name])
    assert open(got, 'rb').read() == open(ref, 'rb').read()
    if name is not None:  # (the filter matters on this clip: the comparison above can tell them apart)
        assert open(got, 'rb').read() != open(coded['bits'], 'rb').read()


def test_flags_absent_nothing_new_runs(coded, model, source, monkeypatch):
    from aivc_amd import decode as dec_cli
    from aivc_amd import encode as enc_cli
    from aivc_amd import ops
    calls = []
    monkeypatch.setattr(ops, 'resize_u8', lambda *a, **k: calls.append(a))
    tmp = coded['tmp']
    _run(enc_cli, model, ['-i', coded['raw'], '--gop', GOP, '-o', str(tmp / 'off.bin')])
    _run(dec_cli, model, ['-i', str(tmp / 'off.bin'), '-o', str(tmp / 'off.yuv')])
    assert calls == [] and len(pc.read_planes(tmp / 'off.yuv', *SRC)) == N


def test_log_and_result_state_the_coded_size(coded):
    out = coded['out']
    assert (out['w'], out['h']) == CODED and out['nb_frames_to_code'] == N
    from aivc_amd.real_life import cat_binary_files as container
    data_dim = container.unpack_video(open(coded['bits'], 'rb').read())[0]
    assert sorted(data_dim['x']) == sorted(CODED)  # the header's frame size


@pytest.mark.parametrize('size,name', [((96, 64), None), ((97, 63), 'hamming'), ((32, 24), 'box')])
def test_decode_out_size_yuv_is_pillow_on_the_plain_decode(size, name, coded, model, capsys):
    """the .yuv output, with --verify: the digests are the coded planes', so 0 planes differ whatever the output size"""
    from aivc_amd import decode as dec_cli
    tmp = coded['tmp']
    path = str(tmp / ('out_%dx%d.yuv' % size))
    status, text = _run(dec_cli, model, ['-i', coded['bits'], '-o', path, '--out_size', '%dx%d' % size, '--verify']
                        + (['--resample', name] if name else []))
    assert status == 0 and '[VERIFY] %d frames, 0 planes differ' % N in text
    got = pc.read_planes(path, *size)
    assert len(got) == N
    for g, fr in zip(got, coded['plain']):
        want = rc.pil_resize_frame(fr, size[0], size[1], name or 'bicubic')
        assert all(np.array_equal(g[k], want[k]) for k in 'yuv')


def test_decode_out_size_pictures(coded, model, cuda):
    """<idx>.png: the pictures the plain path writes from Pillow-resized planes"""
    from PIL import Image
    from aivc_amd import decode as dec_cli
    from aivc_amd.real_life.decode import write_png_folder
    tmp = coded['tmp']
    size = (80, 56)
    status, _ = _run(dec_cli, model, ['-i', coded['bits'], '-o', str(tmp / 'png') + '/', '--out_size', '%dx%d' % size,
                                      '--resample', 'bilinear'])
    assert status == 0
    want = [rc.pil_resize_frame({k: v[None] for k, v in fr.items()}, size[0], size[1], 'bilinear') for fr in coded['plain']]
    write_png_folder([{k: torch.from_numpy(np.array(v)) for k, v in fr.items()} for fr in want], str(tmp / 'png_ref'), cuda,
                     list(range(N)))
    assert sorted(os.listdir(tmp / 'png')) == sorted('%d.png' % i for i in range(N))
    for i in range(N):
        a, b = np.asarray(Image.open(tmp / 'png' / ('%d.png' % i))), np.asarray(Image.open(tmp / 'png_ref' / ('%d.png' % i)))
        assert a.shape == (size[1], size[0], 3) and np.array_equal(a, b)


def test_partial_decode_resizes_what_it_returns(coded, model):
    from aivc_amd import decode as dec_cli
    tmp = coded['tmp']
    size = (96, 64)
    argv = ['-i', coded['bits'], '--out_size', '%dx%d' % size, '--verify']
    assert _run(dec_cli, model, argv + ['-o', str(tmp / 'whole_up.yuv')])[0] == 0
    status, text = _run(dec_cli, model, argv + ['-o', str(tmp / 'part_up.yuv'), '--frames', '2:3'])
    assert status == 0 and '[VERIFY] 2 frames, 0 planes differ' in text and 'partial decode: 2 frames written' in text
    whole, part = pc.read_planes(tmp / 'whole_up.yuv', *size), pc.read_planes(tmp / 'part_up.yuv', *size)
    assert len(part) == 2 and all(np.array_equal(g[k], w[k]) for g, w in zip(part, whole[2:4]) for k in 'yuv')
    status, _ = _run(dec_cli, model, argv + ['-o', str(tmp / 'level_up.yuv'), '--max_level', '0'])
    level = pc.read_planes(tmp / 'level_up.yuv', *size)  # the I frames: 0, 4 (the unit's last) ... of every unit
    assert status == 0 and 0 < len(level) < N and all(np.array_equal(level[0][k], whole[0][k]) for k in 'yuv')


def test_host_functions_take_the_sizes(coded, model, cuda):
    """real_life.encode.encode({'size', 'resample'}) and decode_one_video({'out_size', 'resample'}) without the command lines"""
    from aivc_amd.real_life.decode import Decoder, decode_one_video
    from aivc_amd.real_life.encode import encode
    tmp = coded['tmp']
    bits = str(tmp / 'host.bin')
    with contextlib.redirect_stdout(io.StringIO()):
        encode({'model': model, 'sequence_path': coded['raw'], 'GOP_struct_name': GOP, 'final_file': bits, 'size': CODED})
        frames = decode_one_video({'decoder': Decoder({'full_net': model}), 'bitstream_path': bits, 'device': str(cuda),
                                   'out_size': (40, 30), 'resample': 'box', 'frames': (1, 1)})
    assert open(bits, 'rb').read() == open(coded['bits'], 'rb').read()
    want = rc.pil_resize_frame({k: v[None] for k, v in coded['plain'][1].items()}, 40, 30, 'box')
    assert len(frames) == 1 and all(np.array_equal(torch.as_tensor(frames[0][k]).cpu().numpy(), want[k]) for k in 'yuv')


# ---- two ranks -----------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, q, raw, bits, argv):
    """one rank of encode.py: both on the box's one GPU over gloo, as tests/test_gpu_scene_cut.py starts its ranks"""
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      AIVC_DIST_BACKEND='gloo', AIVC_SINGLE_DEVICE='1')
    import torch.distributed as dist
    from aivc_amd import encode as enc_cli
    from aivc_amd import parallel, synth
    from aivc_amd.models import arch

    def tiny_model(name, dev):
        return parallel.broadcast_model(synth.make_model(arch.TINY_WIDTHS, seed=7, device=dev))
    enc_cli.get_model = tiny_model
    out = enc_cli.main(['-i', raw, '-o', bits] + argv)
    q.put((rank, None if out is None else out['nb_frames_to_code']))
    dist.destroy_process_group()


def test_two_ranks_write_the_bytes_of_one_process(coded):
    import torch.multiprocessing as mp
    tmp = coded['tmp']
    with socket.socket() as s:
        s.bind(('127.0.0.1', 0))
        port = s.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    two = str(tmp / 'two.bin')
    argv = ['--gop', GOP, '--size', '%dx%d' % CODED, '--digests']
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, coded['raw'], two, argv)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, N), (1, None)]
    assert open(two, 'rb').read() == open(coded['bits'], 'rb').read()
    assert open(two + '.md5').read() == open(coded['bits'] + '.md5').read()
