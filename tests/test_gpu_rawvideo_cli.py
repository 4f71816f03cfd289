"""-i clip.y4m / --pix_fmt / -o out.y4m / --out_pix_fmt / --fps through the command lines, against the numpy statement of
tests/rawvideo_cases.py on the host: a 64 x 48 clip of 10 frames as 10-bit 4:4:4 .y4m (and a 66 x 50 one as headerless P010),
coded under 1_GOP_4 (two units) with synthetic weights.  The reference of every comparison is the same command line on a plain
8-bit 4:2:0 .yuv file that numpy converted, or the plain decode converted by numpy.  No tolerance: bytes with ==."""
import contextlib
import io
import os
import socket
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_cases as pc  # noqa: E402
import rawvideo_cases as rvc  # noqa: E402
import resize_cases as rc  # noqa: E402
import scene_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE, P010_SIZE = (64, 48), (66, 50)  # w x h; 66 x 50: even sides, a tight row of 132 bytes that is no multiple of 16
N, GOP = 10, '1_GOP_4'


@pytest.fixture(scope='module')
def model(cuda):
    from aivc_amd import synth
    from aivc_amd.models import arch
    return synth.make_model(arch.TINY_WIDTHS, seed=7, device=cuda)


def _run(cli, model, argv):
    """cli.main(argv) with the tiny model -> (what it returned, what it printed)"""
    from aivc_amd import decode as dec_cli
    from aivc_amd import encode as enc_cli
    mp = pytest.MonkeyPatch()
    buf = io.StringIO()
    try:
        for mod in (enc_cli, dec_cli):
            mp.setattr(mod, 'get_model', lambda name, dev: model)
        with contextlib.redirect_stdout(buf):
            out = cli.main(argv)
    finally:
        mp.undo()
    return out, buf.getvalue()


def deep_frames(name, w, h, seed):
    """N frames of the layout `name` (10-bit) grown from the synthetic 8-bit clip: every sample gets two random low bits, 4:4:4
    chroma is the 4:2:0 plane repeated with its own low bits per sample, so pairs and quads round in every way"""
    from aivc_amd import synth
    rng = np.random.default_rng(seed)
    b, depth, top, sx, sy, arr = rvc.FORMATS[name]
    assert depth == 10
    out = []
    planes, total = rvc.planes_of(name, w, h)
    pairs = arr in ('uv', 'vu')

    def deep(a, rows, cols, rx=1, ry=1):
        a = np.repeat(np.repeat(a, ry, 0), rx, 1)[:rows, :cols].astype(np.int64)
        v = (a << 2) | rng.integers(0, 4, a.shape)
        return ((v << 6) | rng.integers(0, 64, a.shape)) if top else v
    for fr in synth.synthetic_video(w, h, N, seed=seed):
        buf = np.zeros(total, np.uint8)
        rvc._put(buf, planes[0], b, deep(fr['y'], h, w))
        rows, cols = planes[1][2], planes[1][3] // (2 if pairs else 1)
        u, v = (deep(fr[k], rows, cols, 2 >> sx, 2 >> sy) for k in 'uv')
        if pairs:
            first, second = (u, v) if arr == 'uv' else (v, u)
            rvc._put(buf, planes[1], b, np.stack([first, second], 2).reshape(rows, -1))
        else:
            rvc._put(buf, planes[1], b, u)
            rvc._put(buf, planes[2], b, v)
        out.append(buf)
    return out


def converted(name, w, h, raw_frames):
    return [dict(zip('yuv', rvc.ingest(fr, name, w, h))) for fr in raw_frames]


@pytest.fixture(scope='module')
def coded(model, tmp_path_factory):
    """the 64 x 48 clip as C444p10 .y4m (frame 0 at an odd byte) and as the numpy-converted plain .yuv; encode.py --digests on the
    .y4m; the plain decode of that stream"""
    from aivc_amd import decode as dec_cli
    from aivc_amd import encode as enc_cli
    tmp = tmp_path_factory.mktemp('rawvideo_cli')
    raw = deep_frames('yuv444p10le', SIZE[0], SIZE[1], 11)
    y4m = rvc.write_y4m(str(tmp / 'clip.y4m'), 'yuv444p10le', SIZE[0], SIZE[1], raw, fps=(30, 1), header_extra=' XA')
    assert open(y4m, 'rb').read().index(b'\n') % 2 == 0  # 'FRAME\n' follows: frame 0's samples start at an odd byte
    conv = converted('yuv444p10le', SIZE[0], SIZE[1], raw)
    yuv = str(tmp / ('conv_%dx%d_30_420.yuv' % SIZE))
    cases.write_yuv(yuv, conv)
    bits = str(tmp / 'deep.bin')
    out, text = _run(enc_cli, model, ['-i', y4m, '--gop', GOP, '-o', bits, '--digests'])
    status, _ = _run(dec_cli, model, ['-i', bits, '-o', str(tmp / 'plain.yuv')])
    assert status == 0
    plain = pc.read_planes(tmp / 'plain.yuv', *SIZE)
    assert len(plain) == N
    return {'tmp': tmp, 'y4m': y4m, 'yuv': yuv, 'conv': conv, 'bits': bits, 'out': out, 'text': text, 'plain': plain}


def test_y4m_encodes_to_the_bytes_of_the_converted_file(coded, model):
    from aivc_amd import encode as enc_cli
    ref = str(coded['tmp'] / 'ref.bin')
    _, text = _run(enc_cli, model, ['-i', coded['yuv'], '--gop', GOP, '-o', ref])
    assert open(coded['bits'], 'rb').read() == open(ref, 'rb').read()
    assert '[INFO] input: yuv444p10le 64x48, 10 frames (converted to 8-bit 4:2:0 on the device)' in coded['text']
    assert '[INFO] input:' not in text and coded['out']['nb_frames_to_code'] == N


def test_headerless_p010_and_a_wrong_pix_fmt(coded, model):
    from aivc_amd import encode as enc_cli
    tmp = coded['tmp']
    w, h = P010_SIZE
    raw = deep_frames('p010le', w, h, 12)
    path = str(tmp / ('surf_%dx%d_30.yuv' % P010_SIZE))
    np.concatenate(raw).tofile(path)
    ref_yuv = str(tmp / ('surfconv_%dx%d_30_420.yuv' % P010_SIZE))
    cases.write_yuv(ref_yuv, converted('p010le', w, h, raw))
    got, ref, wrong = (str(tmp / n) for n in ('p010.bin', 'p010_ref.bin', 'p010_wrong.bin'))
    _run(enc_cli, model, ['-i', path, '--gop', GOP, '-o', got, '--pix_fmt', 'p010le'])
    _run(enc_cli, model, ['-i', ref_yuv, '--gop', GOP, '-o', ref])
    assert open(got, 'rb').read() == open(ref, 'rb').read()
    # the same bytes read as planar 10-bit (the same frame size): the comparison above can tell
    _run(enc_cli, model, ['-i', path, '--gop', GOP, '-o', wrong, '--pix_fmt', 'yuv420p10le'])
    assert open(wrong, 'rb').read() != open(got, 'rb').read()


def test_decode_to_y4m_10_bit(coded, model):
    from aivc_amd import decode as dec_cli
    out = str(coded['tmp'] / 'out.y4m')
    status, _ = _run(dec_cli, model, ['-i', coded['bits'], '-o', out, '--out_pix_fmt', 'yuv420p10le'])
    assert status == 0
    toks, name, w, h, frames = rvc.read_y4m(out)
    assert 'C420p10' in toks and 'F25:1' in toks and (name, w, h) == ('yuv420p10le', SIZE[0], SIZE[1]) and len(frames) == N
    for raw, fr in zip(frames, coded['plain']):
        words = raw.view('<u2')
        want = np.concatenate([fr[k].reshape(-1).astype(np.uint16) << 2 for k in 'yuv'])
        assert np.array_equal(words, want)
    status, _ = _run(dec_cli, model, ['-i', coded['bits'], '-o', str(coded['tmp'] / 'fps.y4m'), '--fps', '30000:1001', '--frames', '2:3'])
    toks, name, _, _, frames = rvc.read_y4m(str(coded['tmp'] / 'fps.y4m'))
    assert status == 0 and 'F30000:1001' in toks and 'C420' in toks and len(frames) == 2
    assert frames[0].tobytes() == b''.join(coded['plain'][2][k].tobytes() for k in 'yuv')


def test_decode_out_size_then_nv12(coded, model):
    from aivc_amd import decode as dec_cli
    size = (40, 30)
    out = str(coded['tmp'] / 'small_40x30.yuv')
    status, text = _run(dec_cli, model, ['-i', coded['bits'], '-o', out, '--out_size', '%dx%d' % size, '--out_pix_fmt', 'nv12', '--verify'])
    assert status == 0 and '[VERIFY] %d frames, 0 planes differ' % N in text
    data = np.fromfile(out, np.uint8).reshape(N, -1)
    for raw, fr in zip(data, coded['plain']):
        small = rc.pil_resize_frame(fr, size[0], size[1], 'bicubic')
        assert np.array_equal(raw, rvc.export(np.asarray(small['y']), np.asarray(small['u']), np.asarray(small['v']), 'nv12'))


def test_verify_against_the_manifest_of_the_10_bit_encode(coded, model):
    from aivc_amd import decode as dec_cli
    status, text = _run(dec_cli, model, ['-i', coded['bits'], '-o', str(coded['tmp'] / 'verified.y4m'), '--verify'])
    assert status == 0 and '[VERIFY] %d frames, 0 planes differ' % N in text


def test_evaluate_reads_the_y4m(coded, cuda):
    from aivc_amd import evaluate as eval_cli

    def lines(raw):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            eval_cli.main(['--raw', raw, '--compressed', str(coded['tmp'] / 'plain.yuv'), '--bitstream', coded['bits']])
        return buf.getvalue().splitlines()
    got, want = lines(coded['y4m']), lines(coded['yuv'])
    assert got == want and len(got) == 4 and got[0].startswith('PSNR') and got[3].startswith('Size [bytes]')


def test_aivc_round_trips_the_y4m(coded, model):
    """python -m aivc_amd.aivc -i clip.y4m -o out.y4m: encode, decode, evaluate, status 0"""
    from aivc_amd import aivc as aivc_cli
    tmp = coded['tmp']
    out = str(tmp / 'roundtrip.y4m')
    status, text = _run(aivc_cli, model, ['-i', coded['y4m'], '-o', out, '--bitstream_out', str(tmp / 'roundtrip.bin'), '--gop_size', '4',
                                          '--intra_period', '4', '--end_frame', str(N - 1), '--digests'])
    assert status == 0 and 'PSNR    [dB]' in text and '0 planes differ' in text
    assert open(tmp / 'roundtrip.bin', 'rb').read() == open(coded['bits'], 'rb').read()
    toks, name, w, h, frames = rvc.read_y4m(out)
    assert (name, w, h, len(frames)) == ('yuv420p', SIZE[0], SIZE[1], N)
    assert frames[3].tobytes() == b''.join(coded['plain'][3][k].tobytes() for k in 'yuv')


# ---- two ranks -----------------------------------------------------------------------------------------------------------------
def _rank(rank, world, port, q, raw, bits, argv):
    """one rank of encode.py: both on the box's one GPU over gloo, as tests/test_gpu_resize_cli.py starts its ranks"""
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
    procs = [ctx.Process(target=_rank, args=(r, 2, port, q, coded['y4m'], two, ['--gop', GOP, '--digests'])) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=300) for _ in procs)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert res == [(0, N), (1, None)]
    assert open(two, 'rb').read() == open(coded['bits'], 'rb').read()
    assert open(two + '.md5').read() == open(coded['bits'] + '.md5').read()
