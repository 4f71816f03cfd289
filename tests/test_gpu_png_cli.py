"""--png_coder through the command lines and decode_one_video: a 64 x 48 clip of 6 frames, coded under 1_GOP_4 with synthetic
weights, is decoded into two picture folders, one per coder.  The folders must hold the same names and every pair of pictures the
same pixels (the bytes differ: another filter choice, another deflate).
The odd size 71 x 39 goes through decode_one_video: decode.py itself refuses an odd --out_size with a picture folder (its
check_out_size, for the encoder's sake), whoever codes the pictures; the command line runs --out_size 72x40."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_cases as pc  # noqa: E402
import png_cases as pcs  # noqa: E402
import scene_cases as cases  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (64, 48)  # w x h
N, GOP = 6, '1_GOP_4'


@pytest.fixture(scope='module')
def model(cuda):
    from aivc_amd import synth
    from aivc_amd.models import arch
    return synth.make_model(arch.TINY_WIDTHS, seed=7, device=cuda)


def _run(cli, model, argv):
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
def coded(model, tmp_path_factory):
    from aivc_amd import encode as enc_cli
    from aivc_amd import synth
    tmp = tmp_path_factory.mktemp('png_cli')
    raw, bits = str(tmp / ('clip_%dx%d_30_420.yuv' % SIZE)), str(tmp / 'clip.bin')
    cases.write_yuv(raw, synth.synthetic_video(SIZE[0], SIZE[1], N, seed=13))
    _run(enc_cli, model, ['-i', raw, '--gop', GOP, '-o', bits])
    return {'tmp': tmp, 'bits': bits, 'stream': open(bits, 'rb').read()}


def same_pictures(a, b, n, size):
    """both folders hold 0.png ... <n - 1>.png, RGB pictures of `size` with the same pixels"""
    from PIL import Image
    names = sorted('%d.png' % i for i in range(n))
    assert sorted(os.listdir(a)) == names and sorted(os.listdir(b)) == names
    for name in names:
        for folder in (a, b):
            Image.open(os.path.join(folder, name)).verify()
        pa, pb = (np.asarray(Image.open(os.path.join(folder, name))) for folder in (a, b))
        assert pa.shape == (size[1], size[0], 3) and np.array_equal(pa, pb)


def test_decode_into_a_folder_per_coder(coded, model):
    from aivc_amd import decode as dec_cli
    tmp = coded['tmp']
    for coder, argv in (('device', ['--png_coder', 'device']), ('pillow', [])):
        status, _ = _run(dec_cli, model, ['-i', coded['bits'], '-o', str(tmp / coder) + '/'] + argv)
        assert status == 0
    same_pictures(tmp / 'device', tmp / 'pillow', N, SIZE)
    # the device's files are its coder's: one IDAT whose stream ends in the empty final stored block and the Adler-32
    idat = dict(pcs.chunks(open(tmp / 'device' / '0.png', 'rb').read()))[b'IDAT']
    assert idat[:2] == b'\x78\x01' and idat[-9:-4] == b'\x01\x00\x00\xff\xff'
    assert open(coded['bits'], 'rb').read() == coded['stream']


def test_out_size_and_a_yuv_beside(coded, model):
    from aivc_amd import decode as dec_cli
    tmp = coded['tmp']
    for coder in ('device', 'pillow'):
        status, _ = _run(dec_cli, model, ['-i', coded['bits'], '-o', str(tmp / ('small_' + coder)) + '/', '--out_size', '72x40',
                                          '--png_coder', coder])
        assert status == 0
    same_pictures(tmp / 'small_device', tmp / 'small_pillow', N, (72, 40))
    # a .yuv output does not know the flag: 'pillow' is accepted and changes nothing, 'device' is refused before anything runs
    plain, flagged = str(tmp / 'plain.yuv'), str(tmp / 'flagged.yuv')
    _run(dec_cli, model, ['-i', coded['bits'], '-o', plain])
    _run(dec_cli, model, ['-i', coded['bits'], '-o', flagged, '--png_coder', 'pillow'])
    assert open(plain, 'rb').read() == open(flagged, 'rb').read() and len(pc.read_planes(plain, *SIZE)) == N
    with pytest.raises(SystemExit):
        _run(dec_cli, model, ['-i', coded['bits'], '-o', str(tmp / 'refused.yuv'), '--png_coder', 'device'])
    assert not os.path.exists(tmp / 'refused.yuv') and open(coded['bits'], 'rb').read() == coded['stream']


def test_decode_one_video_returns_the_same_frames(coded, model, cuda):
    from aivc_amd.real_life.decode import Decoder, decode_one_video
    tmp = coded['tmp']
    dec = Decoder({'full_net': model}).eval()

    def run(**kw):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            return decode_one_video(dict({'decoder': dec, 'bitstream_path': coded['bits'], 'device': str(cuda)}, **kw))
    base = run(out_file=str(tmp / 'api_pillow') + '/')
    dev = run(out_file=str(tmp / 'api_device') + '/', png_coder='device')
    assert len(base) == len(dev) == N
    for a, b in zip(base, dev):
        assert all(np.array_equal(torch.as_tensor(a[k]).cpu().numpy(), torch.as_tensor(b[k]).cpu().numpy()) for k in 'yuv')
    same_pictures(tmp / 'api_device', tmp / 'api_pillow', N, SIZE)
    # an odd size: 71 x 39
    run(out_file=str(tmp / 'odd_pillow') + '/', out_size=(71, 39))
    run(out_file=str(tmp / 'odd_device') + '/', out_size=(71, 39), png_coder='device')
    same_pictures(tmp / 'odd_device', tmp / 'odd_pillow', N, (71, 39))
    with pytest.raises(ValueError):
        run(out_file=str(tmp / 'refused_api.yuv'), png_coder='device')
    with pytest.raises(ValueError):
        run(out_file=str(tmp / 'api_device') + '/', png_coder='zlib')


def test_save_tensor_as_img_on_the_device(coded, cuda, tmp_path):
    import torch
    from PIL import Image
    from aivc_amd.func_util.img_processing import save_tensor_as_img
    rgb = torch.from_numpy(pcs.random_picture(39, 71, 3, seed=4)).to(cuda).permute(2, 0, 1)  # [3, h, w]
    grey = torch.from_numpy(pcs.random_picture(39, 71, 1, seed=5)).to(cuda).permute(2, 0, 1)  # [1, h, w]
    for x, mode in ((rgb, 'rgb'), (grey, 'L')):
        for coder in ('pillow', 'device'):
            save_tensor_as_img(x, str(tmp_path / ('%s_%s.png' % (mode, coder))), mode=mode, coder=coder)
        a, b = (np.asarray(Image.open(tmp_path / ('%s_%s.png' % (mode, coder)))) for coder in ('pillow', 'device'))
        assert np.array_equal(a, b) and a.shape[:2] == (39, 71)
