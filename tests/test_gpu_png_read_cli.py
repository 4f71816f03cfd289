"""--png_reader through the command lines, encode() and load_frames: picture folders of a 64 x 48 clip of 6 frames -- PNG triplets
in the old and in the clic layout, and RGB pictures -- are coded under 1_GOP_4 with synthetic weights once per reader.  What the
device reads is what Pillow reads, so the two bitstreams must be the same bytes."""
import contextlib
import io
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import partial_cases as pc  # noqa: E402

pytestmark = pytest.mark.gpu

SIZE = (64, 48)  # w x h
N, GOP = 6, '1_GOP_4'


@pytest.fixture(scope='module')
def model(cuda):
    from aivc_amd import synth
    from aivc_amd.models import arch
    return synth.make_model(arch.TINY_WIDTHS, seed=7, device=cuda)


def _run(cli, model, argv):
    from aivc_amd import encode as enc_cli
    mp = pytest.MonkeyPatch()
    buf = io.StringIO()
    try:
        for module in {cli, enc_cli}:  # (aivc.py runs the other command lines' main)
            mp.setattr(module, 'get_model', lambda name, dev: model, raising=False)
        from aivc_amd import decode as dec_cli
        mp.setattr(dec_cli, 'get_model', lambda name, dev: model, raising=False)
        with contextlib.redirect_stdout(buf):
            out = cli.main(argv)
    finally:
        mp.undo()
    return out, buf.getvalue()


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    """{'old', 'clic', 'rgb', 'palette': folder}; the frames of the triplet folders are synthetic planes, the RGB pictures their
    colour conversion; 'palette' is the RGB folder with picture 2 as a palette PNG"""
    from PIL import Image
    from aivc_amd import synth
    tmp = tmp_path_factory.mktemp('png_read_cli')
    frames = synth.synthetic_video(SIZE[0], SIZE[1], N, seed=13)
    out = {k: str(tmp / k) + '/' for k in ('old', 'clic', 'rgb', 'palette')}
    for d in out.values():
        os.makedirs(d)
    for i, fr in enumerate(frames):
        for k in 'yuv':
            Image.fromarray(fr[k]).save(out['old'] + '%d_%s.png' % (i, k))
            Image.fromarray(fr[k]).save(out['clic'] + 'clic_%05d_%s.png' % (i, k), compress_level=1)
        up = [fr['y']] + [np.repeat(np.repeat(fr[k], 2, 0), 2, 1)[:SIZE[1], :SIZE[0]] for k in 'uv']
        rgb = Image.merge('YCbCr', [Image.fromarray(p) for p in up]).convert('RGB')
        rgb.save(out['rgb'] + '%d.png' % i)
        (rgb.convert('P', palette=Image.ADAPTIVE, colors=32) if i == 2 else rgb).save(out['palette'] + '%d.png' % i)
    return tmp, out


def _encode(model, folder, bits, reader):
    from aivc_amd import encode as enc_cli
    _, text = _run(enc_cli, model, ['-i', folder, '--gop', GOP, '-o', bits] + ([] if reader is None else ['--png_reader', reader]))
    return open(bits, 'rb').read(), [line for line in text.splitlines() if line.startswith('[INFO] input:')]


@pytest.mark.parametrize('kind', ('old', 'clic', 'rgb'))
def test_the_bitstream_does_not_depend_on_the_reader(kind, folders, model):
    tmp, out = folders
    default, lines = _encode(model, out[kind], str(tmp / (kind + '_default.bin')), None)
    assert lines == []
    pillow, lines = _encode(model, out[kind], str(tmp / (kind + '_pillow.bin')), 'pillow')
    assert lines == []
    device, lines = _encode(model, out[kind], str(tmp / (kind + '_device.bin')), 'device')
    assert lines == ['[INFO] input: %d pictures inflated on the device, 0 read by Pillow' % (N if kind == 'rgb' else 3 * N)]
    assert len(device) > 100 and device == pillow == default


def test_a_palette_picture_among_the_rgb_ones(folders, model):
    tmp, out = folders
    pillow, _ = _encode(model, out['palette'], str(tmp / 'palette_pillow.bin'), 'pillow')
    device, lines = _encode(model, out['palette'], str(tmp / 'palette_device.bin'), 'device')
    assert lines == ['[INFO] input: %d pictures inflated on the device, 1 read by Pillow' % (N - 1)]
    assert len(device) > 100 and device == pillow


@pytest.mark.parametrize('kind,mode,rgb', (('old', 'old', False), ('clic', 'clic', False), ('rgb', 'old', True)))
def test_load_frames_with_both_readers(kind, mode, rgb, folders, cuda):
    from aivc_amd.func_util import img_processing as ip
    _, out = folders
    param = {'sequence_path': out[kind], 'idx_starting_frame': 1, 'nb_frame_to_load': 7, 'nb_pad_frame': 2, 'rgb': rgb,
             'loading_mode': mode, 'device': cuda}
    a = ip.load_frames(dict(param))
    b = ip.load_frames(dict(param, png_reader='device'))
    assert list(a) == list(b) == ['frame_%d' % i for i in range(7)]
    for name in a:
        assert isinstance(b[name], ip.YuvDic) and sorted(b[name]) == ['u', 'v', 'y']
        for k in 'yuv':
            assert a[name][k].shape == b[name][k].shape and a[name][k].dtype == b[name][k].dtype == torch.float32
            assert torch.equal(a[name][k].view(torch.int32), b[name][k].view(torch.int32))  # the floats, by bit pattern
            assert a[name].u8[k].shape == b[name].u8[k].shape and torch.equal(a[name].u8[k], b[name].u8[k])
    for k in 'yuv':  # the pad frames repeat frame 5, the last one read
        assert torch.equal(b['frame_5'].u8[k], b['frame_4'].u8[k]) and torch.equal(b['frame_6'].u8[k], b['frame_4'].u8[k])
        assert not torch.equal(b['frame_3'].u8[k], b['frame_4'].u8[k])
    one = (ip.load_RGB_as_YUV420_dic if rgb else ip.load_YUV_as_dic_tensor)
    name = ip._frame_storage_name(out[kind], 2, mode)
    x, y = one(name, cuda), one(name, cuda, reader='device')
    assert all(x[k].shape == y[k].shape and torch.equal(x[k], y[k]) and torch.equal(x.u8[k], y.u8[k]) for k in 'yuv')


def test_aivc_end_to_end_on_the_triplet_folder(folders, model):
    from aivc_amd import aivc as aivc_cli
    tmp, out = folders
    decoded = {}
    for reader in ('pillow', 'device'):
        bits, yuv = str(tmp / ('aivc_%s.bin' % reader)), str(tmp / ('aivc_%s_%dx%d_30_420.yuv' % ((reader,) + SIZE)))
        _, text = _run(aivc_cli, model, ['-i', out['old'], '--coding_config', 'RA', '--gop_size', '4', '--intra_period', '4', '--start_frame', '0',
                                         '--end_frame', str(N - 1), '--bitstream_out', bits, '-o', yuv, '--png_reader', reader])
        assert ('[INFO] input: %d pictures inflated on the device' % (3 * N) in text) == (reader == 'device')
        decoded[reader] = (open(bits, 'rb').read(), open(yuv, 'rb').read())
    assert decoded['device'] == decoded['pillow'] and len(pc.read_planes(str(tmp / ('aivc_device_%dx%d_30_420.yuv' % SIZE)), *SIZE)) == N
