"""aivc_amd.color.rgb_to_yuv420 / yuv_to_rgb (aivc_rgb8_to_yuv420u8_matrix / aivc_yuv8_to_rgb8_matrix,
include/aivc_hip_color_matrix.h) against their numpy statement (aivc_amd.color.forward_numpy / inverse_numpy), byte for byte,
under the guard-zone and poison harness of tests/guarded.py: every input sits between guard zones, every output is allocated
between them, each case runs under both fills and the two results must agree.

Shapes are [n, h, w].  [2, 7, 9]: the scalar kernels, odd sides, n > 1; [2, 6, 32]: the vector kernels, two groups and three row
pairs; [1, 2, 16]: one group; [1, 1, 1]: no chroma sample, the library gets NULL u / v; [1, 8, 48] from a buffer at a one-byte
offset: the scalar kernels at a vector width.  Each under bt709 limited, bt601 full and bt2020 limited, forward with point and
box chroma, inverse with chroma_shift 0 and 1 and floor- and ceil-sized planes, on random bytes and on a picture made of the
0 / 255 corners and of the values around 16, 235 and 240.

The wrappers allocate their outputs themselves, so there is no caller's output to hand in strided; the defective-tensor cases
cover every input."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bridge  # noqa: E402
from guarded import both_fills, guarded  # noqa: E402

pytestmark = pytest.mark.gpu

SPECS = [('bt709', 'limited'), ('bt601', 'full'), ('bt2020', 'limited')]
SHAPES = [(2, 7, 9, False), (2, 6, 32, False), (1, 2, 16, False), (1, 1, 1, False), (1, 8, 48, True)]  # n, h, w, misaligned
EDGE_VALUES = np.array([0, 255, 0, 255, 15, 16, 17, 234, 235, 236, 239, 240, 241], np.uint8)
OLD = {'aivc_rgb8_to_yuv420u8', 'aivc_yuv8_to_rgb8'}
NEW = {'aivc_rgb8_to_yuv420u8_matrix', 'aivc_yuv8_to_rgb8_matrix'}


def pictures(shape, seed):
    """random bytes, and a picture of the 0 / 255 corners and the values around 16 / 235 / 240"""
    rng = np.random.default_rng(seed)
    return {'random': rng.integers(0, 256, shape, dtype=np.uint8), 'edges': EDGE_VALUES[rng.integers(0, EDGE_VALUES.size, shape)]}


def placed(a, dev, fill, misaligned):
    """`a` between guard zones; misaligned: as a contiguous tensor one byte into a guarded buffer"""
    if not misaligned:
        return guarded(a, dev, fill)
    flat = guarded(np.concatenate([np.zeros(1, np.uint8), a.reshape(-1)]), dev, fill)
    x = flat[1:].view(a.shape)
    assert x.is_contiguous() and x.data_ptr() % 2 == 1
    return x


@pytest.mark.parametrize('n,h,w,misaligned', SHAPES)
@pytest.mark.parametrize('spec', SPECS, ids=['%s-%s' % s for s in SPECS])
def test_forward_equals_the_numpy_statement(cuda, spec, n, h, w, misaligned):
    from aivc_amd import color
    ch, cw = h // 2, w // 2
    for kind, rgb in pictures((n, h, w, 3), h * 100 + w).items():
        for down in ('point', 'box'):
            want = color.forward_numpy(rgb, spec, down)
            y, u, v = both_fills(lambda fill: color.rgb_to_yuv420(placed(rgb, cuda, fill, misaligned), spec, down))
            got = (np.frombuffer(y, np.uint8).reshape(n, h, w), np.frombuffer(u, np.uint8).reshape(n, ch, cw),
                   np.frombuffer(v, np.uint8).reshape(n, ch, cw))
            for name, a, b in zip('yuv', got, want):
                assert np.array_equal(a, b), (kind, down, name)


@pytest.mark.parametrize('n,h,w,misaligned', SHAPES)
@pytest.mark.parametrize('spec', SPECS, ids=['%s-%s' % s for s in SPECS])
def test_inverse_equals_the_numpy_statement(cuda, spec, n, h, w, misaligned):
    from aivc_amd import color
    sizes = {'floor': (h // 2, w // 2, 1), 'ceil': ((h + 1) // 2, (w + 1) // 2, 1), 'full': (h, w, 0)}
    if (h, w) == (7, 9):
        assert sizes['floor'][:2] == (3, 4) and sizes['ceil'][:2] == (4, 5)
    for kind, (ch, cw, shift) in sizes.items():
        for name, ycc in pictures((3, n, max(h, 1), max(w, 1)), h * 100 + w + 7).items():
            y, u, v = ycc[0], np.ascontiguousarray(ycc[1][:, :ch, :cw]), np.ascontiguousarray(ycc[2][:, :ch, :cw])
            if kind == 'floor':  # (a second draw: the planes of the three sizes differ)
                u, v = u[:, ::-1].copy(), v[:, :, ::-1].copy()

            def case(fill):
                return color.yuv_to_rgb(*(placed(p, cuda, fill, misaligned) for p in (y, u, v)), spec, chroma_shift=shift)
            if ch * cw == 0:  # a floor-sized plane of a side of 1 is empty: no chroma to read, refused before the library
                with bridge.recording(_ops()), bridge.raises_before_the_library('an empty chroma plane'):
                    case(0xFF)
                continue
            got = np.frombuffer(both_fills(case), np.uint8).reshape(n, h, w, 3)
            assert np.array_equal(got, color.inverse_numpy(y, u, v, spec, shift)), (kind, name)


def _ops():
    from aivc_amd import ops
    return ops


# ---- the bridge: defective tensors, strided views, a side stream -----------------------------------------------------------
def wrappers(dev):
    """name -> (inputs as device tensors, launch(inputs) -> device tensors, call(inputs) -> their bytes on the host, the numpy
    statement of the plain call)"""
    from aivc_amd import color
    spec = color.ColourSpec('bt709', 'limited')
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (2, 6, 32, 3), dtype=np.uint8)
    y, u, v = rng.integers(0, 256, (2, 6, 32), dtype=np.uint8), *rng.integers(0, 256, (2, 2, 3, 16), dtype=np.uint8)

    def on_host(launch):
        return lambda d: np.concatenate([p.cpu().numpy().reshape(-1) for p in launch(d)])

    def forward(d):
        return color.rgb_to_yuv420(d['rgb'], spec, 'box')

    def inverse(d):
        return [color.yuv_to_rgb(d['y'], d['u'], d['v'], spec)]
    return {
        'rgb_to_yuv420': ({'rgb': torch.from_numpy(rgb).to(dev)}, forward, on_host(forward),
                          np.concatenate([p.reshape(-1) for p in color.forward_numpy(rgb, spec, 'box')])),
        'yuv_to_rgb': ({k: torch.from_numpy(a).to(dev) for k, a in (('y', y), ('u', u), ('v', v))}, inverse, on_host(inverse),
                       color.inverse_numpy(y, u, v, spec).reshape(-1)),
    }


@pytest.mark.parametrize('name', ['rgb_to_yuv420', 'yuv_to_rgb'])
def test_defective_tensors_are_rejected_before_the_library(cuda, name):
    ops = _ops()
    inputs, _, call, want = wrappers(cuda)[name]
    assert np.array_equal(call(inputs), want)
    with bridge.recording(ops):  # (the recorder works: the plain call reaches the library)
        with pytest.raises(bridge.Reached):
            call(inputs)
    defects = dict(bridge.DEFECTS, zero_sized=lambda t: t[:0], no_rows=lambda t: t[:, :0],
                   wrong_rank=lambda t: t.reshape((1,) + tuple(t.shape)))
    for leaf in inputs:
        for what, change in defects.items():
            with bridge.recording(ops), bridge.raises_before_the_library('%s: %s %s' % (name, leaf, what)):
                call(dict(inputs, **{leaf: change(inputs[leaf])}))
        with bridge.recording(ops), bridge.raises_before_the_library('%s: %s is no tensor' % (name, leaf)):
            call(dict(inputs, **{leaf: None}))
    from aivc_amd import color
    for bad in ({'spec': ('bt470', 'full')}, {'spec': ('bt709', 'tv')}):
        with bridge.recording(ops), bridge.raises_before_the_library('%s: %s' % (name, bad)):
            if name == 'rgb_to_yuv420':
                color.rgb_to_yuv420(inputs['rgb'], bad['spec'])
            else:
                color.yuv_to_rgb(inputs['y'], inputs['u'], inputs['v'], bad['spec'])
    with bridge.recording(ops), bridge.raises_before_the_library('chroma_down'):
        color.rgb_to_yuv420(wrappers(cuda)['rgb_to_yuv420'][0]['rgb'], ('bt709', 'limited'), 'bilinear')
    yuv = wrappers(cuda)['yuv_to_rgb'][0]
    with bridge.recording(ops), bridge.raises_before_the_library('chroma_shift'):
        color.yuv_to_rgb(yuv['y'], yuv['u'], yuv['v'], ('bt709', 'limited'), chroma_shift=2)
    with bridge.recording(ops), bridge.raises_before_the_library('half-resolution planes at chroma_shift 0'):
        color.yuv_to_rgb(yuv['y'], yuv['u'], yuv['v'], ('bt709', 'limited'), chroma_shift=0)
    with bridge.recording(ops), bridge.raises_before_the_library('u and v of two sizes'):
        color.yuv_to_rgb(yuv['y'], yuv['u'], yuv['v'][:, :2].contiguous(), ('bt709', 'limited'))


@pytest.mark.parametrize('name', ['rgb_to_yuv420', 'yuv_to_rgb'])
def test_a_strided_input_gives_the_plain_bits_or_raises(cuda, name):
    from aivc_amd._lib import AivcNativeError
    inputs, _, call, want = wrappers(cuda)[name]
    for leaf in inputs:
        view = bridge.strided(inputs[leaf])
        assert view is not None and not view.is_contiguous() and torch.equal(view, inputs[leaf])
        try:
            got = call(dict(inputs, **{leaf: view}))
        except (ValueError, AivcNativeError):
            continue
        assert np.array_equal(got, want), leaf


@pytest.mark.parametrize('name', ['rgb_to_yuv420', 'yuv_to_rgb'])
def test_a_call_on_a_side_stream_waits_for_it(cuda, name):
    """the buffers hold a decoy until a copy on the side stream, queued behind a delay, puts the real inputs there: a launch on any
    other stream reads the decoy.  The call has to be ISSUED while the delay runs, else the case proves nothing and fails."""
    ops = _ops()
    inputs, launch, _, want = wrappers(cuda)[name]
    bufs = {k: torch.full_like(t, 77) for k, t in inputs.items()}
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        done = torch.cuda.Event()
        ops.diag_hold_lds(1024, 600000)
        done.record()
        for k in bufs:
            bufs[k].copy_(inputs[k])
        with bridge.recording(ops, forward=True, probe=done.query) as rec:
            out = launch(bufs)  # (the device tensors: nothing is read back before the stream has been waited for)
    side.synchronize()
    assert np.array_equal(np.concatenate([p.cpu().numpy().reshape(-1) for p in out]), want)
    assert [nm for nm, _ in rec.calls] == ['aivc_' + {'rgb_to_yuv420': 'rgb8_to_yuv420u8_matrix', 'yuv_to_rgb': 'yuv8_to_rgb8_matrix'}[name]]
    assert rec.calls[0][1] is False, 'issued after the delay had ended (this proves nothing)'


# ---- the defaults are unchanged ------------------------------------------------------------------------------------------------
def colour_calls(rec):
    return {nm for nm, _ in rec.calls if nm in OLD | NEW}


def test_without_colour_only_the_pillow_entries_run_and_with_it_only_the_new_ones(cuda, tmp_path):
    from PIL import Image
    from aivc_amd import color
    from aivc_amd.func_util import img_processing as ip
    from aivc_amd.real_life.decode import write_png_folder
    ops = _ops()
    spec = color.ColourSpec('bt709', 'limited')
    rgb = pictures((6, 32, 3), 3)['random']
    Image.fromarray(rgb, 'RGB').save(tmp_path / 'pic.png')
    src = str(tmp_path / 'pic')

    def recorded(fn):
        with bridge.recording(ops, forward=True) as rec:
            out = fn()
        return out, rec
    for reader in ('pillow', 'device'):
        plain, rec = recorded(lambda: ip.load_RGB_as_YUV420_dic(src, cuda, reader))
        assert colour_calls(rec) == {'aivc_rgb8_to_yuv420u8'} and (reader == 'device' or len(rec.calls) == 1)
        want = ops.rgb8_to_yuv420u8(torch.from_numpy(rgb[None]).to(cuda))
        assert all(torch.equal(plain.u8[k], w) for k, w in zip('yuv', want))
        for down in ('point', 'box'):
            told, rec = recorded(lambda: ip.load_RGB_as_YUV420_dic(src, cuda, reader, colour=spec, chroma_down=down))
            assert colour_calls(rec) == {'aivc_rgb8_to_yuv420u8_matrix'} and (reader == 'device' or len(rec.calls) == 1)
            for k, w in zip('yuv', color.forward_numpy(rgb[None], spec, down)):
                assert np.array_equal(told.u8[k].cpu().numpy(), w) and told[k].shape == plain[k].shape
    with pytest.raises(ValueError):
        ip.load_RGB_as_YUV420_dic(src, cuda, chroma_down='box')

    planes = {k: t.clone() for k, t in plain.u8.items()}
    y, u, v = (planes[k].cpu().numpy() for k in 'yuv')
    up = {k: torch.from_numpy(np.repeat(np.repeat(planes[k].cpu().numpy(), 2, 1), 2, 2)).to(cuda) for k in 'uv'}
    full = dict(up, y=planes['y'])
    modes = {'yuv420': (planes, 1), 'yuv444': (full, 0), 'yuv444_nodic': (torch.cat([full[k] for k in 'yuv']), 0)}
    for mode, (x, shift) in modes.items():
        for coder in ('pillow', 'device'):
            for colour, entry in ((None, 'aivc_yuv8_to_rgb8'), (spec, 'aivc_yuv8_to_rgb8_matrix')):
                path = str(tmp_path / ('%s_%s_%s.png' % (mode, coder, colour is not None)))
                _, rec = recorded(lambda: ip.save_tensor_as_img(x, path, mode=mode, coder=coder, **({} if colour is None else {'colour': colour})))
                assert colour_calls(rec) == {entry} and (coder == 'device' or len(rec.calls) == 1)
                uu, vv = (u, v) if shift else (full['u'].cpu().numpy(), full['v'].cpu().numpy())
                want = ops.yuv8_to_rgb8(planes['y'], *((planes['u'], planes['v']) if shift else (full['u'], full['v'])),
                                        chroma_shift=shift)[0].cpu().numpy() if colour is None else color.inverse_numpy(y, uu, vv, spec, shift)[0]
                assert np.array_equal(np.asarray(Image.open(path)), want), (mode, coder, colour)

    frames = [planes, {k: 255 - t for k, t in planes.items()}]
    for coder in ('pillow', 'device'):
        for colour, entry in ((None, 'aivc_yuv8_to_rgb8'), (spec, 'aivc_yuv8_to_rgb8_matrix')):
            folder = str(tmp_path / ('folder_%s_%s' % (coder, colour is not None)))
            _, rec = recorded(lambda: write_png_folder(frames, folder, cuda, [4, 5], coder, **({} if colour is None else {'colour': colour})))
            assert colour_calls(rec) == {entry} and (coder == 'device' or [nm for nm, _ in rec.calls] == [entry] * 2)
            for idx, fr in zip((4, 5), frames):
                p = [fr[k].cpu().numpy() for k in 'yuv']
                want = ops.yuv8_to_rgb8(*(fr[k] for k in 'yuv'))[0].cpu().numpy() if colour is None else color.inverse_numpy(*p, spec, 1)[0]
                assert np.array_equal(np.asarray(Image.open(os.path.join(folder, '%d.png' % idx))), want)


def test_load_frames_takes_the_colour_with_both_readers(cuda, tmp_path):
    from PIL import Image
    from aivc_amd import color
    from aivc_amd.func_util import img_processing as ip
    spec = color.ColourSpec('bt2020', 'limited')
    rgb = pictures((3, 8, 48, 3), 9)['edges']
    for i in range(3):
        Image.fromarray(rgb[i], 'RGB').save(tmp_path / ('%d.png' % i))
    want = color.forward_numpy(rgb, spec, 'box')
    for reader in ('pillow', 'device'):
        got = ip.load_frames({'sequence_path': str(tmp_path), 'nb_frame_to_load': 3, 'rgb': True, 'device': cuda, 'png_reader': reader,
                              'colour': spec, 'chroma_down': 'box'})
        for i in range(3):
            for k, w in zip('yuv', want):
                assert np.array_equal(ip.u8_planes(got['frame_%d' % i])[k][0].cpu().numpy(), w[i]), (reader, i, k)
    with pytest.raises(ValueError):
        ip.load_frames({'sequence_path': str(tmp_path), 'nb_frame_to_load': 3, 'rgb': False, 'device': cuda, 'colour': spec})
