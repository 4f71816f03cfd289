"""Image helpers with the reference's names (src/func_util/img_processing.py).

PNG decoding and encoding are Pillow's on the host unless a caller asks for reader='device' / coder='device' (aivc_amd/png.py:
the same pixels, inflated or coded on the device); colour conversion and chroma resampling run on the device
(ops.rgb8_to_yuv420u8 / ops.yuv8_to_rgb8, include/aivc_hip_color.h), bit for bit what Pillow computes for the reference.
Pillow's arithmetic is BT.601, full range; a caller who names what the planes carry (`colour`, an aivc_amd.color.ColourSpec:
BT.601 / 709 / 2020, full or limited range) gets that conversion instead (aivc_amd/color.py), between the same PNG reading and
coding.  colour None, the default everywhere, is Pillow's arithmetic through the calls above.

The loaders return what the reference returns -- float tensors in [0, 1], value k / 255 for the 8-bit level k -- but on the
device (`device` argument / param entry, default 'cuda'), and as a YuvDic: a dict that also carries the uint8 planes it was made
from (`.u8`, {'y','u','v'} of [1, h, w]), which is what the codec's 8-bit first layer takes (u8_planes()).

Chroma sizes: a frame loaded from an RGB PNG has the reference's FLOOR-sized chroma planes (h // 2, w // 2); the planar .yuv
path of this package stores CEIL-sized ones.  They agree for even h and w."""
import os

import numpy as np
import torch

from .. import ops
from ..options import SINK, SOURCE, Source
from .nn_util import get_value


class YuvDic(dict):
    """{'y','u','v'} float tensors; .u8: the same planes as uint8 [1, h, w] tensors"""
    u8 = None


def u8_planes(frame):
    """uint8 planes {'y','u','v'} of [1, h, w] of a loaded frame: the ones it was made from, or round(255 x) of its floats
    (exact for k / 255)"""
    if getattr(frame, 'u8', None) is not None:
        return frame.u8
    return {k: (frame[k] if frame[k].dtype == torch.uint8 else torch.round(frame[k].float() * 255.0).to(torch.uint8))
            .reshape(1, frame[k].shape[-2], frame[k].shape[-1]) for k in ('y', 'u', 'v')}


def get_y_u_v(x):
    return x.get('y'), x.get('u'), x.get('v')


def cast_before_png_saving(param):
    """round(255 * clamp(x, 0, 1)) / 255, half to even (src/func_util/img_processing.py:31-75)."""
    default = {'x': None, 'data_type': 'yuv_dic'}
    x = get_value('x', param, default)
    data_type = get_value('data_type', param, default)

    def cast(t):
        flat = t.contiguous().view(1, 1, -1, 1)
        # x*1 through the 3-channel reconstruction kernel would also work; a 1-channel image cast is
        # the quantise-to-8-bit special case of aivc_frame_to_yuv420 with h = numel, w = 1
        pad = torch.zeros((1, flat.shape[2], 1, 3), dtype=torch.float32, device=t.device)
        pad[..., 0] = flat[..., 0]
        (y, _, _), _ = ops.frame_to_yuv420(pad, flat.shape[2], 1, want_u8=False)
        return y.view(t.shape)
    if data_type == 'tensor':
        return cast(x)
    return {c: cast(x.get(c)) for c in ('y', 'u', 'v')}


def interpolate_nearest(x, scale=2):
    return torch.nn.functional.interpolate(x, scale_factor=scale, mode='nearest')


def _frame_storage_name(sequence_path, absolute_idx, loading_mode):
    if loading_mode == 'old':
        return sequence_path + str(absolute_idx)
    if loading_mode == 'clic':
        return sequence_path + sequence_path.split('/')[-2] + '_' + str(absolute_idx).zfill(5)
    raise ValueError('load_frames: loading_mode %r (expected old or clic)' % (loading_mode,))


def _rgb_to_planes(rgb, source):
    """uint8 RGB [n, h, w, 3] on the device -> (y, u, v): Pillow's arithmetic (source.colour None), or the named one"""
    from .. import color
    color.check_convertible(source.colour, source.chroma_down, None, True)
    if source.colour is None:
        return ops.rgb8_to_yuv420u8(rgb)
    return color.rgb_to_yuv420(rgb, source.colour, source.chroma_down)


def _planes_to_rgb(y, u, v, chroma_shift, colour=None):
    """uint8 planes on the device -> RGB [n, h, w, 3]: Pillow's arithmetic (colour None), or the named one"""
    if colour is None:
        return ops.yuv8_to_rgb8(y, u, v, chroma_shift=chroma_shift)
    from .. import color
    return color.yuv_to_rgb(y, u, v, colour, chroma_shift=chroma_shift)


def load_frames(param):
    """{'frame_0': {'y','u','v'}, 'frame_1': ...} from the folder <sequence_path> (src/func_util/img_processing.py:78-176):
    <idx>_{y,u,v}.png ('old'), <folder name>_<idx, 5 digits>_{y,u,v}.png ('clic'), or one RGB <name>.png per frame (rgb).
    nb_frame_to_load frames from idx_starting_frame on; the last nb_pad_frame of them are not read but repeat the last frame
    that was.  Every plane is a [1, 1, h, w] float tensor on param['device'] (default 'cuda').
    png_reader: 'pillow' (the default) -- one Image.open per picture on the host; 'device' -- the clip's pictures are read by ONE
    aivc_amd.png.read_pictures call (y, u and v together as grey pictures; RGB pictures, then one colour launch per picture size),
    the same planes.  png_stats: a dict that call counts into ('device', 'pillow').
    colour: None (the default) -- RGB pictures become planes by Pillow's arithmetic; an aivc_amd.color.ColourSpec -- by that matrix
    and range, chroma_down 'point' (the default: the chroma of pixel (2i, 2j)) or 'box' (of the 2 x 2 block, rounded once).  Both
    apply to rgb folders only, after the pictures have been read by either reader."""
    default = {'sequence_path': None, 'idx_starting_frame': 0, 'nb_frame_to_load': 3, 'nb_pad_frame': 0, 'rgb': False,
               'loading_mode': 'old', 'device': 'cuda', 'png_stats': None, **SOURCE._asdict()}
    sequence_path = get_value('sequence_path', param, default)
    first = get_value('idx_starting_frame', param, default)
    nb = get_value('nb_frame_to_load', param, default)
    nb_pad = get_value('nb_pad_frame', param, default)
    rgb = get_value('rgb', param, default)
    loading_mode = get_value('loading_mode', param, default)
    device = get_value('device', param, default)
    source = Source.from_param(param)
    from .. import color, png
    color.check_convertible(source.colour, source.chroma_down, sequence_path, rgb)
    if not sequence_path.endswith('/'):
        sequence_path += '/'
    last_loaded = first + nb - nb_pad - 1
    if png.check_reader(source.png_reader) == 'device':
        idx = [min(first + gop_idx, last_loaded) for gop_idx in range(nb)]
        read = _load_on_device({i: _frame_storage_name(sequence_path, i, loading_mode) for i in sorted(set(idx))}, rgb, device,
                               get_value('png_stats', param, default), source)
        return {'frame_' + str(gop_idx): _from_u8(read[i], 4) for gop_idx, i in enumerate(idx)}
    frames = {}
    for gop_idx in range(nb):
        name = _frame_storage_name(sequence_path, min(first + gop_idx, last_loaded), loading_mode)
        if rgb:
            frames['frame_' + str(gop_idx)] = load_RGB_as_YUV420_dic(name, device, colour=source.colour, chroma_down=source.chroma_down)
        else:
            frames['frame_' + str(gop_idx)] = _with_batch_dim(load_YUV_as_dic_tensor(name, device))
    return frames


def _load_on_device(names, rgb, device, stats=None, source=SOURCE):
    """{frame index: storage name} -> {frame index: uint8 planes {'y','u','v'} of [1, h, w]}: one read_pictures call for the clip"""
    from .. import png
    order = list(names)
    if not rgb:
        pics = png.read_pictures([names[i] + '_' + k + '.png' for i in order for k in 'yuv'], device, 'L', stats)
        return {i: {k: pics[3 * n + j].view(1, *pics[3 * n + j].shape[:2]) for j, k in enumerate('yuv')} for n, i in enumerate(order)}
    pics = png.read_pictures([names[i] + '.png' for i in order], device, 'RGB', stats)
    out = {}
    for shape in sorted({tuple(p.shape) for p in pics}):  # (a clip has one size: one colour launch)
        group = [n for n, p in enumerate(pics) if tuple(p.shape) == shape]
        y, u, v = _rgb_to_planes(torch.stack([pics[n] for n in group]), source)
        for j, n in enumerate(group):
            out[order[n]] = {'y': y[j:j + 1], 'u': u[j:j + 1], 'v': v[j:j + 1]}
    return out


def _with_batch_dim(x):
    out = YuvDic({k: x[k].view(1, *x[k].shape) for k in ('y', 'u', 'v')})
    out.u8 = x.u8
    return out


_LEVELS = {}


def _levels(device):
    """k / 255 for k = 0 .. 255 as to_tensor computes it on the host, the correctly rounded quotient, on `device`.  Dividing a
    device tensor by the number 255 multiplies by the rounded reciprocal instead and is one ulp off for some k."""
    device = torch.device(device)
    if device not in _LEVELS:
        _LEVELS[device] = torch.from_numpy(np.arange(256, dtype=np.float32) / np.float32(255)).to(device)
    return _LEVELS[device]


def _from_u8(planes, ndim):
    """uint8 planes [1, h, w] -> YuvDic of k / 255 floats (to_tensor's division) with ndim dimensions"""
    out = YuvDic({k: _levels(p.device)[p.long()].view(*((1,) * (ndim - 2)), p.shape[-2], p.shape[-1])
                  for k, p in planes.items()})
    out.u8 = planes
    return out


def load_RGB_as_YUV420_dic(path_img, device='cuda', reader=SOURCE.png_reader, colour=SOURCE.colour, chroma_down=SOURCE.chroma_down):
    """<path_img>.png, an RGB picture -> {'y': [1,1,h,w], 'u','v': [1,1,h//2,w//2]} (src/func_util/img_processing.py:179-196):
    Pillow's 8-bit RGB -> YCbCr, chroma sample (2i, 2j) kept (nearest, scale 0.5), on the device.  A PNG of another mode
    (palette, grey, alpha) is first brought to 8-bit RGB by Pillow, as part of decoding the file.  reader 'device': the file is
    inflated on the device (aivc_amd.png.read_pictures), the same planes.  colour: an aivc_amd.color.ColourSpec -- that matrix
    and range instead of Pillow's arithmetic, chroma_down 'point' or 'box' (aivc_amd/color.py); the planes keep their sizes."""
    from .. import png
    source = Source(colour=colour, chroma_down=chroma_down)
    if png.check_reader(reader) == 'device':
        return _from_u8(_load_on_device({0: path_img}, True, device, None, source)[0], 4)
    from PIL import Image
    img = Image.open(path_img + '.png')
    if img.mode != 'RGB':
        img = img.convert('RGB')
    rgb = torch.from_numpy(np.asarray(img).copy()).to(device)
    y, u, v = _rgb_to_planes(rgb.view(1, *rgb.shape), source)
    return _from_u8({'y': y, 'u': u, 'v': v}, 4)


def load_YUV_as_dic_tensor(path_img, device='cuda', reader=SOURCE.png_reader):
    """<path_img>_{y,u,v}.png, 8-bit grey pictures -> {'y','u','v'} of 3-D tensors [1, h, w], no batch dimension
    (src/func_util/img_processing.py:199-218).  reader 'device': inflated on the device, the same planes."""
    from .. import png
    if png.check_reader(reader) == 'device':
        return _from_u8(_load_on_device({0: path_img}, False, device)[0], 3)
    from PIL import Image
    planes = {}
    for k in ('y', 'u', 'v'):
        img = Image.open(path_img + '_' + k + '.png')
        if img.mode != 'L':
            img = img.convert('L')
        a = np.asarray(img)
        planes[k] = torch.from_numpy(a.copy()).to(device).view(1, *a.shape)
    return _from_u8(planes, 3)


def _to_u8(t):
    """to_pil_image's cast of a float tensor: mul(255).byte(), a truncation.  8-bit tensors pass through."""
    return t if t.dtype == torch.uint8 else t.mul(255).byte()


def _chw(x):
    return x[0] if x.ndim == 4 else x


def _save_png(a, path_img, mode, coder=SINK.png_coder):
    """a: uint8 [h, w, 3] ('RGB') or [h, w] ('L').  coder 'device': coded where the tensor lies (aivc_amd.png.write_pictures)"""
    from .. import png
    if png.check_coder(coder) == 'device':
        png.write_pictures(a.reshape((1,) + tuple(a.shape[:2]) + (3 if mode == 'RGB' else 1,)), [path_img])
        return
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(a.cpu().numpy()), mode).save(path_img)


def save_tensor_as_img(x, path_img, mode='yuv420', coder=SINK.png_coder, colour=SINK.colour):
    """src/func_util/img_processing.py:221-287.  x holds floats in [0, 1] (cast like to_pil_image: mul(255), truncated) or uint8
    levels, on the device.
      'yuv420'        x: dict, chroma at half resolution -> nearest x 2, cropped to the luma size, YCbCr -> RGB on the device
      'yuv444'        x: dict, chroma at full resolution
      'yuv444_nodic'  x: [1,3,h,w] or [3,h,w] tensor (Y, Cb, Cr)
      'rgb'           x: [1,3,h,w] or [3,h,w] tensor; the planar -> interleaved step is a torch permute of the uint8 tensor
      'L'             x: [1,1,h,w] or [1,h,w] tensor
    Only batch entry 0 is written, as in the reference.  'yuv420' with floor-sized chroma and an odd luma size repeats the
    last chroma row / column (the reference raises there: its upsampled planes are one short).
    coder: 'pillow', or 'device' for a file coded on the device (aivc_amd/png.py): the same pixels, other bytes.
    colour: None -- Pillow's YCbCr -> RGB; an aivc_amd.color.ColourSpec -- the planes carry that matrix and range (the modes
    'yuv420', 'yuv444' and 'yuv444_nodic'; the other two hold no YCbCr, a colour with them is a ValueError)."""
    if mode in ('yuv420', 'yuv444'):
        y, u, v = (_to_u8(_chw(t)) for t in get_y_u_v(x))
        y, u, v = (t.reshape(1, t.shape[-2], t.shape[-1]) for t in (y, u, v))
        rgb = _planes_to_rgb(y, u, v, 1 if mode == 'yuv420' else 0, colour)
        _save_png(rgb[0], path_img, 'RGB', coder)
    elif mode == 'yuv444_nodic':
        p = _to_u8(_chw(x))
        rgb = _planes_to_rgb(p[0:1], p[1:2], p[2:3], 0, colour)
        _save_png(rgb[0], path_img, 'RGB', coder)
    elif mode in ('rgb', 'L') and colour is not None:
        raise ValueError('save_tensor_as_img: mode %r holds no YCbCr planes, colour %s does not apply' % (mode, colour))
    elif mode == 'rgb':
        _save_png(_to_u8(_chw(x)).permute(1, 2, 0), path_img, 'RGB', coder)
    elif mode == 'L':
        _save_png(_to_u8(_chw(x))[0], path_img, 'L', coder)
    else:
        raise ValueError('save_tensor_as_img: mode %r' % (mode,))


def save_yuv_separately(x, path_img):
    """every entry <key> of the dict x -> <path_img>_<key>.png, an 8-bit grey picture (src/func_util/img_processing.py:290-301)"""
    for key in x:
        _save_png(_to_u8(_chw(x[key]))[0], path_img + '_' + key + '.png', 'L')


def resize_frames(frames, w, h, filter=SOURCE.resample, device=None):
    """A list of 4:2:0 frames, dicts of uint8 planes {'y','u','v'} of [1, h0, w0] (device tensors, or host tensors / arrays: those
    are copied to `device`), resized to w x h on the device: y to h x w, u and v to ceil(h / 2) x ceil(w / 2), every plane on its
    own with Pillow's Image.resize arithmetic (ops.resize_u8) -- exactly what resizing each picture of a PNG triplet with Pillow
    gives.  Chroma siting is ignored, as Pillow ignores it there: a chroma plane is resized like any grey picture, its samples
    taken to sit at the centres of its own grid.  Two calls of the op for a clip, one over the y planes and one over u and v
    together.  -> a new list of dicts of [1, h', w'] uint8 device tensors (views into the two results); frames that have the
    size already come back as they are."""
    if not frames:
        return []

    def planes(k):
        got = [torch.as_tensor(fr[k]) for fr in frames]
        return [t if device is None else t.to(device) for t in got]
    hc, wc = (h + 1) // 2, (w + 1) // 2
    y, u, v = planes('y'), planes('u'), planes('v')
    if all(tuple(t.shape[-2:]) == (h, w) for t in y) and all(tuple(t.shape[-2:]) == (hc, wc) for t in u + v):
        return [{'y': a.reshape(1, h, w), 'u': b.reshape(1, hc, wc), 'v': c.reshape(1, hc, wc)} for a, b, c in zip(y, u, v)]
    ry = ops.resize_u8(y, h, w, filter)
    rc = ops.resize_u8(u + v, hc, wc, filter)
    n = len(frames)
    return [{'y': ry[i:i + 1], 'u': rc[i:i + 1], 'v': rc[n + i:n + i + 1]} for i in range(n)]


# ---- a folder of such pictures as the encoder's input -------------------------------------------------------------------
def detect_folder_layout(sequence_path):
    """-> (loading_mode, rgb, [frame indices present, ascending]) from the file names of the folder:
    <idx>_y.png -> ('old', False), <folder>_<00idx>_y.png -> ('clic', False), <idx>.png / <folder>_<00idx>.png -> rgb."""
    import re
    folder = os.path.basename(os.path.normpath(sequence_path))
    names = os.listdir(sequence_path)
    for mode, rgb, pat in (('old', False, r'(\d+)_y\.png'), ('clic', False, re.escape(folder) + r'_(\d{5,})_y\.png'),
                           ('old', True, r'(\d+)\.png'), ('clic', True, re.escape(folder) + r'_(\d{5,})\.png')):
        idx = sorted(int(m.group(1)) for m in (re.fullmatch(pat, n) for n in names) if m)
        if idx:
            return mode, rgb, idx
    raise ValueError('%s holds no <idx>_{y,u,v}.png, <folder>_<idx>_{y,u,v}.png or <idx>.png pictures' % sequence_path)
