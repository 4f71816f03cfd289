#!/usr/bin/env python3
"""Generate tests/golden/img_processing.npz by RUNNING the reference's own func_util/img_processing.py on the CPU.

Runs only where the reference is present; the test-suite uses the committed fixture.  Nothing from the reference is
copied: the fixture holds seeded random pictures, the tensors the reference's load_frames returns for folders made of them
and the pixels of the PNG files its save_tensor_as_img / save_yuv_separately write for seeded random tensors.

torchvision is absent here.  The reference takes two helpers from it, stated below as torchvision documents them:
to_tensor (HWC uint8 picture -> CHW float32, divided by 255) and to_pil_image (CHW float tensor -> mul(255).byte() ->
HWC picture of the given mode).

    python tools/gen_golden_img.py            # rewrites tests/golden/img_processing.npz
"""
import os
import sys
import tempfile
import types

sys.dont_write_bytecode = True

import numpy as np
import torch
from PIL import Image

REF = '/root/reference/src'
OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tests', 'golden', 'img_processing.npz')

# the cases, shared with tests/test_gpu_img_processing.py through the fixture itself
N_FRAMES, H, W = 5, 21, 34            # odd height: floor-sized chroma (10 x 17) from RGB, ceil-sized (11 x 17) in the triplets
FIRST, NB_LOAD, NB_PAD = 1, 5, 2      # frames 1, 2, 3 are read, frame_3 and frame_4 repeat picture 3
CLIC_NAME = 'clip_a'


def install_stubs():
    def to_tensor(img):
        a = np.asarray(img)
        a = a[:, :, None] if a.ndim == 2 else a
        return torch.from_numpy(a.copy()).permute(2, 0, 1).contiguous().to(torch.float32).div(255)

    def to_pil_image(x, mode=None):
        if x.is_floating_point():
            x = x.mul(255).byte()
        a = x.permute(1, 2, 0).numpy()
        return Image.fromarray(np.ascontiguousarray(a[:, :, 0] if a.shape[2] == 1 else a), mode)
    tv = types.ModuleType('torchvision')
    tvt = types.ModuleType('torchvision.transforms')
    tvf = types.ModuleType('torchvision.transforms.functional')
    tvf.to_tensor, tvf.to_pil_image = to_tensor, to_pil_image
    tv.transforms, tvt.functional = tvt, tvf
    sys.modules.update({'torchvision': tv, 'torchvision.transforms': tvt, 'torchvision.transforms.functional': tvf})


def write_folders(root, rgb, y, u, v):
    """the three layouts of the same clip under root -> {'old': path, 'clic': path, 'rgb': path}"""
    paths = {k: os.path.join(root, CLIC_NAME if k == 'clic' else k) for k in ('old', 'clic', 'rgb')}
    for p in paths.values():
        os.makedirs(p)
    for i in range(len(rgb)):
        Image.fromarray(rgb[i], 'RGB').save(os.path.join(paths['rgb'], '%d.png' % i))
        for k, plane in (('y', y), ('u', u), ('v', v)):
            Image.fromarray(plane[i], 'L').save(os.path.join(paths['old'], '%d_%s.png' % (i, k)))
            Image.fromarray(plane[i], 'L').save(os.path.join(paths['clic'], '%s_%05d_%s.png' % (CLIC_NAME, i, k)))
    return paths


def main():
    install_stubs()
    sys.path.insert(0, REF)
    from func_util import img_processing as ref
    rng = np.random.default_rng(20211)
    out = {'first': FIRST, 'nb_load': NB_LOAD, 'nb_pad': NB_PAD}
    rgb = rng.integers(0, 256, (N_FRAMES, H, W, 3), dtype=np.uint8)
    y = rng.integers(0, 256, (N_FRAMES, H, W), dtype=np.uint8)
    u = rng.integers(0, 256, (N_FRAMES, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8)
    v = rng.integers(0, 256, (N_FRAMES, (H + 1) // 2, (W + 1) // 2), dtype=np.uint8)
    out.update(in_rgb=rgb, in_y=y, in_u=u, in_v=v)
    with tempfile.TemporaryDirectory() as root:
        paths = write_folders(root, rgb, y, u, v)
        for layout in ('old', 'clic', 'rgb'):
            frames = ref.load_frames({'sequence_path': paths[layout], 'idx_starting_frame': FIRST, 'nb_frame_to_load': NB_LOAD,
                                      'nb_pad_frame': NB_PAD, 'rgb': layout == 'rgb', 'loading_mode': 'old' if layout == 'rgb' else layout})
            out['load_%s_names' % layout] = np.array(list(frames))
            for name, fr in frames.items():
                for c in 'yuv':
                    out['load_%s_%s_%s' % (layout, name, c)] = fr[c].numpy()
        # save_tensor_as_img: floats that are NOT k / 255, so that the truncation of to_pil_image shows
        g = torch.Generator().manual_seed(7)
        cases = {
            'yuv420': {'y': torch.rand(1, 1, H, W - 1, generator=g), 'u': torch.rand(1, 1, (H + 1) // 2, W // 2, generator=g),
                       'v': torch.rand(1, 1, (H + 1) // 2, W // 2, generator=g)},  # (ceil-sized chroma: 22 rows, cropped to 21)
            'yuv444': {'y': torch.rand(1, 1, H, W, generator=g), 'u': torch.rand(1, 1, H, W, generator=g),
                       'v': torch.rand(1, 1, H, W, generator=g)},
            'rgb': torch.rand(1, 3, H, W, generator=g),
            'yuv444_nodic': torch.rand(3, H, W, generator=g),
            'L': torch.rand(1, 1, H, W, generator=g),
        }
        for mode, x in cases.items():
            if isinstance(x, dict):
                x['y'][0, 0, 0, :4] = torch.tensor([0.0, 1.0, 254.999 / 255, 1 / 255])
                for c in 'yuv':
                    out['save_%s_in_%s' % (mode, c)] = x[c].numpy()
            else:
                out['save_%s_in' % mode] = x.numpy()
            path = os.path.join(root, 'saved_%s.png' % mode)
            ref.save_tensor_as_img(x, path, mode=mode)
            out['save_%s_png' % mode] = np.asarray(Image.open(path))
        sep = {k: t.clone() for k, t in cases['yuv420'].items()}
        ref.save_yuv_separately(sep, os.path.join(root, 'sep'))
        for c in 'yuv':
            out['sep_png_%s' % c] = np.asarray(Image.open(os.path.join(root, 'sep_%s.png' % c)))
    np.savez_compressed(OUT, **out)
    print('wrote %s (%d bytes, %d arrays)' % (OUT, os.path.getsize(OUT), len(out)))


if __name__ == '__main__':
    main()
