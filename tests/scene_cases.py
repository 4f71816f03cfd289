"""The clips and expected layouts of tests/test_scene_plan.py and tests/test_gpu_scene_cut.py, each stated once.  Not a test
module.  Builders make no device tensor.

cut3 (64 x 48) and cut3_odd (33 x 47): 26 frames in three scenes,
    synthetic_video(w, h, 11, seed=3) | synthetic_video(w, h, 9, seed=5, first=40) with luma 255 - y | synthetic_video(w, h, 6, seed=9, first=200)
so the scenes open at display positions 11 and 20.  Mean absolute luma difference to the previous frame: 86.0 and 69.6 grey
levels at the cuts of cut3 and 8.3 ... 10.9 elsewhere (cut3_odd: 89.3, 71.7, at most 13.2); the peak scores are 76.0 and 59.1
against at most 1 for every other frame, far on either side of the default threshold of 10."""
import numpy as np

CUTS = [11, 20]
SIZES = {'cut3': (64, 48), 'cut3_odd': (33, 47)}
N_FRAMES = 26

# clip / configured structure -> ([unit names], [frames of the clip per unit])
LAYOUTS = {
    ('cut3', '1_GOP_8'): (['1_GOP_8', 'LDP_1', '1_GOP_8', '1_GOP_8'], [9, 2, 9, 6]),
    ('cut3', '1_GOP_4'): (['1_GOP_4', '1_GOP_4', '1_GOP_0', '1_GOP_4', '1_GOP_2', '1_GOP_0', '1_GOP_4', '1_GOP_4'],
                          [5, 5, 1, 5, 3, 1, 5, 1]),
    ('cut3_odd', '2_GOP_4'): (['2_GOP_4', 'LDP_1', '2_GOP_4', '2_GOP_4'], [9, 2, 9, 6]),
}


def host_frames(name):
    """-> list of {'y', 'u', 'v'} uint8 numpy planes"""
    from aivc_amd import synth
    w, h = SIZES[name]
    a = synth.synthetic_video(w, h, 11, seed=3)
    b = synth.synthetic_video(w, h, 9, seed=5, first=40)
    for f in b:
        f['y'] = (255 - f['y'].astype(np.int64)).astype(np.uint8)
    c = synth.synthetic_video(w, h, 6, seed=9, first=200)
    return a + b + c


def cut_free_frames(n=12, size=(64, 48)):
    from aivc_amd import synth
    return synth.synthetic_video(size[0], size[1], n, seed=3)


def pair_sad_numpy(planes):
    """the statement of aivc_pair_sad_u8: [sum |planes[i + 1] - planes[i]|] as Python integers"""
    return [int(np.abs(b.astype(np.int64) - a.astype(np.int64)).sum()) for a, b in zip(planes, planes[1:])]


def write_yuv(path, frames):
    with open(path, 'wb') as f:
        for fr in frames:
            for k in 'yuv':
                f.write(np.ascontiguousarray(fr[k]).tobytes())


def i_frames(name):
    from aivc_amd.func_util.GOP_structure import FRAME_I, generate_gop_struct
    return sum(f['type'] == FRAME_I for f in generate_gop_struct(name).values())
