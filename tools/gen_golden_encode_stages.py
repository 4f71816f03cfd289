#!/usr/bin/env python3
"""Generate tests/golden/encode_stages.npz: what real_life.encode.encode writes for one small call with the quality log, the
digest manifest and scene cuts all on -- the bitstream, the manifest and detailed.txt, byte for byte.  Needs a GPU.

    python tools/gen_golden_encode_stages.py [--out FILE.npz]

The fixture was made ONCE, at the commit before encode() was cut into stages, and pins that the stages write what the one body
wrote (tests/test_gpu_verify.py::test_encode_stages_write_the_bytes_of_the_one_body).  Run at a later commit it states what
that commit writes: regenerate it only for a change that is meant to alter the stream, the manifest or the log.

The case (encode_case, shared with the test): the synthetic 96 x 64 clip of tests/test_gpu_verify.py, 3 frames, 1_GOP_2 -- a
unit of two frames plus a padded one -- with the default-width synthetic model of the command line.  flag_bitstream_debug is
the caller's to add: the debug digests are not part of the fixture (they are checked against the decode of the bitstream)."""
import os
import sys

sys.dont_write_bytecode = True
ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), '..')
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, 'tests', 'golden', 'encode_stages.npz')

W, H, N, GOP, NOISE, SCENE_CUT = 96, 64, 3, '1_GOP_2', 2.0, 10.0
CLIP_NAME = 'clip_%dx%d_30_420' % (W, H)


def encode_case(model, directory, **more):
    """write the clip under `directory` and encode it -> (what encode() returned, {'bitstream', 'manifest', 'detailed': paths})"""
    import numpy as np
    from aivc_amd import synth
    from aivc_amd.real_life.encode import encode
    raw = os.path.join(directory, CLIP_NAME + '.yuv')
    with open(raw, 'wb') as f:
        for fr in synth.synthetic_video(W, H, N, noise=NOISE):
            for k in 'yuv':
                f.write(np.ascontiguousarray(fr[k]).tobytes())
    bits, log_dir = os.path.join(directory, 'out', 'stream.bin'), os.path.join(directory, 'log')
    out = encode(dict({'model': model, 'sequence_path': raw, 'GOP_struct_name': GOP, 'final_file': bits, 'digests': True,
                       'working_dir': log_dir, 'scene_cut': SCENE_CUT}, **more))
    return out, {'bitstream': bits, 'manifest': bits + '.md5', 'detailed': os.path.join(log_dir, 'detailed.txt')}


def default_model(device):
    """what aivc_amd.cli_common.get_model builds when the assets are absent (same seeds, same calibration)"""
    from aivc_amd import synth
    model = synth.make_model(device=device)
    synth.calibrate_operating_point(model, device)
    return model


def main():
    import tempfile
    import numpy as np
    import torch
    path = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == '--out' else OUT
    with tempfile.TemporaryDirectory() as tmp:
        _, files = encode_case(default_model(torch.device('cuda:0')), tmp)
        np.savez_compressed(path, bitstream=np.fromfile(files['bitstream'], np.uint8),
                            manifest=np.array(open(files['manifest']).read()), detailed=np.array(open(files['detailed']).read()))
    print('wrote', path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
