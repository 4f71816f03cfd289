"""The reference's sanity configuration as an executable check (src/sanity_script.sh:5-13, README.md:157-171):
model ms_ssim-2021cc-6, BlowingBubbles_416x240_50_420.yuv, frames 0-100, RA with --gop_size 16 --intra_period 32 must give

    PSNR    [dB]: 26.72133      MS-SSIM     : 0.93531      MS-SSIM [dB]: 11.89147      Size [bytes]: 28429

Neither the weights (git-LFS) nor the video are in the reference snapshot, so this is SKIPPED until
they appear: put them under <assets>/models/ms_ssim-2021cc-6/0_model.pt and
<assets>/raw_videos/BlowingBubbles_416x240_50_420.yuv with <assets> = $AIVC_ASSETS, the repository root or its parent.
The moment they exist the test runs the CLI end to end and holds it to the four numbers."""
import os
import re
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT

MODEL = 'ms_ssim-2021cc-6'
VIDEO = 'BlowingBubbles_416x240_50_420.yuv'
EXPECT = {'PSNR    [dB]': 26.72133, 'MS-SSIM     ': 0.93531, 'MS-SSIM [dB]': 11.89147, 'Size [bytes]': 28429}


def _assets():
    for root in (os.environ.get('AIVC_ASSETS'), ROOT, os.path.dirname(ROOT)):
        if root and os.path.isfile(os.path.join(root, 'models', MODEL, '0_model.pt')) and \
                os.path.isfile(os.path.join(root, 'raw_videos', VIDEO)):
            return root
    return None


def test_expected_numbers_are_the_readme_s():
    """(runs everywhere) the constants above are the ones the reference documents: the output block of its README
    (README.md:167-170), stored verbatim as tests/golden/sanity_expected_output.txt"""
    with open(os.path.join(GOLDEN, 'sanity_expected_output.txt')) as f:
        text = f.read()
    for k, v in EXPECT.items():
        assert re.search(re.escape(k) + r':\s*' + re.escape(('%.5f' % v) if isinstance(v, float) else str(v)), text), k


@pytest.mark.gpu
@pytest.mark.skipif(_assets() is None, reason='reference assets absent (models/%s/0_model.pt, raw_videos/%s)' % (MODEL, VIDEO))
def test_sanity_script_numbers(tmp_path):
    root = _assets()
    env = dict(os.environ, AIVC_MODELS_DIR=os.path.join(root, 'models'), PYTHONPATH=ROOT)
    out = subprocess.run([sys.executable, '-m', 'aivc_amd.aivc', '-i', os.path.join(root, 'raw_videos', VIDEO),
                          '-o', str(tmp_path / 'compressed.yuv'), '--bitstream_out', str(tmp_path / 'bitstream.bin'),
                          '--start_frame', '0', '--end_frame', '100', '--coding_config', 'RA', '--gop_size', '16',
                          '--intra_period', '32', '--model', MODEL], cwd=ROOT, env=env, capture_output=True, text=True,
                         timeout=1800)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    got = {}
    for k in EXPECT:
        m = re.search(re.escape(k) + r':\s*([0-9.]+)', out.stdout)
        assert m, (k, out.stdout[-2000:])
        got[k] = float(m.group(1))
    # the size is the bit-exactness check (identical latents and coder); quality to the digits the README prints
    assert int(got['Size [bytes]']) == EXPECT['Size [bytes]'], got
    assert abs(got['PSNR    [dB]'] - EXPECT['PSNR    [dB]']) < 5e-4, got
    assert abs(got['MS-SSIM     '] - EXPECT['MS-SSIM     ']) < 5e-5, got
    assert abs(got['MS-SSIM [dB]'] - EXPECT['MS-SSIM [dB]']) < 5e-4, got
