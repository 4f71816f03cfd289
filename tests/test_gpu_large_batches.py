"""GPU tier: every kernel of the default path on a batch whose tensors contain byte 2^31 and byte 2^32 -- the level batches the
codec forms at 1080p with default widths (FrameCodec max_batch 16 ... 64).  The cases, their operands and the fp64 evaluation are
in tests/conv_cases.py (LARGE_CASES, large_*).  One large launch per case, read twice:

  a. windows against fp64   for the images that hold a mark (byte 2^31 / 2^32 of x, y, gate or residual), the image before each,
                            image 0 and the last: 24 x 24 output pixels in the top-left corner, against the bottom-right corner
                            and around the pixel that holds the mark, against torch in fp64 on the gathered input window (its
                            halo real pixels inside the image, the layer's own replicate padding / zero extension at a border).
                            Bound |y - ref| <= 2e-5 max(1, |ref|): what both versions of the contract are held to against fp64
                            (test_gpu_winograd.py, test_wide_golden.py); a wrapped address is an error of the output's own size.
  b. the whole output       against launches of at most 8 images (every tensor below 2^31 bytes: the sizes test_gpu_winograd.py,
                            test_gpu_gdn_resident.py and test_gpu_ops.py pin to the oracle bit for bit), torch.equal chunk by chunk.

Both the large launch and every chunk launch must take the case's variant (size rule in force: these are real sizes).

Quantities held in 32 bits, read from the kernels before the first run, and their maxima at the tested shapes (B = bytes):

  conv_wino.hip (301 / 302 / 303; n = 66)
    r_off, iss_off      uint32 B offset inside ONE image of x     301: 270*480*128*4 = 66,355,200; 302: 540*960*64*4 = 132,710,400
                                                                  (limit 0xFFFF0000, conv2d_wino_supported); 303 forms 64-bit
                                                                  per-lane addresses (iss_addr), the in-image part < 66,355,200
    iy * Wi + ix        int pixel index inside one image          518,399 (302)
    lane_b + immediates uint32 B offset inside one output ROW     472 * sx + c4 + 508 + 7 * sx < 246,000 (sx = 512)
    img_b, row_b        size_t                                    303: 66 * 540*960*64*4 = 8,758,886,400
    a.total, blk        int / uint32 entries of the block list    301: 66*17*30*2 = 67,320; 302: 67,320; 303: 66*17*30*1*4 = 134,640
    d.ubase offset      size_t                                    cb * nch * 8192 floats
    slow path ybase, o  size_t elements (not taken here: no gate, no sigmoid)
  gdn.hip (400; n = 66 x 129,600 and 34 x 518,400 pixels)
    M, m0 = tile * 64   int pixels                                17,625,600 (limit 0x7FFFFFC0, gdn_resident_supported)
    ntiles, tile + G    int                                       275,400 + 512
    d_voff              uint32 B offset inside a 64-pixel tile    < 32,768;  src = p.x + (size_t)m0 * C
    lane_b + row * ROWB uint32 B offset inside a tile             < 32,768;  yb / rsb = base + (size_t)m0 * C
  conv_thin.hip, thin_mfma_kernel (2; n = 34, 540 x 960 x 64)
    img_bytes           unsigned = descriptor num_records         132,710,400 (limit 0x7FFFFFC0, thin_mfma_ok)
    tile_off, voff      int B offset inside one image             < 132,710,400; -64 for a unit outside the image (beyond num_records)
    u_src               int element offset of a patch unit        (5 * 960 + 33) * 64 + 48
    ntiles, tile + G    int                                       30 * 135 * 34 = 137,700 + 256
    lane_out, off       int elements inside two output rows       (1920 + 1 + 2 * 28) * 6 + 5 + 2 * 19 * 6
    img, base           long: p.x + (long)n * H * W * Cin; (((long)n * h_out + 2 qy) * w_out + 2 tx0) * CO
  conv_thin.hip, thin_tconv_kernel (1; n = 18, 540 x 960 x 128)
    blockIdx.x / .y     tiles 60 * 68 = 4,080; n = 18 (grid y: at most 65,535 images)
    i, pp, q            int inside a patch of 10 * 18 pixels      5,760
    xn, pixel offsets   size_t: p.x + (size_t)n * H * W * Cin; ((size_t)iy * W + ix) * Cin; opix size_t
    (no buffer descriptor and no 32-bit offset: the kernel has no per-image limit, conv2d_thin_supported needs none)
  conv_images.hip (191; n = 34, 1080 x 1920)
    oy, oc              uint32 sample index in an 8-bit plane     34 * 1080 * 1920 = 70,502,400 (limit 0x7FFFFFFF, conv_images_supported)
    ntiles, t           uint32                                    34 * 135 * 30 = 137,700
    yb64 -> yb_hi/yb_lo 64-bit row base from a size_t product     ((b * 540 + oy) * 960 + ox0) * 64 floats: up to 4,512,153,600 B
    lane_off + imm      uint32 B offset inside 32 output pixels   (31 * 64 + 4) * 4 + 240 = 8,192
  conv_mfma_kernel.h (155 / 113 under 'fp32'; n = 34, 540 x 960 x 64)
    for_sub_batches     chunk = 0xFFFFFFF0 / 132,710,400 = 32 images (4,246,732,800 B of input per launch), then 2; in_off,
                        out_off size_t.  in_elems = 1,127,976,960 < 0xFFFFFFFF (conv2d_mfma_addressable)
    off (LDS-DMA loop)  uint32 B offset inside a SUB-BATCH of x   < 4,246,732,800 (limit 0xFFFFFFF0, LOADER_MAX_BYTES)
    out_pixel, o        size_t                                    113 writes 34 * 1080 * 1920 * 32 floats = 9,024,307,200 B

No quantity overflows at a tested shape; no kernel or *_supported limit was changed."""
import time

import numpy as np
import pytest
import torch

from conv_cases import LARGE_CASES, LARGE_CHUNK, LARGE_MARKS, LARGE_WINDOW, large_launch, large_tensors, large_window_fp64, large_windows

pytestmark = pytest.mark.gpu

FP64_BOUND = 2e-5  # |y - ref| <= FP64_BOUND * max(1, |ref|)
assert LARGE_MARKS == (1 << 31, 1 << 32)


@pytest.mark.parametrize('case', LARGE_CASES, ids=repr)
def test_large_batch_against_fp64_windows_and_small_launches(case, cuda):
    """Prints the worst |y - ref| / max(1, |ref|) over the case's fp64 windows before asserting the bound.  On an MI355X: between
    1.8e-07 (400-gdn64) and 5.31e-06 (155-conv5s2-64to128-gdn-fp32); the Winograd forms 2.58e-06 / 3.52e-06 / 1.6e-06 (EXPERIMENTS.md,
    "Large batches", has every case)."""
    from aivc_amd import ops
    c = case
    t0 = time.time()
    prev = ops.set_precision(c.precision) if c.precision else None
    d = y = chunk = None
    try:
        d = large_tensors(c, cuda, 1000 + LARGE_CASES.index(c))
        y, codes = large_launch(ops, c, d, 0, c.n)  # the ONE large launch: both comparisons read y
        assert codes == c.variants, (c, codes)
        assert tuple(y.shape) == (c.n, c.ho, c.wo, c.co)
        marks, wins = large_windows(c, d)
        assert {m[1] for m in marks} == set(LARGE_MARKS), 'the batch is sized to cross both marks'
        # a. windows against fp64
        s, worst = LARGE_WINDOW, (0.0, None)
        for img, oy0, ox0 in wins:
            ref = large_window_fp64(c, d, img, oy0, ox0)
            got = y[img, oy0:oy0 + s, ox0:ox0 + s].cpu().numpy().astype(np.float64)
            e = float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
            worst = max(worst, (e, (img, oy0, ox0)))
        print('\nlarge batch %s: %d images, marks %s, %d windows, worst fp64 error %.3g at (image, row, column) %s'
              % (c, c.n, sorted({(m[0], m[1].bit_length() - 1, m[2]) for m in marks}), len(wins), worst[0], worst[1]))
        assert worst[0] <= FP64_BOUND, (c, worst)
        # b. every byte of the output against launches of at most LARGE_CHUNK images
        for lo in range(0, c.n, LARGE_CHUNK):
            hi = min(lo + LARGE_CHUNK, c.n)
            chunk, codes = large_launch(ops, c, d, lo, hi)
            assert codes == c.variants, (c, lo, codes)
            assert torch.equal(y[lo:hi], chunk), (c, lo, hi)
        print('large batch %s: %.1f s' % (c, time.time() - t0))
    finally:
        if prev is not None:
            ops.set_precision(prev)
        del d, y, chunk
        torch.cuda.empty_cache()
