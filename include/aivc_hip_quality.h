/*
 * aivc_hip_quality.h -- per-frame statistics of the encoder's quality log (part of the C ABI of libaivc_hip.so since ABI 20;
 * conventions, types and error codes: aivc_hip.h).
 *
 * Replaces: src/model_mngt/loss_function.py:194,203-205,239-240,415-435 (MSELoss over the three planes of a frame, the
 * warping error, the means of the alpha and beta maps: torch fp32 expressions over one frame at a time) -- for every frame of
 * a level batch in one call each, on what the codec already holds: the 8-bit planes and the auxiliary outputs of the motion
 * compensation.  Nothing is converted or materialised.  MS-SSIM stays on aivc_ssim_means / aivc_pool2x2 (aivc_hip.h).
 *
 * Both results are independent of the launch grid: the first is integer arithmetic, the second adds in a fixed order.
 * These entry points have no `_ref` twin in the CPU oracle; their CPU statement is numpy (tests/test_gpu_quality_stats.py).
 */
#ifndef AIVC_HIP_QUALITY_H
#define AIVC_HIP_QUALITY_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups per plane of aivc_frame_sse_u8, and the 64-bit words of scratch it needs for n frames */
#define AIVC_SSE_BLOCKS 64
#define AIVC_SSE_SCRATCH_WORDS(n) ((size_t)(n) * 3 * AIVC_SSE_BLOCKS)

/* Exact sum of squared differences of n frames of 8-bit 4:2:0 planes, per frame and plane:
 *   sse[f][p] = sum over the plane of (a - b)^2,   p = 0, 1, 2 for y, u, v.
 * src_* / rec_*: the planes of the n frames stacked per plane, y [n][h][w], u and v [n][ceil(h/2)][ceil(w/2)].
 * partials: AIVC_SSE_SCRATCH_WORDS(n) uint64 of scratch; sse: [n][3] uint64.
 * Integer arithmetic throughout (a term is at most 255^2, a plane of 2^47 samples cannot overflow the 64-bit sums): the
 * result does not depend on the order of the additions, hence not on the grid, the GPU or the number of ranks.
 * Two launches: AIVC_SSE_BLOCKS workgroups per (frame, plane) leave one partial each, then one wavefront per (frame, plane)
 * adds them.  16-byte loads wherever the two planes of a pair share their alignment (bytes in front of the first 16-byte
 * boundary and behind the last are read one by one), single bytes otherwise. */
int aivc_frame_sse_u8(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, const uint8_t *rec_y,
                      const uint8_t *rec_u, const uint8_t *rec_v, int32_t n, int32_t h, int32_t w, uint64_t *partials,
                      uint64_t *sse, aivc_stream_t stream);

/* Sums over the auxiliary outputs of a batch of n frames, as FrameCodec.encode_batch(want_aux=True) holds them:
 *   alpha, beta   [n][h][w] fp32 (aivc_warp_blend_rows)
 *   warping       [n][h][w][cs_warp] fp32, the first c channels used (the motion-compensated prediction x_warp)
 *   code          [n][h][w][cs_code] fp32, the first c channels used (the frame to code as 4:4:4, aivc_yuv420u8_to_444)
 *   out[f] = { sum alpha, sum beta, sum over pixels and the c used channels of (warping - code)^2 },   double [n][3].
 * 1 <= c <= 4, c <= cs_warp, c <= cs_code.  The buffers hold cs_* floats for EVERY pixel, the last one included: with
 * cs_warp == 4 and a 16-byte aligned pointer a pixel of warping is read as one 16-byte access.
 * NULL alpha / beta / warping: what an I frame reports (it has no motion compensation): alpha and beta are maps of ones
 * (both sums are h * w), warping is a map of zeros (the third sum is the sum of code^2).
 * Arithmetic: every value is widened to fp64 first; a term of the third sum is d * d with d = warping - code, both in fp64.
 * Per frame and sum, lane j of AIVC_RATE_LANES adds the terms of its pixels p = j, j + L, j + 2L, ... in that order (inside
 * a pixel: channel 0, 1, ..., c - 1), starting from +0.0; then lanes[j] += lanes[j + s] for s = L/2, L/4, ..., 1 -- the
 * lane-then-tree order of aivc_bounds_rate, so the bits depend neither on the grid nor on how the frames are batched.
 * lanes: n * 3 * AIVC_RATE_LANES doubles of scratch.  Two launches. */
int aivc_frame_aux_stats(const float *alpha, const float *beta, const float *warping, const float *code, int32_t n,
                         int32_t h, int32_t w, int32_t c, int32_t cs_warp, int32_t cs_code, double *lanes, double *out,
                         aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_QUALITY_H */
