/*
 * aivc_hip_warp.h -- the stand-alone warp in every sampling mode of the reference's signature (part of the C ABI of
 * libaivc_hip.so since ABI 18; conventions, types and error codes: aivc_hip.h).
 *
 * Replaces: src/func_util/optical_flow.py:14-55, warp(x, flo, interpol_mode, padding_mode, align_corners): two
 * grid_sample calls (the image, and an all-ones tensor for the validity mask), the mask's threshold and the product.
 *
 * This entry point has no `_ref` twin in the CPU oracle (the codec itself only ever warps in the mode of aivc_warp /
 * aivc_warp_blend); its semantics are pinned by tests/test_warp_modes.py against the reference's own outputs.
 */
#ifndef AIVC_HIP_WARP_H
#define AIVC_HIP_WARP_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* interpol_mode */
#define AIVC_WARP_BILINEAR 0
#define AIVC_WARP_NEAREST 1
#define AIVC_WARP_BICUBIC 2
/* padding_mode */
#define AIVC_WARP_BORDER 0
#define AIVC_WARP_ZEROS 1
#define AIVC_WARP_REFLECTION 2

/* the reference zeroes an output pixel whose mask (the sampling weights applied to ones) is below this */
#define AIVC_WARP_MASK_THRESHOLD 0.9999f

/* x [n][h][w][c], flow [n][h][w][2] (pixel units, channel 0 horizontal) -> out [n][h][w][c], fp32.
 *
 * Position (fp32, in this order; d = max(size - 1, 1) -- the reference normalises with size - 1 whatever align_corners says):
 *   g = 2 * (col + v) / d - 1
 *   p = (g + 1) * ((size - 1) / 2)           align_corners != 0
 *   p = fma(g + 1, size / 2, -0.5)           align_corners == 0: ((col + v) * size / (size - 1)) - 0.5, a slight zoom about
 *                                            the frame centre even at zero flow
 * Sampling is grid_sample's:
 *   bilinear  4 taps around floor(p), weights (1 - t) and t per direction;
 *   nearest   the tap at nearbyint(p) (half to even);
 *   bicubic   4 x 4 taps from floor(p) - 1, cubic convolution weights with A = -0.75;
 *   border      clamps p to [0, size - 1] (bicubic: each tap index instead);
 *   reflection  reflects p about 0 and size - 1 (align_corners) resp. -0.5 and size - 0.5, then clamps (bicubic: each tap index);
 *   zeros       taps outside the frame read 0.
 * Mask: the same weights applied to ones, accumulated in the same tap order -- the sum of the weights of the in-frame taps
 * under zeros, of all weights otherwise.  mask < AIVC_WARP_MASK_THRESHOLD -> every channel of the pixel is 0 (the WHOLE pixel,
 * not an attenuation: in practice every pixel whose footprint leaves the frame under zeros); otherwise out = the sample.
 *
 * (AIVC_WARP_BILINEAR, AIVC_WARP_BORDER, align_corners != 0) IS aivc_warp: the call is forwarded, any c, same bits.
 * Every other combination needs c % 4 == 0 and 16-byte aligned x and out (one thread per pixel and 4 channels).
 * AIVC_ERR_ARG for an unknown interp / pad code. */
int aivc_warp_modes(const float *x, const float *flow, int32_t n, int32_t h, int32_t w, int32_t c, int32_t interp,
                    int32_t pad, int32_t align_corners, float *out, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_WARP_H */
