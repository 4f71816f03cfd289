/*
 * aivc_hip_rates.h -- the latent gain / quantisation stages with ONE GAIN ROW PER IMAGE of the batch (part of the C ABI of
 * libaivc_hip.so since ABI 21; conventions, types and error codes: aivc_hip.h).
 *
 * The codec pushes the frames of a dependency level of ALL intra-period units through the networks as one batch.  When the
 * units are coded at different rate indices (FrameCodec.encode_units(idx_rate=[...]), aivc_amd/rate_control.py), the images
 * of a batch have different gain vectors; aivc_channel_gain / aivc_quantize_center / aivc_dequantize (aivc_hip.h) take one
 * [c] vector per call.  These three take a table instead:
 *
 *   tensors  [n][npix][c]   (n images of npix positions, channels innermost)
 *   gains    [n][c]         image i uses row i
 *
 * Their kernels (csrc/latent.hip) are the only kernels of the three ops: a single-gain entry point is the one-row call
 * (n = 1, npix * c elements in the one image, the [c] vector as the table).  So per element there is one statement of the
 * arithmetic (fabsf of the gain inside the kernel, rintf, the clamp to the coder's alphabet, (r + mu) * |g|), and image i
 * comes out with the bits the single-gain entry point gives for that image alone with row i by construction
 * (tests/test_gpu_latent_rows.py).  The same pointers may be NULL, with the same meaning.  The image is a coordinate of the
 * grid (blockIdx.y, like the batch entropy kernels): n > 65535, or more than 0x7fffffff * 256 elements per image, is
 * AIVC_ERR_UNSUPPORTED; n <= 0, c <= 0 or a NULL required pointer is AIVC_ERR_ARG; npix == 0 is AIVC_OK (nothing to do).
 * Element-wise and HBM-bound: every element is read and written once, consecutive lanes on consecutive addresses.
 *
 * The rows are built by the caller: GainMatrix.gain_rows stacks what GainMatrix.gain_vector gives for every distinct rate of
 * the batch (aivc_gain_interp for a fractional one), so a fractional rate has the bits of the single-rate path.
 * These entry points have no `_ref` twin in the CPU oracle; the single-gain entry points, which run the same kernels, have one.
 */
#ifndef AIVC_HIP_RATES_H
#define AIVC_HIP_RATES_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* out[i][p][ch] = in[i][p][ch] * fabsf(gains[i][ch]).  gains may be NULL (copy). */
int aivc_channel_gain_rows(const float *in, const float *gains, int32_t n, size_t npix, int32_t c, float *out,
                           aivc_stream_t stream);

/* Encoder side: q = clamp(rint(y - mu), -256, 256) (half-to-even); y_hat = (q + mu) * |gains_dec[i]|.
 * mu == NULL means mu = 0; gains_dec == NULL means gain 1.  q (int16) and y_hat may each be NULL, not both. */
int aivc_quantize_center_rows(const float *y, const float *mu, const float *gains_dec, int32_t n, size_t npix, int32_t c,
                              int16_t *q, float *y_hat, aivc_stream_t stream);

/* Decoder side: y_hat = ((float)q + mu) * |gains_dec[i]|. */
int aivc_dequantize_rows(const int16_t *q, const float *mu, const float *gains_dec, int32_t n, size_t npix, int32_t c,
                         float *y_hat, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_RATES_H */
