// latent.hip -- the latent ops: hyper-prior parameter split, gain interpolation, and channel gain, quantisation and
// dequantisation (include/aivc_hip.h, include/aivc_hip_rates.h).
//
// The three gain ops have ONE kernel each, which takes a table of one gain row per image: grid (ceil(per / 256), n) over
// [n][per] elements, blockIdx.y is the image, one element per thread, consecutive lanes on consecutive addresses;
// element-wise and HBM-bound.  The single-gain entry points (aivc_channel_gain, aivc_quantize_center, aivc_dequantize) are
// the one-row call: n = 1, per = npix * c, the caller's [c] vector as the table.  So image i of a row call has the bits of a
// single-gain call with row i by construction; the rounding, the clamp and the NaN rule that decide the symbols are stated
// once.  Both kinds of call size their grid in rows_grid: a single-gain call of more than 0x7fffffff * 256 elements is
// AIVC_ERR_UNSUPPORTED (it used to be launched on a silently truncated grid); every other argument has the result it had.
#include "common.h"
#include "../../include/aivc_hip_rates.h"

namespace aivc {

__global__ __launch_bounds__(256) void hyper_params_kernel(const float *__restrict__ hs, int n, int hh, int wh,
                                                           int c, int h, int w, float *__restrict__ mu,
                                                           float *__restrict__ sigma) {
  const size_t gid = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t total = (size_t)n * h * w * c;
  if (gid >= total) return;
  const int ch = (int)(gid % c);
  const size_t pix = gid / c;
  const int q = (int)(pix % w), r = (int)((pix / w) % h), b = (int)(pix / ((size_t)w * h));
  const float *src = hs + (((size_t)b * hh + r) * wh + q) * 2 * c;
  mu[gid] = src[ch];
  float lv = src[c + ch];
  lv = lv < -18.4207f ? -18.4207f : lv;
  lv = lv > 10.0f ? 10.0f : lv;
  sigma[gid] = aivc_expf_det(0.5f * lv);
}

__global__ __launch_bounds__(256) void gain_interp_kernel(const float *__restrict__ g_r, const float *__restrict__ g_t,
                                                          int c, float l, float *__restrict__ out) {
  const int ch = blockIdx.x * blockDim.x + threadIdx.x;
  if (ch < c) out[ch] = aivc_gain_interp_one(g_r[ch], g_t[ch], l);
}

__global__ __launch_bounds__(256) void channel_gain_rows_kernel(const float *__restrict__ in, const float *__restrict__ gains,
                                                                size_t per, int c, float *__restrict__ out) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const size_t gid = (size_t)blockIdx.y * per + e;
  out[gid] = gains ? in[gid] * __builtin_fabsf(gains[(size_t)blockIdx.y * c + e % c]) : in[gid];
}

__global__ __launch_bounds__(256) void quantize_center_rows_kernel(const float *__restrict__ y, const float *__restrict__ mu,
                                                                   const float *__restrict__ gains, size_t per, int c,
                                                                   int16_t *__restrict__ q, float *__restrict__ y_hat) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const size_t gid = (size_t)blockIdx.y * per + e;
  const float m = mu ? mu[gid] : 0.0f;
  float r = __builtin_rintf(mu ? y[gid] - m : y[gid]);
  r = r < -256.0f ? -256.0f : (r > 256.0f ? 256.0f : r);  // the alphabet of the coder: symbols 0 .. 512
  const float level = r == r ? r : 0.0f;  // in [-256, 256]; a NaN latent: q = 0 (its y_hat stays NaN)
  if (q) q[gid] = (int16_t)level;
  if (y_hat) {
    float v = mu ? r + m : r;
    if (gains) v = v * __builtin_fabsf(gains[(size_t)blockIdx.y * c + e % c]);
    y_hat[gid] = v;
  }
}

__global__ __launch_bounds__(256) void dequantize_rows_kernel(const int16_t *__restrict__ q, const float *__restrict__ mu,
                                                              const float *__restrict__ gains, size_t per, int c,
                                                              float *__restrict__ y_hat) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= per) return;
  const size_t gid = (size_t)blockIdx.y * per + e;
  float v = mu ? (float)q[gid] + mu[gid] : (float)q[gid];
  if (gains) v = v * __builtin_fabsf(gains[(size_t)blockIdx.y * c + e % c]);
  y_hat[gid] = v;
}

// the launch grid and the elements per image; not AIVC_OK: the batch does not fit a grid
static int rows_grid(int32_t n, size_t npix, int32_t c, dim3 *grid, size_t *per) {
  if (n > 65535) return AIVC_ERR_UNSUPPORTED;  // grid.y
  *per = npix * (size_t)c;
  if (*per > (size_t)0x7fffffff * 256) return AIVC_ERR_UNSUPPORTED;  // grid.x
  *grid = dim3(cdiv(*per, 256), (unsigned)n);
  return AIVC_OK;
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_hyper_params(const float *hs, int32_t n, int32_t hh, int32_t wh, int32_t c, int32_t h, int32_t w,
                                  float *mu, float *sigma, aivc_stream_t stream) {
  if (!hs || !mu || !sigma || n <= 0 || c <= 0 || h <= 0 || w <= 0 || hh < h || wh < w) return AIVC_ERR_ARG;
  hipLaunchKernelGGL(hyper_params_kernel, dim3(cdiv((size_t)n * h * w * c, 256)), dim3(256), 0, to_stream(stream), hs,
                     n, hh, wh, c, h, w, mu, sigma);
  return check_launch("hyper_params");
}

AIVC_EXPORT int aivc_gain_interp(const float *g_r, const float *g_t, int32_t c, float l, float *out,
                                 aivc_stream_t stream) {
  if (!g_r || !g_t || !out || c <= 0) return AIVC_ERR_ARG;
  hipLaunchKernelGGL(gain_interp_kernel, dim3(cdiv(c, 256)), dim3(256), 0, to_stream(stream), g_r, g_t, c, l, out);
  return check_launch("gain_interp");
}

// a single gain: one row
AIVC_EXPORT int aivc_channel_gain(const float *in, const float *gain, size_t npix, int32_t c, float *out,
                                  aivc_stream_t stream) {
  return aivc_channel_gain_rows(in, gain, 1, npix, c, out, stream);
}

AIVC_EXPORT int aivc_quantize_center(const float *y, const float *mu, const float *gain_dec, size_t npix, int32_t c,
                                     int16_t *q, float *y_hat, aivc_stream_t stream) {
  return aivc_quantize_center_rows(y, mu, gain_dec, 1, npix, c, q, y_hat, stream);
}

AIVC_EXPORT int aivc_dequantize(const int16_t *q, const float *mu, const float *gain_dec, size_t npix, int32_t c,
                                float *y_hat, aivc_stream_t stream) {
  return aivc_dequantize_rows(q, mu, gain_dec, 1, npix, c, y_hat, stream);
}

AIVC_EXPORT int aivc_channel_gain_rows(const float *in, const float *gains, int32_t n, size_t npix, int32_t c, float *out,
                                       aivc_stream_t stream) {
  if (!in || !out || n <= 0 || c <= 0) return AIVC_ERR_ARG;
  dim3 grid;
  size_t per;
  if (int rc = rows_grid(n, npix, c, &grid, &per)) return rc;
  if (npix == 0) return AIVC_OK;
  hipLaunchKernelGGL(channel_gain_rows_kernel, grid, dim3(256), 0, to_stream(stream), in, gains, per, c, out);
  return check_launch("channel_gain_rows");
}

AIVC_EXPORT int aivc_quantize_center_rows(const float *y, const float *mu, const float *gains_dec, int32_t n, size_t npix,
                                          int32_t c, int16_t *q, float *y_hat, aivc_stream_t stream) {
  if (!y || n <= 0 || c <= 0 || (!q && !y_hat)) return AIVC_ERR_ARG;
  dim3 grid;
  size_t per;
  if (int rc = rows_grid(n, npix, c, &grid, &per)) return rc;
  if (npix == 0) return AIVC_OK;
  hipLaunchKernelGGL(quantize_center_rows_kernel, grid, dim3(256), 0, to_stream(stream), y, mu, gains_dec, per, c, q, y_hat);
  return check_launch("quantize_center_rows");
}

AIVC_EXPORT int aivc_dequantize_rows(const int16_t *q, const float *mu, const float *gains_dec, int32_t n, size_t npix,
                                     int32_t c, float *y_hat, aivc_stream_t stream) {
  if (!q || !y_hat || n <= 0 || c <= 0) return AIVC_ERR_ARG;
  dim3 grid;
  size_t per;
  if (int rc = rows_grid(n, npix, c, &grid, &per)) return rc;
  if (npix == 0) return AIVC_OK;
  hipLaunchKernelGGL(dequantize_rows_kernel, grid, dim3(256), 0, to_stream(stream), q, mu, gains_dec, per, c, y_hat);
  return check_launch("dequantize_rows");
}
