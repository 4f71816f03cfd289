// latent_rows.hip -- channel gain, quantisation and dequantisation of a batch whose images have one gain row EACH
// (include/aivc_hip_rates.h): what channel_gain_kernel / quantize_center_kernel / dequantize_kernel of pixel_ops.hip do with
// one [c] vector per launch, for the level batches of units coded at different rate indices.
//
// Element-wise, HBM-bound: grid (ceil(npix * c / 256), n), blockIdx.y is the image, one element per thread, consecutive lanes
// on consecutive addresses.  Per element the operations are those of pixel_ops.hip, in the same order.
#include "common.h"
#include "../../include/aivc_hip_rates.h"

namespace aivc {

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
