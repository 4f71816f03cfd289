// quality.hip -- per-frame statistics of the encoder's quality log (include/aivc_hip_quality.h): the exact squared error of
// 8-bit 4:2:0 planes and the sums over the motion compensation's auxiliary maps, for every frame of a level batch at once.
//
// Both are streaming reductions, HBM-bound: every input byte is read once, in 16-byte accesses where the layout allows,
// consecutive lanes on consecutive addresses; LDS is used for the workgroup's reduction only.  Neither result depends on the
// grid: the first is integer arithmetic, the second walks the fixed lanes of csrc/rate.hip.
#include "reduce.h"
#include "../../include/aivc_hip_quality.h"

namespace aivc {

constexpr int SSE_THREADS = 256;
// One pass of a plane's AIVC_SSE_BLOCKS workgroups covers 64 * 256 * 16 = 262144 bytes; a larger plane (from 512 x 513
// samples on: 1080p luma takes 8 passes) is walked with that stride.
constexpr size_t SSE_PASS_BYTES = (size_t)AIVC_SSE_BLOCKS * SSE_THREADS * 16;

__device__ __forceinline__ uint32_t sq_diff4(uint32_t a, uint32_t b) {  // sum of (a_k - b_k)^2 over the 4 bytes: <= 4 * 65025
  uint32_t s = 0;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int d = (int)((a >> (8 * k)) & 255u) - (int)((b >> (8 * k)) & 255u);
    s += (uint32_t)(d * d);
  }
  return s;
}

// grid (AIVC_SSE_BLOCKS, n * 3): workgroup (bx, f * 3 + p) leaves the sum over its share of plane p of frame f
__global__ void __launch_bounds__(SSE_THREADS) frame_sse_u8_kernel(const uint8_t *sy, const uint8_t *su, const uint8_t *sv,
                                                                   const uint8_t *ry, const uint8_t *ru, const uint8_t *rv,
                                                                   size_t size_y, size_t size_c, uint64_t *partials) {
  const int f = blockIdx.y / 3, p = blockIdx.y % 3;
  const size_t size = p == 0 ? size_y : size_c;
  const uint8_t *a = (p == 0 ? sy : (p == 1 ? su : sv)) + (size_t)f * size;
  const uint8_t *b = (p == 0 ? ry : (p == 1 ? ru : rv)) + (size_t)f * size;
  const size_t t = (size_t)blockIdx.x * SSE_THREADS + threadIdx.x, T = (size_t)AIVC_SSE_BLOCKS * SSE_THREADS;
  // planes that do not share their alignment are read byte by byte
  const ByteSplit sp(a, size, ((uintptr_t)a & 15) != ((uintptr_t)b & 15));
  uint64_t acc = 0;
  const uint4 *va = reinterpret_cast<const uint4 *>(a + sp.head), *vb = reinterpret_cast<const uint4 *>(b + sp.head);
  for (size_t i = t; i < sp.nvec; i += T) {
    const uint4 x = va[i], y = vb[i];
    acc += sq_diff4(x.x, y.x) + sq_diff4(x.y, y.y) + sq_diff4(x.z, y.z) + sq_diff4(x.w, y.w);  // <= 16 * 65025: no 32-bit overflow
  }
  sp.outside(t, T, [&](size_t j) {
    const int d = (int)a[j] - (int)b[j];
    acc += (uint32_t)(d * d);
  });
  block_partial_u64<SSE_THREADS>(acc, partials + (size_t)blockIdx.y * AIVC_SSE_BLOCKS + blockIdx.x);
}

// grid (AIVC_RATE_LANES / 256, n): lane j of frame f adds the terms of its pixels j, j + L, ... into lanes[f][0..2][j]
template <bool VEC4>  // VEC4: cs_warp == 4 and warping 16-byte aligned: one 16-byte load per pixel
__global__ void __launch_bounds__(256) frame_aux_lanes_kernel(const float *alpha, const float *beta, const float *warping,
                                                              const float *code, size_t hw, int c, int cs_warp, int cs_code,
                                                              double *lanes) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t f = blockIdx.y;
  const float *al = alpha ? alpha + f * hw : nullptr, *be = beta ? beta + f * hw : nullptr;
  const float *wp = warping ? warping + f * hw * (size_t)cs_warp : nullptr;
  const float *cd = code + f * hw * (size_t)cs_code;
  double sa = 0.0, sb = 0.0, se = 0.0;
  for (size_t p = j; p < hw; p += AIVC_RATE_LANES) {
    if (al) sa = sa + (double)al[p];
    if (be) sb = sb + (double)be[p];
    float wv[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (wp) {
      if (VEC4) {
        const float4 v = reinterpret_cast<const float4 *>(wp)[p];
        wv[0] = v.x, wv[1] = v.y, wv[2] = v.z, wv[3] = v.w;
      } else {
        for (int k = 0; k < c; ++k) wv[k] = wp[p * (size_t)cs_warp + k];
      }
    }
    for (int k = 0; k < c; ++k) {
      const double d = (double)wv[k] - (double)cd[p * (size_t)cs_code + k];
      se = se + d * d;
    }
  }
  double *out = lanes + f * 3 * AIVC_RATE_LANES;
  out[j] = sa;
  out[AIVC_RATE_LANES + j] = sb;
  out[2 * (size_t)AIVC_RATE_LANES + j] = se;
}

// grid (3, n): the fixed tree of rate_tree_kernel (reduce.h), one workgroup per sum
__global__ void __launch_bounds__(1024) frame_aux_tree_kernel(double *lanes, double ones_sum, int alpha_null, int beta_null,
                                                              double *out) {
  const size_t q = (size_t)blockIdx.y * 3 + blockIdx.x;
  double *l = lanes + q * AIVC_RATE_LANES;
  fixed_tree_sum(l);
  if (threadIdx.x == 0) {
    const bool ones = (blockIdx.x == 0 && alpha_null) || (blockIdx.x == 1 && beta_null);
    out[q] = ones ? ones_sum : l[0];
  }
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_frame_sse_u8(const uint8_t *src_y, const uint8_t *src_u, const uint8_t *src_v, const uint8_t *rec_y,
                                  const uint8_t *rec_u, const uint8_t *rec_v, int32_t n, int32_t h, int32_t w,
                                  uint64_t *partials, uint64_t *sse, aivc_stream_t stream) {
  if (n == 0) return AIVC_OK;
  if (n < 0 || h <= 0 || w <= 0 || !src_y || !src_u || !src_v || !rec_y || !rec_u || !rec_v || !partials || !sse)
    return AIVC_ERR_ARG;
  if ((size_t)n * 3 > 65535) return AIVC_ERR_UNSUPPORTED;  // grid.y
  const size_t size_y = (size_t)h * w, size_c = (size_t)((h + 1) / 2) * ((w + 1) / 2);
  hipLaunchKernelGGL(frame_sse_u8_kernel, dim3(AIVC_SSE_BLOCKS, n * 3), dim3(SSE_THREADS), 0, to_stream(stream), src_y, src_u,
                     src_v, rec_y, rec_u, rec_v, size_y, size_c, partials);
  // one wavefront per (frame, plane): the AIVC_SSE_BLOCKS partials -> sse[f][p]
  hipLaunchKernelGGL(fold_partials_u64_kernel<AIVC_SSE_BLOCKS>, dim3(n * 3), dim3(64), 0, to_stream(stream), partials, sse);
  return check_launch("frame_sse_u8");
}

AIVC_EXPORT int aivc_frame_aux_stats(const float *alpha, const float *beta, const float *warping, const float *code, int32_t n,
                                     int32_t h, int32_t w, int32_t c, int32_t cs_warp, int32_t cs_code, double *lanes,
                                     double *out, aivc_stream_t stream) {
  if (n == 0) return AIVC_OK;
  if (n < 0 || h <= 0 || w <= 0 || !code || !lanes || !out || c < 1 || c > 4 || cs_code < c || (warping && cs_warp < c))
    return AIVC_ERR_ARG;
  if (n > 65535) return AIVC_ERR_UNSUPPORTED;  // grid.y
  const size_t hw = (size_t)h * w;
  const dim3 grid(AIVC_RATE_LANES / 256, n);
  if (warping && cs_warp == 4 && ((uintptr_t)warping & 15) == 0)
    hipLaunchKernelGGL(frame_aux_lanes_kernel<true>, grid, dim3(256), 0, to_stream(stream), alpha, beta, warping, code, hw, c,
                       cs_warp, cs_code, lanes);
  else
    hipLaunchKernelGGL(frame_aux_lanes_kernel<false>, grid, dim3(256), 0, to_stream(stream), alpha, beta, warping, code, hw, c,
                       cs_warp, cs_code, lanes);
  hipLaunchKernelGGL(frame_aux_tree_kernel, dim3(3, n), dim3(1024), 0, to_stream(stream), lanes, (double)hw, alpha ? 0 : 1,
                     beta ? 0 : 1, out);
  return check_launch("frame_aux_stats");
}
