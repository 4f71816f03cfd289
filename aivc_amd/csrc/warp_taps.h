// warp_taps.h -- per-pixel arithmetic of warp_modes_kernel (pixel_ops.hip): sample position, tap indices, weights and the
// mask of one output pixel, in fp32 and in the operation order of torch's CPU grid_sample, which produced the fixtures
// (tests/golden/warp_modes.npz).
// Compiled with -ffp-contract=off: every fused multiply-add is written out.
#pragma once
#include "../../include/aivc_hip_warp.h"

namespace aivc {

constexpr float WARP_CUBIC_A = -0.75f;

// taps per direction
template <int INTERP> struct WarpFootprint { static constexpr int N = INTERP == AIVC_WARP_BICUBIC ? 4 : (INTERP == AIVC_WARP_BILINEAR ? 2 : 1); };

// the reference's normalisation (with size - 1 whatever align_corners says) followed by grid_sample's unnormalisation
__device__ __forceinline__ float warp_modes_position(float pos, int size, bool align_corners) {
  const int d = size - 1 > 1 ? size - 1 : 1;
  const float g = 2.0f * pos / (float)d - 1.0f;
  if (align_corners) return (g + 1.0f) * ((float)(size - 1) * 0.5f);
  return __builtin_fmaf(g + 1.0f, (float)size * 0.5f, -0.5f);
}

// padding of a coordinate (bilinear / nearest: the position; bicubic: a tap index as a float).  zeros leaves it alone.
template <int PAD>
__device__ __forceinline__ float warp_modes_pad(float p, int size, bool align_corners) {
  if (PAD == AIVC_WARP_ZEROS) return p;
  if (PAD == AIVC_WARP_REFLECTION) {
    const float lo = align_corners ? 0.0f : -0.5f;
    const float twice_span = align_corners ? (float)(2 * (size - 1)) : (float)(2 * size);
    if (twice_span == 0.0f) {
      p = 0.0f;
    } else {
      const float a = __builtin_fabsf(p - lo);
      const float extra = a - __builtin_truncf(a / twice_span) * twice_span;
      const float back = twice_span - extra;
      p = (extra < back ? extra : back) + lo;
    }
  }
  p = p > 0.0f ? p : 0.0f;  // (a NaN ends at 0)
  const float hi = (float)(size - 1);
  return p < hi ? p : hi;
}

// float coordinate that is a whole number -> index, or -1 when it is outside [0, size).  Border and reflection have
// already brought it inside; the integer clamp only keeps a NaN / infinite flow from ever forming an outside address.
template <int PAD>
__device__ __forceinline__ int warp_modes_index(float f, int size) {
  if (PAD == AIVC_WARP_ZEROS) return (f >= 0.0f && f <= (float)(size - 1)) ? (int)f : -1;
  int i = (int)f;
  i = i > 0 ? i : 0;
  return i < size - 1 ? i : size - 1;
}

__device__ __forceinline__ float warp_cubic_inner(float u) { return ((WARP_CUBIC_A + 2.0f) * u - (WARP_CUBIC_A + 3.0f)) * u * u + 1.0f; }
__device__ __forceinline__ float warp_cubic_outer(float u) {
  return ((WARP_CUBIC_A * u - 5.0f * WARP_CUBIC_A) * u + 8.0f * WARP_CUBIC_A) * u - 4.0f * WARP_CUBIC_A;
}

// one direction of one pixel: N tap indices (-1: reads 0) and their weights
template <int N> struct WarpAxis {
  int idx[N];
  float wgt[N];
};

template <int INTERP, int PAD>
__device__ __forceinline__ WarpAxis<WarpFootprint<INTERP>::N> warp_modes_axis(float pos, int size, bool align_corners) {
  WarpAxis<WarpFootprint<INTERP>::N> a;
  float p = warp_modes_position(pos, size, align_corners);
  if (INTERP == AIVC_WARP_NEAREST) {
    p = warp_modes_pad<PAD>(p, size, align_corners);
    a.idx[0] = warp_modes_index<PAD>(__builtin_nearbyintf(p), size);
    a.wgt[0] = 1.0f;
  } else if (INTERP == AIVC_WARP_BILINEAR) {
    p = warp_modes_pad<PAD>(p, size, align_corners);
    const float p0 = __builtin_floorf(p);
    const float t = p - p0;
    a.idx[0] = warp_modes_index<AIVC_WARP_ZEROS>(p0, size);  // (at p = size - 1 the second tap is outside, with weight 0)
    a.idx[1 % WarpFootprint<INTERP>::N] = warp_modes_index<AIVC_WARP_ZEROS>(p0 + 1.0f, size);
    a.wgt[0] = 1.0f - t;
    a.wgt[1 % WarpFootprint<INTERP>::N] = t;
  } else {
    const float p0 = __builtin_floorf(p);
    const float t = p - p0;
    const float u = 1.0f - t;
    const float wgt[4] = {warp_cubic_outer(t + 1.0f), warp_cubic_inner(t), warp_cubic_inner(u), warp_cubic_outer(u + 1.0f)};
    for (int k = 0; k < WarpFootprint<INTERP>::N; ++k) {
      a.idx[k] = warp_modes_index<PAD>(warp_modes_pad<PAD>(p0 - 1.0f + (float)k, size, align_corners), size);
      a.wgt[k] = wgt[k];
    }
  }
  return a;
}

// Everything of one output pixel that does not depend on the channel: pixel offsets of the N x N taps (row-major, -1:
// reads 0), the weights, and whether the mask keeps the pixel.
template <int INTERP> struct WarpModesTaps {
  static constexpr int N = WarpFootprint<INTERP>::N;
  int off[N * N];
  float wx[N], wy[N];  // bicubic: the two directions' weights (applied row by row); nearest: unused
  float w2[N * N];     // bilinear: the four products nw, ne, sw, se
  bool keep;
};

// Weighted sum of the taps' values in torch's order: bilinear  nw * a + ne * b + sw * c + se * d  with the PRODUCT weights;
// bicubic  each row  cx0 * v0 + cx1 * v1 + cx2 * v2 + cx3 * v3, then the rows with cy likewise; nearest the value itself.
// Every term after the first is ONE fused multiply-add, as torch's CPU kernel contracts them: with that the bilinear modes
// reproduce the fixtures' outputs and masks bit for bit (bicubic: to a few units in the last place, its coefficients round
// differently there).  val(k) returns the value of tap k (0 when it is outside).
template <int INTERP, typename F>
__device__ __forceinline__ float warp_modes_sum(const WarpModesTaps<INTERP> &t, F val) {
  constexpr int N = WarpFootprint<INTERP>::N;
  if (INTERP == AIVC_WARP_NEAREST) return val(0);
  if (INTERP == AIVC_WARP_BILINEAR) {
    float r = val(0) * t.w2[0];
    for (int k = 1; k < N * N; ++k) r = __builtin_fmaf(val(k), t.w2[k], r);
    return r;
  }
  float out = 0.0f;
  for (int i = 0; i < N; ++i) {
    float row = t.wx[0] * val(i * N);
    for (int j = 1; j < N; ++j) row = __builtin_fmaf(t.wx[j], val(i * N + j), row);
    out = i == 0 ? t.wy[0] * row : __builtin_fmaf(t.wy[i], row, out);
  }
  return out;
}

template <int INTERP, int PAD>
__device__ __forceinline__ WarpModesTaps<INTERP> warp_modes_taps(int h, int w, float fx, float fy, int row, int col, bool align_corners) {
  constexpr int N = WarpFootprint<INTERP>::N;
  const auto ax = warp_modes_axis<INTERP, PAD>((float)col + fx, w, align_corners);
  const auto ay = warp_modes_axis<INTERP, PAD>((float)row + fy, h, align_corners);
  WarpModesTaps<INTERP> t;
  for (int i = 0; i < N; ++i) {
    t.wx[i] = ax.wgt[i];
    t.wy[i] = ay.wgt[i];
    for (int j = 0; j < N; ++j) {
      t.off[i * N + j] = (ay.idx[i] >= 0 && ax.idx[j] >= 0) ? ay.idx[i] * w + ax.idx[j] : -1;
      t.w2[i * N + j] = ax.wgt[j] * ay.wgt[i];
    }
  }
  const float mask = warp_modes_sum<INTERP>(t, [&](int k) { return t.off[k] >= 0 ? 1.0f : 0.0f; });
  t.keep = !(mask < AIVC_WARP_MASK_THRESHOLD);
  return t;
}

}  // namespace aivc
