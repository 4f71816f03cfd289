// color.hip -- 8-bit RGB <-> YCbCr of the PNG frame I/O (include/aivc_hip_color.h): Pillow's JFIF tables, integer only.
//
// HBM-bound: 3 B in and 1.5 B out per pixel forward, the reverse backward.  The tables (7 x 256 and 4 x 256 int16) are
// copied into LDS once per workgroup; every lookup is a 2-byte LDS read.  The vector kernels give a thread 16 consecutive
// pixels of a row (48 bytes of RGB = three 16-byte accesses, 16 bytes of Y); the scalar kernels cover every other
// width / alignment.
#define AIVC_COLOR_TABLE __attribute__((aligned(16))) static __device__ const  // (copied to LDS 16 bytes at a time)
#include "color_tables.h"
#include "common.h"
#include "../../include/aivc_hip_color.h"

namespace aivc {

constexpr int COLOR_THREADS = 256;

template <int TABLES>
__device__ __forceinline__ void tables_to_lds(int16_t *lds, const int16_t (*src)[256]) {
  const uint4 *s = reinterpret_cast<const uint4 *>(&src[0][0]);
  uint4 *d = reinterpret_cast<uint4 *>(lds);
  for (int i = threadIdx.x; i < TABLES * 256 / 8; i += COLOR_THREADS) d[i] = s[i];
  __syncthreads();
}

__device__ __forceinline__ int fwd_y(const int16_t *t, int r, int g, int b) {
  return (t[AIVC_COLOR_Y_R * 256 + r] + t[AIVC_COLOR_Y_G * 256 + g] + t[AIVC_COLOR_Y_B * 256 + b]) >> 6;
}
__device__ __forceinline__ int fwd_cb(const int16_t *t, int r, int g, int b) {
  return ((t[AIVC_COLOR_CB_R * 256 + r] + t[AIVC_COLOR_CB_G * 256 + g] + (b << 5)) >> 6) + 128;
}
__device__ __forceinline__ int fwd_cr(const int16_t *t, int r, int g, int b) {
  return (((r << 5) + t[AIVC_COLOR_CR_G * 256 + g] + t[AIVC_COLOR_CR_B * 256 + b]) >> 6) + 128;
}
__device__ __forceinline__ int clamp8(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }
__device__ __forceinline__ void inv_rgb(const int16_t *t, int y, int cb, int cr, int &r, int &g, int &b) {
  r = clamp8(y + (t[AIVC_COLOR_R_CR * 256 + cr] >> 6));
  g = clamp8(y + ((t[AIVC_COLOR_G_CB * 256 + cb] + t[AIVC_COLOR_G_CR * 256 + cr]) >> 6));
  b = clamp8(y + (t[AIVC_COLOR_B_CB * 256 + cb] >> 6));
}
// byte k of an array of little-endian words (k is a compile-time constant wherever this is used)
__device__ __forceinline__ int byte_of(const uint32_t *wd, int k) { return (wd[k >> 2] >> ((k & 3) * 8)) & 255u; }

// ---- RGB -> 4:2:0 ------------------------------------------------------------------------------------------------------
// one thread: rows 2 rp and 2 rp + 1, columns 16 g .. 16 g + 15.  w % 16 == 0; rgb, y 16-byte and u, v 8-byte aligned.
__global__ __launch_bounds__(COLOR_THREADS) void rgb8_to_yuv420u8_vec_kernel(const uint8_t *__restrict__ rgb, int n, int h, int w,
                                                                             uint8_t *__restrict__ yo, uint8_t *__restrict__ uo,
                                                                             uint8_t *__restrict__ vo) {
  __shared__ __attribute__((aligned(16))) int16_t t[AIVC_COLOR_FWD_TABLES * 256];
  tables_to_lds<AIVC_COLOR_FWD_TABLES>(t, AIVC_COLOR_FWD);
  const int groups = w >> 4, hp = (h + 1) >> 1, ch = h >> 1, cw = w >> 1;
  const size_t gid = (size_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (gid >= (size_t)n * hp * groups) return;
  const int g = (int)(gid % groups);
  const int rp = (int)((gid / groups) % hp);
  const size_t img = gid / groups / hp;
#pragma unroll
  for (int row = 0; row < 2; ++row) {
    const int yy = 2 * rp + row;
    if (yy >= h) break;
    const size_t pix = (img * h + yy) * (size_t)w + 16 * g;
    const uint4 *src = reinterpret_cast<const uint4 *>(rgb + pix * 3);
    uint32_t in[12];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const uint4 x = src[q];
      in[4 * q] = x.x, in[4 * q + 1] = x.y, in[4 * q + 2] = x.z, in[4 * q + 3] = x.w;
    }
    uint32_t lum[4] = {0, 0, 0, 0}, cb[2] = {0, 0}, cr[2] = {0, 0};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int r = byte_of(in, 3 * p), gg = byte_of(in, 3 * p + 1), b = byte_of(in, 3 * p + 2);
      lum[p >> 2] |= (uint32_t)fwd_y(t, r, gg, b) << ((p & 3) * 8);
      if (row == 0 && (p & 1) == 0) {
        cb[p >> 3] |= (uint32_t)fwd_cb(t, r, gg, b) << (((p >> 1) & 3) * 8);
        cr[p >> 3] |= (uint32_t)fwd_cr(t, r, gg, b) << (((p >> 1) & 3) * 8);
      }
    }
    *reinterpret_cast<uint4 *>(yo + pix) = make_uint4(lum[0], lum[1], lum[2], lum[3]);
    if (row == 0 && rp < ch) {
      const size_t cpix = (img * ch + rp) * (size_t)cw + 8 * g;
      *reinterpret_cast<uint2 *>(uo + cpix) = make_uint2(cb[0], cb[1]);
      *reinterpret_cast<uint2 *>(vo + cpix) = make_uint2(cr[0], cr[1]);
    }
  }
}

// one thread: the 2 x 2 block at (2 by, 2 bx), what of it lies inside the frame.  Any size and alignment.
__global__ __launch_bounds__(COLOR_THREADS) void rgb8_to_yuv420u8_kernel(const uint8_t *__restrict__ rgb, int n, int h, int w,
                                                                         uint8_t *__restrict__ yo, uint8_t *__restrict__ uo,
                                                                         uint8_t *__restrict__ vo) {
  __shared__ __attribute__((aligned(16))) int16_t t[AIVC_COLOR_FWD_TABLES * 256];
  tables_to_lds<AIVC_COLOR_FWD_TABLES>(t, AIVC_COLOR_FWD);
  const int hp = (h + 1) >> 1, wp = (w + 1) >> 1, ch = h >> 1, cw = w >> 1;
  const size_t gid = (size_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (gid >= (size_t)n * hp * wp) return;
  const int bx = (int)(gid % wp);
  const int by = (int)((gid / wp) % hp);
  const size_t img = gid / wp / hp;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = 2 * by + dy, xx = 2 * bx + dx;
      if (yy >= h || xx >= w) continue;
      const size_t pix = (img * h + yy) * (size_t)w + xx;
      const int r = rgb[pix * 3], g = rgb[pix * 3 + 1], b = rgb[pix * 3 + 2];
      yo[pix] = (uint8_t)fwd_y(t, r, g, b);
      if (dy == 0 && dx == 0 && by < ch && bx < cw) {
        const size_t cpix = (img * ch + by) * (size_t)cw + bx;
        uo[cpix] = (uint8_t)fwd_cb(t, r, g, b);
        vo[cpix] = (uint8_t)fwd_cr(t, r, g, b);
      }
    }
  }
}

// ---- planar YCbCr -> RGB -------------------------------------------------------------------------------------------------
// one thread: 16 consecutive pixels of one row.  w % 16 == 0, cw == w >> SHIFT exactly; y, rgb 16-byte aligned, u, v aligned to
// their 16 >> SHIFT bytes.
template <int SHIFT>
__global__ __launch_bounds__(COLOR_THREADS) void yuv8_to_rgb8_vec_kernel(const uint8_t *__restrict__ yi, const uint8_t *__restrict__ ui,
                                                                         const uint8_t *__restrict__ vi, int n, int h, int w, int ch,
                                                                         int cw, uint8_t *__restrict__ rgb) {
  __shared__ __attribute__((aligned(16))) int16_t t[AIVC_COLOR_INV_TABLES * 256];
  tables_to_lds<AIVC_COLOR_INV_TABLES>(t, AIVC_COLOR_INV);
  const int groups = w >> 4;
  const size_t gid = (size_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (gid >= (size_t)n * h * groups) return;
  const int g = (int)(gid % groups);
  const int yy = (int)((gid / groups) % h);
  const size_t img = gid / groups / h;
  const size_t pix = (img * h + yy) * (size_t)w + 16 * g;
  const int cy = min(yy >> SHIFT, ch - 1);
  const size_t cpix = (img * ch + cy) * (size_t)cw + ((16 * g) >> SHIFT);
  uint32_t lum[4], cb[4], cr[4];
  {
    const uint4 x = *reinterpret_cast<const uint4 *>(yi + pix);
    lum[0] = x.x, lum[1] = x.y, lum[2] = x.z, lum[3] = x.w;
  }
  if (SHIFT == 0) {
    const uint4 a = *reinterpret_cast<const uint4 *>(ui + cpix), b = *reinterpret_cast<const uint4 *>(vi + cpix);
    cb[0] = a.x, cb[1] = a.y, cb[2] = a.z, cb[3] = a.w;
    cr[0] = b.x, cr[1] = b.y, cr[2] = b.z, cr[3] = b.w;
  } else {
    const uint2 a = *reinterpret_cast<const uint2 *>(ui + cpix), b = *reinterpret_cast<const uint2 *>(vi + cpix);
    cb[0] = a.x, cb[1] = a.y, cb[2] = cb[3] = 0;
    cr[0] = b.x, cr[1] = b.y, cr[2] = cr[3] = 0;
  }
  uint32_t out[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    int r, gg, b;
    inv_rgb(t, byte_of(lum, p), byte_of(cb, p >> SHIFT), byte_of(cr, p >> SHIFT), r, gg, b);
    out[(3 * p) >> 2] |= (uint32_t)r << (((3 * p) & 3) * 8);
    out[(3 * p + 1) >> 2] |= (uint32_t)gg << (((3 * p + 1) & 3) * 8);
    out[(3 * p + 2) >> 2] |= (uint32_t)b << (((3 * p + 2) & 3) * 8);
  }
  uint4 *dst = reinterpret_cast<uint4 *>(rgb + pix * 3);
#pragma unroll
  for (int q = 0; q < 3; ++q) dst[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}

// one thread per pixel.  Any size and alignment; chroma indices clamp to the plane.
__global__ __launch_bounds__(COLOR_THREADS) void yuv8_to_rgb8_kernel(const uint8_t *__restrict__ yi, const uint8_t *__restrict__ ui,
                                                                     const uint8_t *__restrict__ vi, int n, int h, int w, int ch, int cw,
                                                                     int shift, uint8_t *__restrict__ rgb) {
  __shared__ __attribute__((aligned(16))) int16_t t[AIVC_COLOR_INV_TABLES * 256];
  tables_to_lds<AIVC_COLOR_INV_TABLES>(t, AIVC_COLOR_INV);
  const size_t gid = (size_t)blockIdx.x * COLOR_THREADS + threadIdx.x;
  if (gid >= (size_t)n * h * w) return;
  const int xx = (int)(gid % w);
  const int yy = (int)((gid / w) % h);
  const size_t img = gid / w / h;
  const size_t cpix = (img * ch + min(yy >> shift, ch - 1)) * (size_t)cw + min(xx >> shift, cw - 1);
  int r, g, b;
  inv_rgb(t, yi[gid], ui[cpix], vi[cpix], r, g, b);
  rgb[gid * 3] = (uint8_t)r;
  rgb[gid * 3 + 1] = (uint8_t)g;
  rgb[gid * 3 + 2] = (uint8_t)b;
}

static inline bool aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// one thread per work item, COLOR_THREADS per block: the block count has to fit a grid's x dimension
static inline bool grid_ok(size_t items) { return (items + COLOR_THREADS - 1) / COLOR_THREADS <= (size_t)INT32_MAX; }

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_rgb8_to_yuv420u8(const uint8_t *rgb, int32_t n, int32_t h, int32_t w, uint8_t *y, uint8_t *u, uint8_t *v,
                                      aivc_stream_t stream) {
  if (!rgb || !y || n <= 0 || h <= 0 || w <= 0) return AIVC_ERR_ARG;
  const bool chroma = (h / 2) > 0 && (w / 2) > 0;
  if (chroma && (!u || !v)) return AIVC_ERR_ARG;
  const size_t hp = ((size_t)h + 1) / 2;
  const bool vec = w % 16 == 0 && aligned_to(rgb, 16) && aligned_to(y, 16) && (!chroma || (aligned_to(u, 8) && aligned_to(v, 8)));
  const size_t items = (size_t)n * hp * (vec ? (size_t)w / 16 : ((size_t)w + 1) / 2);
  if (!grid_ok(items)) return AIVC_ERR_UNSUPPORTED;
  if (vec)
    hipLaunchKernelGGL(rgb8_to_yuv420u8_vec_kernel, dim3(cdiv(items, COLOR_THREADS)), dim3(COLOR_THREADS), 0, to_stream(stream), rgb,
                       n, h, w, y, u, v);
  else
    hipLaunchKernelGGL(rgb8_to_yuv420u8_kernel, dim3(cdiv(items, COLOR_THREADS)), dim3(COLOR_THREADS), 0, to_stream(stream), rgb, n,
                       h, w, y, u, v);
  return check_launch("rgb8_to_yuv420u8");
}

AIVC_EXPORT int aivc_yuv8_to_rgb8(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, int32_t h, int32_t w, int32_t ch,
                                  int32_t cw, int32_t chroma_shift, uint8_t *rgb, aivc_stream_t stream) {
  if (!y || !u || !v || !rgb || n <= 0 || h <= 0 || w <= 0 || ch <= 0 || cw <= 0) return AIVC_ERR_ARG;
  if (chroma_shift == 0) {
    if (ch != h || cw != w) return AIVC_ERR_ARG;
  } else if (chroma_shift == 1) {
    if (ch < h / 2 || cw < w / 2) return AIVC_ERR_ARG;
  } else {
    return AIVC_ERR_ARG;
  }
  const uintptr_t ca = 16 >> chroma_shift;
  const bool vec = w % 16 == 0 && cw == (w >> chroma_shift) && aligned_to(y, 16) && aligned_to(rgb, 16) && aligned_to(u, ca) &&
                   aligned_to(v, ca);
  const size_t items = (size_t)n * h * (vec ? (size_t)w / 16 : (size_t)w);
  if (!grid_ok(items)) return AIVC_ERR_UNSUPPORTED;
  const dim3 grid(cdiv(items, COLOR_THREADS)), block(COLOR_THREADS);
  if (vec && chroma_shift == 0)
    hipLaunchKernelGGL(yuv8_to_rgb8_vec_kernel<0>, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, rgb);
  else if (vec)
    hipLaunchKernelGGL(yuv8_to_rgb8_vec_kernel<1>, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, rgb);
  else
    hipLaunchKernelGGL(yuv8_to_rgb8_kernel, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, chroma_shift, rgb);
  return check_launch("yuv8_to_rgb8");
}
