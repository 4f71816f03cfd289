// color_matrix.hip -- 8-bit RGB <-> YCbCr by matrix and range (include/aivc_hip_color_matrix.h): integer multiply-adds with 14
// fractional bits, the coefficients kernel arguments.
//
// HBM-bound like color.hip, and with its ownership: 3 B in and 1.5 B out per pixel forward, the reverse backward; nine integer
// multiply-adds per pixel stay well under the memory time, so there is no table and no LDS.  The vector kernels give a thread 16
// consecutive pixels of a row (48 bytes of RGB = three 16-byte accesses, 16 bytes of Y), the forward one both rows of a 2 x 16
// block: the box chroma of a 2 x 2 block is summed in the registers of the one thread that reads all four pixels.  The scalar
// kernels cover every other width / alignment.  No atomics, no memset: every output byte is written exactly once.
#include "common.h"
#include "../../include/aivc_hip_color_matrix.h"

namespace aivc {

constexpr int CM_THREADS = 256;
constexpr int CM_S = AIVC_COLOR_MATRIX_SHIFT;

struct FwdCoef {
  int m[3][3];
  int ybias;    // (fwd_off[0] << S) + (1 << (S - 1))
  int cbias[2]; // the same of Cb, Cr at the chroma shift: S (point) or S + 2 (box)
};
struct InvCoef {
  int cy, rv, gu, gv, bu, yoff;
};

// clamp(v >> SH, 0, 255) with the clamp IN FRONT of the shift: the same value (a floor shift is monotonic, and every v of at
// least 256 << SH lands on 255), but not the shape `clamp(v >> SH)` that hipcc folds, two results at a time, into
// v_ashr_pk_u8_i32.  The code it emits around that instruction takes the upper half of its result to be zero; on the MI355X
// the upper half came back holding bits 16 ... 23 of the unshifted sum of the second source, which the following
// v_lshl_or_b32 then ORed into byte 2 of the packed word (seen as wrong Y at every pixel 4k + 2 of the vector kernel, the
// scalar kernels being right; experiments/colour.md).  The build has none of these instructions now.
template <int SH>
__device__ __forceinline__ int cm_round8(int v) {
  constexpr int top = (256 << SH) - 1;
  return (v < 0 ? 0 : (v > top ? top : v)) >> SH;
}
__device__ __forceinline__ int cm_dot(const int (&row)[3], int r, int g, int b) { return row[0] * r + row[1] * g + row[2] * b; }
__device__ __forceinline__ int cm_luma(const FwdCoef &c, int r, int g, int b) { return cm_round8<CM_S>(cm_dot(c.m[0], r, g, b) + c.ybias); }
// acc: the chroma row times the pixel (point) or the sum of that over the 2 x 2 block (box; the product is linear in the pixel)
template <bool BOX>
__device__ __forceinline__ int cm_chroma(const FwdCoef &c, int k, int acc) {
  return cm_round8<BOX ? CM_S + 2 : CM_S>(acc + c.cbias[k]);
}
__device__ __forceinline__ void cm_inv_rgb(const InvCoef &c, int y, int cb, int cr, int &r, int &g, int &b) {
  const int yy = c.cy * (y - c.yoff) + (1 << (CM_S - 1));
  cb -= 128, cr -= 128;
  r = cm_round8<CM_S>(yy + c.rv * cr);
  g = cm_round8<CM_S>(yy + c.gu * cb + c.gv * cr);
  b = cm_round8<CM_S>(yy + c.bu * cb);
}
// byte k of an array of little-endian words (k is a compile-time constant wherever this is used)
__device__ __forceinline__ int cm_byte_of(const uint32_t *wd, int k) { return (wd[k >> 2] >> ((k & 3) * 8)) & 255u; }

// ---- RGB -> 4:2:0 ------------------------------------------------------------------------------------------------------
// one thread: rows 2 rp and 2 rp + 1, columns 16 g .. 16 g + 15.  w % 16 == 0; rgb, y 16-byte and u, v 8-byte aligned.
template <bool BOX>
__global__ __launch_bounds__(CM_THREADS) void rgb8_to_yuv420u8_matrix_vec_kernel(const uint8_t *__restrict__ rgb, int n, int h, int w,
                                                                                 FwdCoef c, uint8_t *__restrict__ yo,
                                                                                 uint8_t *__restrict__ uo, uint8_t *__restrict__ vo) {
  const int groups = w >> 4, hp = (h + 1) >> 1, ch = h >> 1, cw = w >> 1;
  const size_t gid = (size_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (gid >= (size_t)n * hp * groups) return;
  const int g = (int)(gid % groups);
  const int rp = (int)((gid / groups) % hp);
  const size_t img = gid / groups / hp;
  int cb[8] = {0, 0, 0, 0, 0, 0, 0, 0}, cr[8] = {0, 0, 0, 0, 0, 0, 0, 0};
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
    uint32_t lum[4] = {0, 0, 0, 0};
#pragma unroll
    for (int p = 0; p < 16; ++p) {
      const int r = cm_byte_of(in, 3 * p), gg = cm_byte_of(in, 3 * p + 1), b = cm_byte_of(in, 3 * p + 2);
      lum[p >> 2] |= (uint32_t)cm_luma(c, r, gg, b) << ((p & 3) * 8);
      if (BOX || (row == 0 && (p & 1) == 0)) {
        cb[p >> 1] += cm_dot(c.m[1], r, gg, b);
        cr[p >> 1] += cm_dot(c.m[2], r, gg, b);
      }
    }
    *reinterpret_cast<uint4 *>(yo + pix) = make_uint4(lum[0], lum[1], lum[2], lum[3]);
  }
  if (rp < ch) {  // (both rows of the block lie inside the frame then)
    uint32_t u2[2] = {0, 0}, v2[2] = {0, 0};
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      u2[s >> 2] |= (uint32_t)cm_chroma<BOX>(c, 0, cb[s]) << ((s & 3) * 8);
      v2[s >> 2] |= (uint32_t)cm_chroma<BOX>(c, 1, cr[s]) << ((s & 3) * 8);
    }
    const size_t cpix = (img * ch + rp) * (size_t)cw + 8 * g;
    *reinterpret_cast<uint2 *>(uo + cpix) = make_uint2(u2[0], u2[1]);
    *reinterpret_cast<uint2 *>(vo + cpix) = make_uint2(v2[0], v2[1]);
  }
}

// one thread: the 2 x 2 block at (2 by, 2 bx), what of it lies inside the frame.  Any size and alignment.
template <bool BOX>
__global__ __launch_bounds__(CM_THREADS) void rgb8_to_yuv420u8_matrix_kernel(const uint8_t *__restrict__ rgb, int n, int h, int w, FwdCoef c,
                                                                             uint8_t *__restrict__ yo, uint8_t *__restrict__ uo,
                                                                             uint8_t *__restrict__ vo) {
  const int hp = (h + 1) >> 1, wp = (w + 1) >> 1, ch = h >> 1, cw = w >> 1;
  const size_t gid = (size_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (gid >= (size_t)n * hp * wp) return;
  const int bx = (int)(gid % wp);
  const int by = (int)((gid / wp) % hp);
  const size_t img = gid / wp / hp;
  int cb = 0, cr = 0;
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const int yy = 2 * by + dy, xx = 2 * bx + dx;
      if (yy >= h || xx >= w) continue;
      const size_t pix = (img * h + yy) * (size_t)w + xx;
      const int r = rgb[pix * 3], g = rgb[pix * 3 + 1], b = rgb[pix * 3 + 2];
      yo[pix] = (uint8_t)cm_luma(c, r, g, b);
      if (BOX || (dy == 0 && dx == 0)) {
        cb += cm_dot(c.m[1], r, g, b);
        cr += cm_dot(c.m[2], r, g, b);
      }
    }
  }
  if (by < ch && bx < cw) {  // (all four pixels of the block lie inside the frame then)
    const size_t cpix = (img * ch + by) * (size_t)cw + bx;
    uo[cpix] = (uint8_t)cm_chroma<BOX>(c, 0, cb);
    vo[cpix] = (uint8_t)cm_chroma<BOX>(c, 1, cr);
  }
}

// ---- planar YCbCr -> RGB -------------------------------------------------------------------------------------------------
// one thread: 16 consecutive pixels of one row.  w % 16 == 0, cw == w >> SHIFT exactly; y, rgb 16-byte aligned, u, v aligned to
// their 16 >> SHIFT bytes.
template <int SHIFT>
__global__ __launch_bounds__(CM_THREADS) void yuv8_to_rgb8_matrix_vec_kernel(const uint8_t *__restrict__ yi, const uint8_t *__restrict__ ui,
                                                                             const uint8_t *__restrict__ vi, int n, int h, int w, int ch,
                                                                             int cw, InvCoef c, uint8_t *__restrict__ rgb) {
  const int groups = w >> 4;
  const size_t gid = (size_t)blockIdx.x * CM_THREADS + threadIdx.x;
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
    cm_inv_rgb(c, cm_byte_of(lum, p), cm_byte_of(cb, p >> SHIFT), cm_byte_of(cr, p >> SHIFT), r, gg, b);
    out[(3 * p) >> 2] |= (uint32_t)r << (((3 * p) & 3) * 8);
    out[(3 * p + 1) >> 2] |= (uint32_t)gg << (((3 * p + 1) & 3) * 8);
    out[(3 * p + 2) >> 2] |= (uint32_t)b << (((3 * p + 2) & 3) * 8);
  }
  uint4 *dst = reinterpret_cast<uint4 *>(rgb + pix * 3);
#pragma unroll
  for (int q = 0; q < 3; ++q) dst[q] = make_uint4(out[4 * q], out[4 * q + 1], out[4 * q + 2], out[4 * q + 3]);
}

// one thread per pixel.  Any size and alignment; chroma indices clamp to the plane.
__global__ __launch_bounds__(CM_THREADS) void yuv8_to_rgb8_matrix_kernel(const uint8_t *__restrict__ yi, const uint8_t *__restrict__ ui,
                                                                         const uint8_t *__restrict__ vi, int n, int h, int w, int ch, int cw,
                                                                         int shift, InvCoef c, uint8_t *__restrict__ rgb) {
  const size_t gid = (size_t)blockIdx.x * CM_THREADS + threadIdx.x;
  if (gid >= (size_t)n * h * w) return;
  const int xx = (int)(gid % w);
  const int yy = (int)((gid / w) % h);
  const size_t img = gid / w / h;
  const size_t cpix = (img * ch + min(yy >> shift, ch - 1)) * (size_t)cw + min(xx >> shift, cw - 1);
  int r, g, b;
  cm_inv_rgb(c, yi[gid], ui[cpix], vi[cpix], r, g, b);
  rgb[gid * 3] = (uint8_t)r;
  rgb[gid * 3 + 1] = (uint8_t)g;
  rgb[gid * 3 + 2] = (uint8_t)b;
}

static inline bool cm_aligned_to(const void *p, uintptr_t a) { return (reinterpret_cast<uintptr_t>(p) & (a - 1)) == 0; }
// one thread per work item, CM_THREADS per block: the block count has to fit a grid's x dimension
static inline bool cm_grid_ok(size_t items) { return (items + CM_THREADS - 1) / CM_THREADS <= (size_t)INT32_MAX; }

static inline bool cm_coef_ok(int32_t v) { return v >= -AIVC_COLOR_MATRIX_MAX_COEF && v <= AIVC_COLOR_MATRIX_MAX_COEF; }
static inline bool cm_offset_ok(int32_t v) { return v >= 0 && v <= 255; }
// the limits under which every int32 sum of the kernels stays below 2^31
static bool cm_matrix_ok(const aivc_color_matrix *m) {
  if (!m) return false;
  for (int i = 0; i < 3; ++i) {
    for (int j = 0; j < 3; ++j)
      if (!cm_coef_ok(m->fwd[i][j])) return false;
    if (!cm_offset_ok(m->fwd_off[i])) return false;
  }
  for (int i = 0; i < 5; ++i)
    if (!cm_coef_ok(m->inv[i])) return false;
  return cm_offset_ok(m->inv_yoff);
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_rgb8_to_yuv420u8_matrix(const uint8_t *rgb, int32_t n, int32_t h, int32_t w, const aivc_color_matrix *m,
                                             int32_t chroma_down, uint8_t *y, uint8_t *u, uint8_t *v, aivc_stream_t stream) {
  if (!rgb || !y || n <= 0 || h <= 0 || w <= 0) return AIVC_ERR_ARG;
  if (!cm_matrix_ok(m) || (chroma_down != 0 && chroma_down != 1)) return AIVC_ERR_ARG;
  const bool chroma = (h / 2) > 0 && (w / 2) > 0;
  if (chroma && (!u || !v)) return AIVC_ERR_ARG;
  FwdCoef c;
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) c.m[i][j] = m->fwd[i][j];
  const int cs = chroma_down ? CM_S + 2 : CM_S;
  c.ybias = (m->fwd_off[0] << CM_S) + (1 << (CM_S - 1));
  c.cbias[0] = (m->fwd_off[1] << cs) + (1 << (cs - 1));
  c.cbias[1] = (m->fwd_off[2] << cs) + (1 << (cs - 1));
  const size_t hp = ((size_t)h + 1) / 2;
  const bool vec = w % 16 == 0 && cm_aligned_to(rgb, 16) && cm_aligned_to(y, 16) && (!chroma || (cm_aligned_to(u, 8) && cm_aligned_to(v, 8)));
  const size_t items = (size_t)n * hp * (vec ? (size_t)w / 16 : ((size_t)w + 1) / 2);
  if (!cm_grid_ok(items)) return AIVC_ERR_UNSUPPORTED;
  const dim3 grid(cdiv(items, CM_THREADS)), block(CM_THREADS);
  if (vec && chroma_down)
    hipLaunchKernelGGL(rgb8_to_yuv420u8_matrix_vec_kernel<true>, grid, block, 0, to_stream(stream), rgb, n, h, w, c, y, u, v);
  else if (vec)
    hipLaunchKernelGGL(rgb8_to_yuv420u8_matrix_vec_kernel<false>, grid, block, 0, to_stream(stream), rgb, n, h, w, c, y, u, v);
  else if (chroma_down)
    hipLaunchKernelGGL(rgb8_to_yuv420u8_matrix_kernel<true>, grid, block, 0, to_stream(stream), rgb, n, h, w, c, y, u, v);
  else
    hipLaunchKernelGGL(rgb8_to_yuv420u8_matrix_kernel<false>, grid, block, 0, to_stream(stream), rgb, n, h, w, c, y, u, v);
  return check_launch("rgb8_to_yuv420u8_matrix");
}

AIVC_EXPORT int aivc_yuv8_to_rgb8_matrix(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, int32_t h, int32_t w, int32_t ch,
                                         int32_t cw, int32_t chroma_shift, const aivc_color_matrix *m, uint8_t *rgb,
                                         aivc_stream_t stream) {
  if (!y || !u || !v || !rgb || n <= 0 || h <= 0 || w <= 0 || ch <= 0 || cw <= 0) return AIVC_ERR_ARG;
  if (!cm_matrix_ok(m)) return AIVC_ERR_ARG;
  if (chroma_shift == 0) {
    if (ch != h || cw != w) return AIVC_ERR_ARG;
  } else if (chroma_shift == 1) {
    if (ch < h / 2 || cw < w / 2) return AIVC_ERR_ARG;
  } else {
    return AIVC_ERR_ARG;
  }
  const InvCoef c = {m->inv[0], m->inv[1], m->inv[2], m->inv[3], m->inv[4], m->inv_yoff};
  const uintptr_t ca = 16 >> chroma_shift;
  const bool vec = w % 16 == 0 && cw == (w >> chroma_shift) && cm_aligned_to(y, 16) && cm_aligned_to(rgb, 16) && cm_aligned_to(u, ca) &&
                   cm_aligned_to(v, ca);
  const size_t items = (size_t)n * h * (vec ? (size_t)w / 16 : (size_t)w);
  if (!cm_grid_ok(items)) return AIVC_ERR_UNSUPPORTED;
  const dim3 grid(cdiv(items, CM_THREADS)), block(CM_THREADS);
  if (vec && chroma_shift == 0)
    hipLaunchKernelGGL(yuv8_to_rgb8_matrix_vec_kernel<0>, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, c, rgb);
  else if (vec)
    hipLaunchKernelGGL(yuv8_to_rgb8_matrix_vec_kernel<1>, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, c, rgb);
  else
    hipLaunchKernelGGL(yuv8_to_rgb8_matrix_kernel, grid, block, 0, to_stream(stream), y, u, v, n, h, w, ch, cw, chroma_shift, c, rgb);
  return check_launch("yuv8_to_rgb8_matrix");
}
