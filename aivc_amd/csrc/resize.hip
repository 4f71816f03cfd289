// resize.hip -- Pillow's 8-bit resampling of single-channel planes (include/aivc_hip_resize.h): a horizontal pass, then a
// vertical pass on its result rounded to uint8, each a weighted sum over a run-time number of taps with integer coefficients
// from a host-made table.  Integer arithmetic only, so the result depends on neither the grid nor the path a row takes.
//
// Both passes give a thread 4 neighbouring output columns (one 32-bit store where the row allows it) x 4 rows, a workgroup
// 256 columns x 16 rows.  The horizontal pass needs bytes first[i] + k of a row for every column i of the tile: windows that
// overlap and start at any byte, so the rows are staged in LDS with aligned 16-byte loads (a wavefront stages the four rows
// it then computes) and the taps read four bytes of LDS at a time, out of two aligned words.  The vertical pass needs the same four columns of
// count[y] input rows: four bytes a row, straight from memory -- neighbouring output rows share input rows, the second
// read is a cache's.  The tap loops are what the kernels spend their time on, not the traffic: experiments/resize.md.
#include "common.h"
#include "../../include/aivc_hip_resize.h"

namespace aivc {

constexpr int RS_TX = 64, RS_TY = 4;        // threads of a workgroup: column quads x wavefronts
constexpr int RS_COLS = 4, RS_ROWS = 4;     // outputs of a thread
constexpr int RS_TILE_W = RS_TX * RS_COLS;  // 256 columns
constexpr int RS_TILE_H = RS_TY * RS_ROWS;  // 16 rows
static_assert(RS_TILE_W == AIVC_RESIZE_TILE_W, "the header states the tile width");
constexpr int RS_ROUND = 1 << 21, RS_SHIFT = 22;

typedef uint32_t rs_chunk_t __attribute__((ext_vector_type(4)));               // one aligned 16-byte chunk
typedef const rs_chunk_t __attribute__((address_space(1))) *rs_chunk_ptr;     // in global memory: global_load, not flat_load
typedef int32_t rs_int4 __attribute__((ext_vector_type(4)));

// where the planes of a pass lie: a table of pointers (the caller's planes) or back to back (the intermediate)
struct RsSource {
  const uint8_t *const *table;
  const uint8_t *base;
  size_t plane_bytes, pitch;
  __device__ __forceinline__ const uint8_t *plane(size_t p) const { return table ? table[p] : base + p * plane_bytes; }
};

__device__ __forceinline__ uint32_t rs_load4(const uint8_t *p) {  // four bytes at any alignment
  uint32_t v;
  __builtin_memcpy(&v, p, 4);
  return v;
}

// bytes at ... at + 3 of LDS, any alignment, out of the two aligned words that hold them: a misaligned 4-byte LDS read is
// served at about a lane a clock (measured: the horizontal pass ran 3 to 4 times longer with them, experiments/resize.md)
__device__ __forceinline__ uint32_t rs_lds_load4(const uint8_t *lds, uint32_t at) {
  const uint32_t *w = (const uint32_t *)lds + (at >> 2);
  return __builtin_amdgcn_alignbyte(w[1], w[0], at & 3u);  // ({w[1], w[0]} >> 8 (at & 3)), low word
}

// acc[j] += byte j of v * k   (|k| < 2^23: v_mad_i32_i24)
__device__ __forceinline__ void rs_mad4(int32_t (&acc)[RS_COLS], uint32_t v, int32_t k) {
#pragma unroll
  for (int j = 0; j < RS_COLS; ++j) acc[j] = (__mul24((int)((v >> (8 * j)) & 255u), k) + acc[j]);
}

__device__ __forceinline__ uint32_t rs_clip(int32_t acc) {
  const int32_t v = acc >> RS_SHIFT;
  return (uint32_t)(v < 0 ? 0 : v > 255 ? 255 : v);
}

// columns x ... x + 3 of the output row at `row` (the row's first byte), w columns wide
__device__ __forceinline__ void rs_store4(uint8_t *row, int x, int w, const int32_t (&acc)[RS_COLS]) {
  uint32_t b[RS_COLS];
#pragma unroll
  for (int j = 0; j < RS_COLS; ++j) b[j] = rs_clip(acc[j]);
  uint8_t *o = row + x;
  if (x + RS_COLS <= w && ((uintptr_t)o & 3) == 0) {
    *(uint32_t *)o = b[0] | b[1] << 8 | b[2] << 16 | b[3] << 24;
  } else {
#pragma unroll
    for (int j = 0; j < RS_COLS; ++j)
      if (x + j < w) o[j] = (uint8_t)b[j];
  }
}

// Horizontal pass.  grid (tiles of 16 rows over ALL planes, tiles of 256 columns), dynamic LDS RS_TILE_H * lds_pitch bytes,
// lds_pitch = x_span + 19 rounded up to 16.  dst: rows of dst_pitch bytes back to back over all planes.
__global__ void __launch_bounds__(RS_TX *RS_TY) resize_rows_kernel(RsSource src, int h, int w_in, int w_out, size_t rows,
                                                                    const int32_t *__restrict__ xb, const int32_t *__restrict__ xk,
                                                                    int taps, int kpitch, int lds_pitch, uint8_t *__restrict__ dst,
                                                                    size_t dst_pitch) {
  extern __shared__ __attribute__((aligned(16))) uint8_t rs_lds[];
  const int tx = threadIdx.x, ty = threadIdx.y;
  const int x0 = blockIdx.y * RS_TILE_W;
  const int xl = min(x0 + RS_TILE_W - 1, w_out - 1);
  const int s0 = xb[2 * x0];                           // the tile's first input column
  const int need = min(xb[2 * xl] + taps, w_in) - s0;  // bytes of a row from there on that a tap with a coefficient can touch
  const size_t row0 = (size_t)blockIdx.x * RS_TILE_H + (size_t)ty * RS_ROWS;
  int shift[RS_ROWS];
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) {  // this wavefront's rows: aligned chunks -> LDS, the row's misalignment kept as `shift`
    shift[r] = 0;
    if (row0 + r < rows) {
      const size_t p = (row0 + r) / (size_t)h;
      const uint8_t *g = src.plane(p) + (row0 + r - p * (size_t)h) * src.pitch + s0;
      const int sh = (int)((uintptr_t)g & 15);
      shift[r] = sh;
      rs_chunk_ptr a = (rs_chunk_ptr)(g - sh);
      rs_chunk_t *l = (rs_chunk_t *)(rs_lds + (size_t)(ty * RS_ROWS + r) * lds_pitch);
      const int nch = (sh + need + 15) >> 4;  // every one of them holds a byte of the row; 16 nch + 4 <= lds_pitch
      for (int c = tx; c < nch; c += RS_TX) l[c] = a[c];
    }
  }
  __syncthreads();
  const int xq = x0 + tx * RS_COLS;
  int off[RS_COLS];
#pragma unroll
  for (int j = 0; j < RS_COLS; ++j) off[j] = xb[2 * min(xq + j, w_out - 1)] - s0;
  int32_t acc[RS_ROWS][RS_COLS];
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r)
#pragma unroll
    for (int j = 0; j < RS_COLS; ++j) acc[r][j] = RS_ROUND;
  const bool kin = xq < kpitch;  // (a quad behind the last column has no coefficients: zeros)
  // Four taps a step.  A tap behind a column's count has a zero coefficient; the LDS byte it multiplies lies inside the row
  // of the image (offset < 15 + x_span), staged or not, and so does the second aligned word of its load (< 19 + x_span <= lds_pitch).
  for (int k = 0; k < taps; k += 4) {
    rs_int4 kq[4];
#pragma unroll
    for (int t = 0; t < 4; ++t) kq[t] = kin ? *(const rs_int4 *)(xk + (size_t)(k + t) * kpitch + xq) : rs_int4{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < RS_ROWS; ++r) {
      const uint32_t at = (uint32_t)((ty * RS_ROWS + r) * lds_pitch + shift[r] + k);
#pragma unroll
      for (int j = 0; j < RS_COLS; ++j) {
        const uint32_t v = rs_lds_load4(rs_lds, at + off[j]);
        const int32_t k0 = kq[0][j], k1 = kq[1][j], k2 = kq[2][j], k3 = kq[3][j];
        int32_t a = acc[r][j];
        a = (__mul24((int)(v & 255u), k0) + a);
        a = (__mul24((int)((v >> 8) & 255u), k1) + a);
        a = (__mul24((int)((v >> 16) & 255u), k2) + a);
        acc[r][j] = (__mul24((int)(v >> 24), k3) + a);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r)
    if (row0 + r < rows && xq < w_out) rs_store4(dst + (row0 + r) * dst_pitch, xq, w_out, acc[r]);
}

// Vertical pass.  grid (n * tiles_y, tiles of 256 columns): workgroup (p * tiles_y + t, bx) writes rows 16 t ... of plane p.
// dst: [n][h_out][w] back to back.
__global__ void __launch_bounds__(RS_TX *RS_TY) resize_cols_kernel(RsSource src, int h_out, int w, int tiles_y,
                                                                    const int32_t *__restrict__ yb, const int32_t *__restrict__ yk,
                                                                    int kpitch, uint8_t *__restrict__ dst) {
  const size_t p = blockIdx.x / (unsigned)tiles_y;
  const int tile = (int)(blockIdx.x - p * (unsigned)tiles_y);
  const int xq = (blockIdx.y * RS_TX + threadIdx.x) * RS_COLS;
  if (xq >= w) return;
  const uint8_t *s = src.plane(p) + xq;
  const bool whole = xq + RS_COLS <= w;  // else: the last columns of the rows, byte by byte (nothing behind a row is read)
  uint8_t *d = dst + p * (size_t)h_out * w;
#pragma unroll
  for (int r = 0; r < RS_ROWS; ++r) {
    const int y = tile * RS_TILE_H + threadIdx.y * RS_ROWS + r;
    if (y >= h_out) break;
    const int first = yb[2 * y], count = yb[2 * y + 1];
    const uint8_t *in = s + (size_t)first * src.pitch;
    const int32_t *kp = yk + y;
    int32_t acc[RS_COLS] = {RS_ROUND, RS_ROUND, RS_ROUND, RS_ROUND};
    if (whole) {
#pragma unroll 4
      for (int k = 0; k < count; ++k) rs_mad4(acc, rs_load4(in + (size_t)k * src.pitch), kp[(size_t)k * kpitch]);
    } else {
      for (int k = 0; k < count; ++k) {
        uint32_t v = 0;
        for (int j = 0; xq + j < w; ++j) v |= (uint32_t)in[(size_t)k * src.pitch + j] << (8 * j);
        rs_mad4(acc, v, kp[(size_t)k * kpitch]);
      }
    }
    rs_store4(d + (size_t)y * w, xq, w, acc);
  }
}

// neither pass: plane p -> dst + p * len, four bytes a thread
__global__ void __launch_bounds__(256) resize_copy_kernel(const uint8_t *const *__restrict__ planes, size_t len, size_t quads,
                                                          uint8_t *__restrict__ dst) {
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= quads) return;
  const uint8_t *s = planes[blockIdx.y];
  uint8_t *d = dst + (size_t)blockIdx.y * len;
  for (size_t i = 4 * q; i < min(4 * q + 4, len); ++i) d[i] = s[i];
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_resize_u8(const uint8_t *const *planes, int32_t n, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out,
                               const int32_t *xb, const int32_t *xk, int32_t x_taps, int32_t x_span, const int32_t *yb,
                               const int32_t *yk, uint8_t *tmp, uint8_t *out, aivc_stream_t stream) {
  if (n < 0) return AIVC_ERR_ARG;
  if (n == 0) return AIVC_OK;
  if (!planes || !out || h_in < 1 || w_in < 1 || h_out < 1 || w_out < 1) return AIVC_ERR_ARG;
  if (!xb != !xk || !yb != !yk) return AIVC_ERR_ARG;
  if ((!xb && w_out != w_in) || (!yb && h_out != h_in)) return AIVC_ERR_ARG;
  if (xb && (x_taps < 4 || x_taps % 4 || x_span < 1)) return AIVC_ERR_ARG;
  if (xb && yb && !tmp) return AIVC_ERR_ARG;
  if (xb && x_span > AIVC_RESIZE_MAX_SPAN) return AIVC_ERR_UNSUPPORTED;  // LDS: 16 rows of x_span + 19 bytes in 64 KiB
  const size_t col_tiles = ((size_t)w_out + RS_TILE_W - 1) / RS_TILE_W;
  const size_t row_tiles_h = ((size_t)n * h_in + RS_TILE_H - 1) / RS_TILE_H;  // horizontal pass: rows of all planes
  const size_t tiles_y = ((size_t)h_out + RS_TILE_H - 1) / RS_TILE_H;         // vertical pass: per plane
  if (col_tiles > 65535) return AIVC_ERR_UNSUPPORTED;
  if (xb && row_tiles_h > 0x7fffffffull) return AIVC_ERR_UNSUPPORTED;
  if (yb && (size_t)n * tiles_y > 0x7fffffffull) return AIVC_ERR_UNSUPPORTED;
  hipStream_t s = to_stream(stream);
  const dim3 block(RS_TX, RS_TY);
  if (!xb && !yb) {
    const size_t len = (size_t)h_in * w_in, quads = (len + 3) / 4;
    if ((quads + 255) / 256 > 0x7fffffffull || n > 65535) return AIVC_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(resize_copy_kernel, dim3((unsigned)((quads + 255) / 256), n), dim3(256), 0, s, planes, len, quads, out);
    return check_launch("resize_u8 (copy)");
  }
  RsSource src{planes, nullptr, 0, (size_t)w_in};
  if (xb) {
    const size_t pitch = yb ? AIVC_RESIZE_PITCH(w_out) : (size_t)w_out;
    const int lds_pitch = (x_span + 19 + 15) & ~15;
    hipLaunchKernelGGL(resize_rows_kernel, dim3((unsigned)row_tiles_h, (unsigned)col_tiles), block, (size_t)RS_TILE_H * lds_pitch, s,
                       src, h_in, w_in, w_out, (size_t)n * h_in, xb, xk, x_taps, (int)AIVC_RESIZE_PITCH(w_out), lds_pitch,
                       yb ? tmp : out, pitch);
    src = RsSource{nullptr, tmp, (size_t)h_in * pitch, pitch};
  }
  if (yb)
    hipLaunchKernelGGL(resize_cols_kernel, dim3((unsigned)((size_t)n * tiles_y), (unsigned)col_tiles), block, 0, s, src, h_out, w_out,
                       (int)tiles_y, yb, yk, (int)AIVC_RESIZE_PITCH(h_out), out);
  return check_launch("resize_u8");
}
