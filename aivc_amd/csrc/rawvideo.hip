// rawvideo.hip -- raw video layouts to and from the codec's 8-bit 4:2:0 planes (include/aivc_hip_rawvideo.h, where the arithmetic
// is stated): 8 ... 16-bit samples, 4:2:0 / 4:2:2 / 4:4:4 / grey, planar or interleaved chroma, row pitches, frames at any byte.
//
// Both directions are element-wise passes, HBM-bound, with no reuse to exploit: one launch per call, a lane per ALIGNED 16-byte
// chunk of one row of the side that is written.  What a lane reads -- 16 bytes for an 8-bit plane up to 64 bytes per source row
// for 4:4:4 or interleaved 16-bit chroma -- lies wherever the row and the frame put it, so it comes in aligned 16-byte chunks
// through the byte funnel of reduce.h with the lane's own shift; consecutive lanes read consecutive bytes.  A chunk is loaded
// only if it holds a byte of the buffer it belongs to (the frame, or the stack of planes), so nothing outside is touched; the
// bytes of a chunk that lie outside a row feed outputs that are never stored.  The lanes at the two ends of a row, whose chunk
// holds bytes of a neighbouring row, store byte by byte.
// The work of a frame is laid out flat -- luma rows, then the chroma planes' rows, `chunks per row` lanes each -- on grid.x, the
// frames on grid.y (walked in strides of the grid, so their number has no limit).
#include "reduce.h"
#include "../../include/aivc_hip_rawvideo.h"

namespace aivc {

constexpr int RAW_THREADS = 256;

struct RawGeom {
  int32_t w, h, cw, ch;     // the 4:2:0 side: luma and ceil-half chroma size
  int32_t cw_src, ch_src;   // the layout's chroma plane, in samples (an interleaved plane has 2 cw_src per row)
  int32_t ty;               // source chroma rows per 4:2:0 row
  int32_t sh_y, sh_c;       // ingest: bits dropped from a luma sample / a chroma sum
  int32_t top;              // 16 - depth where the bits sit at the top of the word, else 0
  int32_t up;               // export: a 16-bit word is the byte << up
  int32_t chroma;           // aivc_rawvideo_chroma
  uint32_t cy, cc;          // lanes per row of the written side: luma, chroma
  uint32_t items_y, items_c, items;  // lanes per frame: luma, ONE chroma plane, all
  int64_t off[3], pitch[3];
  int64_t frame_bytes;      // offset 0 ... the end of the last plane's last tight row
};

__device__ __forceinline__ chunk16_t zero16() { return chunk16_t{0u, 0u, 0u, 0u}; }

// V x 16 bytes from address p (any alignment) out of V + 1 aligned chunks; a chunk that holds no byte of [lo, hi) is not loaded
// and reads as zeros
template <int V>
__device__ __forceinline__ void load_bytes(uintptr_t p, uintptr_t lo, uintptr_t hi, uint32_t (&d)[4 * V]) {
  const uintptr_t base = p & ~(uintptr_t)15;
  const uint32_t s = (uint32_t)(p & 15), ws = s >> 2, bs = s & 3u;
  chunk16_t c[V + 1];
#pragma unroll
  for (int k = 0; k <= V; ++k) {  // every load is issued before the first use
    const uintptr_t a = base + 16 * k;
    c[k] = zero16();
    if (a + 16 > lo && a < hi && (k < V || s != 0)) c[k] = *(chunk16_ptr)a;
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    const chunk16_t r = funnel16(c[k], c[k + 1], ws, bs);
    d[4 * k] = r.x, d[4 * k + 1] = r.y, d[4 * k + 2] = r.z, d[4 * k + 3] = r.w;
  }
}

// the chunk of a written row `len` bytes long that starts at row byte x0 (dst + x0 is 16-byte aligned; x0 may be negative and
// x0 + 16 may exceed len): one 16-byte store where the whole chunk is the row's, else its bytes of the row one by one
__device__ __forceinline__ void store_chunk(uint8_t *dst, int64_t len, int64_t x0, const uint32_t (&o)[4]) {
  if (x0 >= 0 && x0 + 16 <= len) {
    *(chunk16_t *)(dst + x0) = chunk16_t{o[0], o[1], o[2], o[3]};
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k)
      if (x0 + k >= 0 && x0 + k < len) dst[x0 + k] = (uint8_t)(o[k >> 2] >> (8 * (k & 3)));
  }
}

// ---- ingest -----------------------------------------------------------------------------------------------------------------
// 16 outputs from column x0 on: output o sums, over `rows` source rows, the TX samples (x0 + o) TX + b, every XS-th sample of the
// row counted (XS = 2: an interleaved plane, p0 / p1 then point at the component's first sample).  n_cols: samples of the
// component per row -- the odd column out at the right edge repeats.
template <int BPS, int TX, int XS>
__device__ __forceinline__ void ingest_chunk(uintptr_t p0, uintptr_t p1, int rows, int64_t x0, int n_cols, uintptr_t lo, uintptr_t hi,
                                             int sh, int top, uint32_t (&out)[4]) {
  constexpr int V = BPS * TX * XS;  // 16-byte vectors per source row
  uint32_t d[2][4 * V];
  const int64_t skip = x0 * (TX * XS * BPS);
  load_bytes<V>(p0 + skip, lo, hi, d[0]);
  if (rows == 2) load_bytes<V>(p1 + skip, lo, hi, d[1]);
  if (BPS == 1 && TX == 1 && XS == 1 && rows == 1) {  // sh == 0: the bytes as they are
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = d[0][j];
    return;
  }
  const uint32_t half = sh > 0 ? 1u << (sh - 1) : 0u;
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = 0;
#pragma unroll
  for (int o = 0; o < 16; ++o) {
    uint32_t s = 0;
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      if (r < rows) {
        uint32_t tap[TX];
#pragma unroll
        for (int b = 0; b < TX; ++b) {
          const int k = (o * TX + b) * XS;  // sample index in the loaded bytes
          tap[b] = BPS == 1 ? (d[r][k >> 2] >> (8 * (k & 3))) & 0xffu : ((d[r][k >> 1] >> (16 * (k & 1))) & 0xffffu) >> top;
        }
        if (TX == 2 && (x0 + o) * 2 + 1 >= n_cols) tap[TX - 1] = tap[0];
#pragma unroll
        for (int b = 0; b < TX; ++b) s += tap[b];
      }
    }
    s = (s + half) >> sh;
    out[o >> 2] |= (s < 255u ? s : 255u) << (8 * (o & 3));
  }
}

template <int BPS, int CTX, int CXS>
__global__ void __launch_bounds__(RAW_THREADS) rawvideo_ingest_kernel(const uint8_t *const *__restrict__ frames, int n, RawGeom g,
                                                                      uint8_t *__restrict__ y, uint8_t *__restrict__ u,
                                                                      uint8_t *__restrict__ v) {
  uint32_t t = blockIdx.x * RAW_THREADS + threadIdx.x;
  if (t >= g.items) return;
  int plane = 0;
  uint32_t per_row = g.cy;
  if (t >= g.items_y) {
    t -= g.items_y;
    plane = 1;
    per_row = g.cc;
    if (t >= g.items_c) t -= g.items_c, plane = 2;
  }
  const int row = (int)(t / per_row), c = (int)(t % per_row);
  const int len = plane ? g.cw : g.w, rows_out = plane ? g.ch : g.h;
  uint8_t *stack = plane == 0 ? y : plane == 1 ? u : v;
  // the source: plane, first sample of the component, rows
  int sp = plane, xo = 0;
  if (plane && g.chroma >= AIVC_CHROMA_UV) sp = 1, xo = (plane == 2) != (g.chroma == AIVC_CHROMA_VU);
  const int ty = plane ? g.ty : 1;
  const int r0 = min(ty * row, (plane ? g.ch_src : g.h) - 1), r1 = min(ty * row + 1, (plane ? g.ch_src : g.h) - 1);
  for (int f = blockIdx.y; f < n; f += gridDim.y) {
    uint8_t *dst = stack + ((size_t)f * rows_out + row) * len;
    const int64_t x0 = 16 * (int64_t)c - (int64_t)((uintptr_t)dst & 15);
    if (x0 >= len) continue;
    uint32_t out[4];
    if (plane && g.chroma == AIVC_CHROMA_NONE) {
      out[0] = out[1] = out[2] = out[3] = 0x80808080u;
    } else {
      const uintptr_t lo = (uintptr_t)frames[f], hi = lo + g.frame_bytes;
      const uintptr_t first = lo + g.off[sp] + xo * BPS;
      const uintptr_t p0 = first + r0 * g.pitch[sp], p1 = first + r1 * g.pitch[sp];
      if (plane == 0)
        ingest_chunk<BPS, 1, 1>(p0, p0, 1, x0, g.w, lo, hi, g.sh_y, g.top, out);
      else
        ingest_chunk<BPS, CTX, CXS>(p0, p1, ty, x0, g.cw_src, lo, hi, g.sh_c, g.top, out);
    }
    store_chunk(dst, len, x0, out);
  }
}

// ---- export -----------------------------------------------------------------------------------------------------------------
// the 16 bytes from byte b0 on of a written row whose samples are BPS bytes each, XS components interleaved: G = BPS XS bytes
// per pixel.  s0 / s1: the component rows (pixels back to back), [lo0, hi0) / [lo1, hi1) the stacks they lie in.
template <int BPS, int XS>
__device__ __forceinline__ void export_chunk(uintptr_t s0, uintptr_t lo0, uintptr_t hi0, uintptr_t s1, uintptr_t lo1, uintptr_t hi1,
                                             int64_t b0, int up, uint32_t (&out)[4]) {
  constexpr int G = BPS * XS, LOG_G = G == 1 ? 0 : G == 2 ? 1 : 2;
  const int64_t g0 = b0 >> LOG_G;  // the pixel the chunk's first byte belongs to (floor: b0 may be negative)
  const uint32_t q = (uint32_t)(b0 & (G - 1));
  uint32_t pix[2][4];
  load_bytes<1>(s0 + g0, lo0, hi0, pix[0]);
  if (XS == 2) load_bytes<1>(s1 + g0, lo1, hi1, pix[1]);
  if (G == 1) {
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = pix[0][j];
    return;
  }
  uint32_t e[5] = {0u, 0u, 0u, 0u, 0u};  // the row's bytes from pixel g0 on: 20 of them hold every shifted chunk
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    const int px = k / G, comp = (k % G) / BPS, bi = k % BPS;
    const uint32_t word = ((pix[comp][px >> 2] >> (8 * (px & 3))) & 0xffu) << (BPS == 2 ? up : 0);
    e[k >> 2] |= ((word >> (8 * bi)) & 0xffu) << (8 * (k & 3));
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[j] = __builtin_amdgcn_alignbyte(e[j + 1], e[j], q);
}

template <int BPS, int CXS>
__global__ void __launch_bounds__(RAW_THREADS) rawvideo_export_kernel(const uint8_t *__restrict__ y, const uint8_t *__restrict__ u,
                                                                      const uint8_t *__restrict__ v, int n, RawGeom g,
                                                                      uint8_t *const *__restrict__ frames) {
  uint32_t t = blockIdx.x * RAW_THREADS + threadIdx.x;
  if (t >= g.items) return;
  int plane = 0;
  uint32_t per_row = g.cy;
  if (t >= g.items_y) {
    t -= g.items_y;
    plane = 1;
    per_row = g.cc;
    if (t >= g.items_c) t -= g.items_c, plane = 2;
  }
  const int row = (int)(t / per_row), c = (int)(t % per_row);
  const bool pairs = plane && CXS == 2;  // the interleaved plane: u and v rows, or v and u
  const int pix = plane ? g.cw : g.w, rows_in = plane ? g.ch : g.h;
  const int64_t len = (int64_t)pix * BPS * (pairs ? 2 : 1);
  const uint8_t *a = plane == 0 ? y : plane == 1 ? u : v, *b = a;
  if (pairs) a = g.chroma == AIVC_CHROMA_VU ? v : u, b = g.chroma == AIVC_CHROMA_VU ? u : v;
  const size_t stack_bytes = (size_t)n * rows_in * pix;
  for (int f = blockIdx.y; f < n; f += gridDim.y) {
    uint8_t *dst = frames[f] + g.off[plane] + row * g.pitch[plane];
    const int64_t b0 = 16 * (int64_t)c - (int64_t)((uintptr_t)dst & 15);
    if (b0 >= len) continue;
    const size_t at = ((size_t)f * rows_in + row) * pix;
    const uintptr_t lo0 = (uintptr_t)a, lo1 = (uintptr_t)b;
    uint32_t out[4];
    if (pairs)
      export_chunk<BPS, 2>(lo0 + at, lo0, lo0 + stack_bytes, lo1 + at, lo1, lo1 + stack_bytes, b0, g.up, out);
    else
      export_chunk<BPS, 1>(lo0 + at, lo0, lo0 + stack_bytes, lo0 + at, lo0, lo0 + stack_bytes, b0, g.up, out);
    store_chunk(dst, len, b0, out);
  }
}

// *fmt checked and laid out for a launch -> AIVC_OK, or the error code.  to_raw: the lanes follow the layout's rows.
static int raw_geometry(const aivc_rawvideo_fmt *fmt, bool to_raw, RawGeom &g) {
  const aivc_rawvideo_fmt &m = *fmt;
  if (m.w < 1 || m.h < 1 || (m.bytes_per_sample != 1 && m.bytes_per_sample != 2) || m.depth < 8 || m.depth > 16 ||
      (m.bytes_per_sample == 1 && m.depth > 8) || (m.msb_aligned != 0 && m.msb_aligned != 1) || m.chroma < AIVC_CHROMA_NONE ||
      m.chroma > AIVC_CHROMA_VU)
    return AIVC_ERR_ARG;
  const bool has_c = m.chroma != AIVC_CHROMA_NONE, pairs = m.chroma >= AIVC_CHROMA_UV;
  if (has_c && (m.shift_x < 0 || m.shift_x > 1 || m.shift_y < 0 || m.shift_y > 1)) return AIVC_ERR_ARG;
  const int sx = has_c ? m.shift_x : 1, sy = has_c ? m.shift_y : 1;
  g.w = m.w, g.h = m.h, g.cw = (m.w + 1) / 2, g.ch = (m.h + 1) / 2;
  g.cw_src = sx ? g.cw : m.w, g.ch_src = sy ? g.ch : m.h;
  const int n_planes = !has_c ? 1 : pairs ? 2 : 3;
  const int64_t tight[3] = {(int64_t)m.w * m.bytes_per_sample, (int64_t)g.cw_src * m.bytes_per_sample * (pairs ? 2 : 1),
                            (int64_t)g.cw_src * m.bytes_per_sample};
  g.frame_bytes = 0;
  for (int p = 0; p < 3; ++p) {
    g.off[p] = g.pitch[p] = 0;
    if (p >= n_planes) continue;
    if (m.offset[p] < 0 || m.pitch[p] < tight[p]) return AIVC_ERR_ARG;
    if (m.offset[p] >= (int64_t)1 << 31 || m.pitch[p] >= (int64_t)1 << 31) return AIVC_ERR_UNSUPPORTED;
    g.off[p] = m.offset[p], g.pitch[p] = m.pitch[p];
    const int64_t end = m.offset[p] + ((p ? g.ch_src : m.h) - 1) * m.pitch[p] + tight[p];
    if (end > g.frame_bytes) g.frame_bytes = end;
  }
  if (g.frame_bytes >= (int64_t)1 << 31) return AIVC_ERR_UNSUPPORTED;
  if (pairs && sx == 0) return AIVC_ERR_UNSUPPORTED;
  if (to_raw && has_c && !(sx == 1 && sy == 1)) return AIVC_ERR_UNSUPPORTED;
  g.ty = 2 >> sy;
  g.sh_y = m.depth - 8;
  g.sh_c = m.depth - 8 + (1 - sx) + (1 - sy);
  g.top = m.msb_aligned ? 16 - m.depth : 0;
  g.up = m.msb_aligned ? 8 : m.depth - 8;
  g.chroma = m.chroma;
  // lanes per row: the aligned chunks a row of len bytes can reach into, wherever it starts
  const int64_t len_y = to_raw ? tight[0] : m.w, len_c = to_raw ? tight[1] : g.cw;
  g.cy = (uint32_t)((len_y + 30) / 16), g.cc = (uint32_t)((len_c + 30) / 16);
  const int planes_c = to_raw ? n_planes - 1 : 2;  // (ingest writes u and v whatever the layout)
  const uint64_t iy = (uint64_t)g.cy * m.h, ic = (uint64_t)g.cc * g.ch, all = iy + planes_c * ic;
  if (all > 0xffffffffull) return AIVC_ERR_UNSUPPORTED;  // (out of reach below 2^31 bytes per frame)
  g.items_y = (uint32_t)iy, g.items_c = (uint32_t)ic, g.items = (uint32_t)all;
  return AIVC_OK;
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_rawvideo_to_yuv420u8(const uint8_t *const *frames, int32_t n, const aivc_rawvideo_fmt *fmt, uint8_t *y,
                                          uint8_t *u, uint8_t *v, aivc_stream_t stream) {
  if (n < 0) return AIVC_ERR_ARG;
  if (n == 0) return AIVC_OK;
  if (!frames || !fmt || !y || !u || !v) return AIVC_ERR_ARG;
  RawGeom g;
  if (const int err = raw_geometry(fmt, false, g)) return err;
  const dim3 grid(cdiv(g.items, RAW_THREADS), n < 65535 ? n : 65535), block(RAW_THREADS);
  const bool wide = fmt->bytes_per_sample == 2, pairs = fmt->chroma >= AIVC_CHROMA_UV;
  const bool two = fmt->chroma != AIVC_CHROMA_NONE && fmt->shift_x == 0;  // two columns per 4:2:0 sample
#define AIVC_RAW_INGEST(BPS, TX, XS) \
  hipLaunchKernelGGL((rawvideo_ingest_kernel<BPS, TX, XS>), grid, block, 0, to_stream(stream), frames, n, g, y, u, v)
  if (wide) {
    if (pairs) AIVC_RAW_INGEST(2, 1, 2); else if (two) AIVC_RAW_INGEST(2, 2, 1); else AIVC_RAW_INGEST(2, 1, 1);
  } else {
    if (pairs) AIVC_RAW_INGEST(1, 1, 2); else if (two) AIVC_RAW_INGEST(1, 2, 1); else AIVC_RAW_INGEST(1, 1, 1);
  }
#undef AIVC_RAW_INGEST
  return check_launch("rawvideo_to_yuv420u8");
}

AIVC_EXPORT int aivc_yuv420u8_to_rawvideo(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n,
                                          const aivc_rawvideo_fmt *fmt, uint8_t *const *frames, aivc_stream_t stream) {
  if (n < 0) return AIVC_ERR_ARG;
  if (n == 0) return AIVC_OK;
  if (!frames || !fmt || !y) return AIVC_ERR_ARG;
  if (fmt->chroma != AIVC_CHROMA_NONE && (!u || !v)) return AIVC_ERR_ARG;
  RawGeom g;
  if (const int err = raw_geometry(fmt, true, g)) return err;
  const dim3 grid(cdiv(g.items, RAW_THREADS), n < 65535 ? n : 65535), block(RAW_THREADS);
  const bool wide = fmt->bytes_per_sample == 2, pairs = fmt->chroma >= AIVC_CHROMA_UV;
#define AIVC_RAW_EXPORT(BPS, XS) \
  hipLaunchKernelGGL((rawvideo_export_kernel<BPS, XS>), grid, block, 0, to_stream(stream), y, u, v, n, g, frames)
  if (wide) {
    if (pairs) AIVC_RAW_EXPORT(2, 2); else AIVC_RAW_EXPORT(2, 1);
  } else {
    if (pairs) AIVC_RAW_EXPORT(1, 2); else AIVC_RAW_EXPORT(1, 1);
  }
#undef AIVC_RAW_EXPORT
  return check_launch("yuv420u8_to_rawvideo");
}
