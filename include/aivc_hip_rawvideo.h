/*
 * aivc_hip_rawvideo.h -- raw video layouts to and from the codec's 8-bit 4:2:0 planes (part of the C ABI of libaivc_hip.so since
 * ABI 26; conventions, types and error codes: aivc_hip.h).
 *
 * What it is for: reading clips that are not headerless planar 8-bit 4:2:0 -- 10/12/16-bit, 4:2:2, 4:4:4, grey, NV12 / P010
 * surfaces with a row pitch, .y4m files -- and writing a decode in such a layout (aivc_amd/rawvideo.py).  The bytes of the file
 * travel to the device as they are, a frame wherever it lies in them; the conversion is one bandwidth pass there.  The
 * reference has no counterpart: it hands every other format to ffmpeg on the host (src/format_conversion/).
 *
 * THE ARITHMETIC, integers only (restated in numpy: tests/rawvideo_cases.py).
 * A sample's value is its byte, or its little-endian 16-bit word, or word >> (16 - depth) where the significant bits sit at
 * the top of the word (P010, P016).  Bits above the depth in an LSB-aligned word are NOT masked: the clamp below takes them.
 * Ingest, to y [h][w] and u, v [ceil(h/2)][ceil(w/2)].  A source chroma plane has cw_src = ceil(w / 2^shift_x) columns and
 * ch_src = ceil(h / 2^shift_y) rows (ffmpeg's convention).  Luma is one tap.  Chroma output (j, i) is the exact sum s of the
 * t = tx * ty source samples one 4:2:0 sample covers, tx = 2 >> shift_x, ty = 2 >> shift_y: rows min(ty j + a, ch_src - 1),
 * a < ty, columns min(tx i + b, cw_src - 1), b < tx -- edge samples repeat (t = 1 for 4:2:0, 2 for 4:2:2, 4 for 4:4:4).  With
 * sh = depth - 8 + log2 t (luma: t = 1)
 *     out = min(255, s)                                if sh == 0      (s <= 255 there for every layout with one byte per sample)
 *     out = min(255, (s + (1 << (sh - 1))) >> sh)      otherwise
 * ONE rounding of the exact sum, never a box average followed by a second rounding.  For 8-bit planes this is Pillow's
 * Image.reduce.  A layout without chroma gives u = v = 128.  Chroma siting is ignored, as in the resize (aivc_hip_resize.h).
 * Export, from the same planes: value = v << (depth - 8), shifted up again by 16 - depth where the bits sit at the top; chroma
 * is copied or interleaved, a layout without chroma drops it.  Export covers shift_x = shift_y = 1 and layouts without
 * chroma: writing 4:2:2 or 4:4:4 would need a choice of upsampling filter.  Export followed by ingest is the identity.
 * These entry points have no `_ref` twin in the CPU oracle; their CPU statement is the numpy of tests/rawvideo_cases.py.
 */
#ifndef AIVC_HIP_RAWVIDEO_H
#define AIVC_HIP_RAWVIDEO_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum aivc_rawvideo_chroma {
  AIVC_CHROMA_NONE = 0,   /* grey: one plane */
  AIVC_CHROMA_PLANAR = 1, /* planes y, u, v */
  AIVC_CHROMA_UV = 2,     /* planes y, uv: one plane of (u, v) sample pairs (NV12, P010) */
  AIVC_CHROMA_VU = 3      /* planes y, vu (NV21) */
};

/* One frame's layout.  plane 0 is luma, plane 1 u (or the interleaved plane), plane 2 v (planar only); offset and pitch of a
 * plane the layout does not have are ignored.  pitch >= the tight row: w (planar chroma: cw_src; interleaved: 2 cw_src) samples
 * of bytes_per_sample bytes; the bytes of a row behind its tight part are neither read as samples nor written. */
typedef struct aivc_rawvideo_fmt {
  int32_t w, h;             /* luma size, >= 1 */
  int32_t bytes_per_sample; /* 1 or 2 (little-endian words) */
  int32_t depth;            /* significant bits, 8 ... 16; 8 with one byte per sample */
  int32_t msb_aligned;      /* 0: the bits sit at the bottom of the word, 1: at the top */
  int32_t shift_x, shift_y; /* chroma subsampling, each 0 or 1 (ignored without chroma) */
  int32_t chroma;           /* enum aivc_rawvideo_chroma */
  int64_t offset[3];        /* byte offset of each plane in the frame, >= 0 */
  int64_t pitch[3];         /* bytes from a row of the plane to the next */
} aivc_rawvideo_fmt;

/* frames[f] in the layout *fmt  ->  y[f], u[f], v[f]   for f < n.
 *   frames   device table of n device pointers (the table 8-byte aligned), each to one frame's bytes.  A pointer may have ANY
 *            byte alignment (a .y4m frame follows a 6-byte `FRAME\n`: 16-bit samples at odd addresses), and the alignments of
 *            one table may differ.
 *   fmt      host pointer, read before the call returns.
 *   y        [n][h][w] uint8, contiguous; u, v: [n][ceil(h/2)][ceil(w/2)] uint8, contiguous.  Any alignment.
 * ONE launch for all frames and all three planes.  A lane owns one aligned 16-byte chunk of one output row: it reads the 16, 32
 * or 64 source bytes per source row that the chunk's samples come from in aligned 16-byte chunks through the byte funnel of
 * reduce.h (the shift is the lane's own: rows and frames lie anywhere) and stores 16 bytes at once; the chunks at the two ends
 * of a row that hold bytes of a neighbouring row are written byte by byte.  Only source chunks that hold at least one byte of
 * the frame -- offset 0 to the end of its last plane's last tight row -- are read: nothing in front of a frame's first byte or
 * behind its last.  An interleaved chroma plane is read once for u and once for v (the second time out of the cache).
 * No atomics, no memset; every output byte is written exactly once.
 * n == 0 writes nothing and returns AIVC_OK.  AIVC_ERR_ARG: n < 0; with n > 0: a NULL pointer, w or h < 1, bytes_per_sample
 * not 1 or 2, depth outside 8 ... 16, depth > 8 with one byte per sample, msb_aligned not 0 or 1, an unknown chroma
 * arrangement, a shift not 0 or 1, a negative offset, a pitch below the tight row.  AIVC_ERR_UNSUPPORTED: a frame, an offset
 * or a pitch of 2^31 bytes or more; an interleaved chroma plane with shift_x = 0 (NV24: no kernel is built for it).  The grid
 * itself sets no further limit: a frame below 2^31 bytes has fewer than 2^32 output chunks (grid.x counts 256 of them), and
 * the frames of a call are walked by at most 65535 rows of workgroups. */
int aivc_rawvideo_to_yuv420u8(const uint8_t *const *frames, int32_t n, const aivc_rawvideo_fmt *fmt, uint8_t *y, uint8_t *u,
                              uint8_t *v, aivc_stream_t stream);

/* y[f], u[f], v[f]  ->  frames[f] in the layout *fmt   for f < n: the mirror of the above, same arguments, same launch shape (a
 * lane owns one aligned 16-byte chunk of one row of a plane of a frame, wherever the frame lies; chunks that reach over the
 * ends of the row's tight part are written byte by byte) and the same error codes, and in addition AIVC_ERR_UNSUPPORTED for
 * a layout with chroma whose shifts are not both 1.  u and v may be NULL for a layout without chroma.  The planes are read in
 * aligned 16-byte chunks, only chunks that hold at least one byte of the stack they belong to. */
int aivc_yuv420u8_to_rawvideo(const uint8_t *y, const uint8_t *u, const uint8_t *v, int32_t n, const aivc_rawvideo_fmt *fmt,
                              uint8_t *const *frames, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_RAWVIDEO_H */
