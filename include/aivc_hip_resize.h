/*
 * aivc_hip_resize.h -- Pillow's 8-bit resampling of single-channel planes (part of the C ABI of libaivc_hip.so since ABI 25;
 * conventions, types and error codes: aivc_hip.h).
 *
 * What it is for: coding a clip at another size than it arrives in, and writing a decode at display size
 * (real_life.encode.encode({'size': ...}), real_life.decode.decode_one_video({'out_size': ...})).  The planes lie on the device as
 * separate tensors (read_yuv, the decoder's output) and never leave it.  The reference has no counterpart: its conversion
 * scripts go through Pillow or ffmpeg on the host.
 *
 * The arithmetic is Image.resize on an 'L' picture (reducing_gap=None, the whole picture as box; the filters box, bilinear,
 * hamming, bicubic and lanczos, which share one code path in Pillow) and the result equals Pillow's byte for byte.  One axis,
 * n_in -> n_out samples: output i is
 *     clip((2^21 + sum over k < count[i] of in[first[i] + k] * K[k][i]) >> 22, 0, 255)
 * with an int32 accumulator and an arithmetic shift; (first, count) and the integer coefficients K (units of 2^-22) are
 * computed on the host in double (aivc_amd/resize.py: axis_tables) and handed in as tables, the device does integer work only.
 * A resize is the horizontal pass, then the vertical pass on its result ROUNDED TO uint8: the order is part of the contract.
 * A pass whose table pointer is NULL is not run (Pillow skips the pass of an axis that keeps its size); with both NULL the
 * planes are copied.
 * This entry point has no `_ref` twin in the CPU oracle; its CPU statement is Pillow itself (tests/resize_cases.py).
 */
#ifndef AIVC_HIP_RESIZE_H
#define AIVC_HIP_RESIZE_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* rows of the tables and of the intermediate are padded to a multiple of 4 entries / bytes */
#define AIVC_RESIZE_PITCH(w) (((size_t)(w) + 3) & ~(size_t)3)
/* bytes of the intermediate (the horizontal pass's result) for n planes; needed only when both passes run */
#define AIVC_RESIZE_TMP_BYTES(n, h_in, w_out) ((size_t)(n) * (size_t)(h_in) * AIVC_RESIZE_PITCH(w_out))
/* output columns of one workgroup of the horizontal pass, and the input bytes per row it can hold in LDS */
#define AIVC_RESIZE_TILE_W 256
#define AIVC_RESIZE_MAX_SPAN 4064

/* out[p] = resize(planes[p])  for p < n.
 *   planes   device table of n device pointers (the table 8-byte aligned), each to h_in x w_in bytes, rows back to back.  A
 *            pointer may have ANY alignment, and the alignments of one table may differ.
 *   out      [n][h_out][w_out] uint8, contiguous, any alignment (rows that start on a 4-byte boundary are stored as words).
 *   xb, xk   the horizontal pass, or both NULL (then w_out == w_in).  xb: int32 [w_out][2], (first, count) per output column,
 *            first + count <= w_in.  xk: int32 [x_taps][AIVC_RESIZE_PITCH(w_out)], TRANSPOSED: xk[k][i] is coefficient k of
 *            column i, zero for k >= count[i] and in the padding columns; |K| < 2^23.  x_taps: a multiple of 4, >= every count.
 *   x_span   max over the tiles t of AIVC_RESIZE_TILE_W columns of first[last column of t] + x_taps - first[first column of t]:
 *            the input bytes a workgroup stages per row.
 *   yb, yk   the vertical pass in the same layout ([h_out][2], [rows >= every count][AIVC_RESIZE_PITCH(h_out)]), or both NULL
 *            (then h_out == h_in).
 *   tmp      AIVC_RESIZE_TMP_BYTES(n, h_in, w_out) bytes of scratch, 4-byte aligned, when both passes run; else unused.
 * Launches: one per pass (or one copy).  Horizontal: a workgroup takes 16 rows x 256 output columns; each of its four
 * wavefronts loads the input bytes of its four rows in aligned 16-byte chunks into LDS (a row's misalignment becomes a byte
 * offset into its LDS row; only chunks that hold at least one byte of the plane are read) and runs the tap loop -- a run-time
 * loop over the table, four taps a step -- out of LDS.  Vertical: a thread takes 4 columns x 4 output rows and reads its input
 * rows four bytes at a time through the caches.  No atomics, no memset; every output byte is written exactly once.
 * n == 0 writes nothing and returns AIVC_OK.  AIVC_ERR_ARG: n < 0; with n > 0: a size < 1, a NULL table / out, one table of a
 * pass without the other, a skipped pass whose axis changes size, x_taps < 4 or not a multiple of 4, x_span < 1, both passes
 * without tmp.  AIVC_ERR_UNSUPPORTED: x_span > AIVC_RESIZE_MAX_SPAN (LDS), or a grid the launch cannot express (more than
 * 2^31 - 1 tiles of 16 rows over all planes, more than 65535 tiles of 256 columns; for the copy, more than 65535 planes). */
int aivc_resize_u8(const uint8_t *const *planes, int32_t n, int32_t h_in, int32_t w_in, int32_t h_out, int32_t w_out,
                   const int32_t *xb, const int32_t *xk, int32_t x_taps, int32_t x_span, const int32_t *yb, const int32_t *yk,
                   uint8_t *tmp, uint8_t *out, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_RESIZE_H */
