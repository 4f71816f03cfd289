/*
 * aivc_hip_png.h -- PNG coding of 8-bit pictures on the device: row filters and a per-segment dynamic-Huffman deflate (part of
 * the C ABI of libaivc_hip.so; conventions, types and error codes: aivc_hip.h).  ABI 26: entry points were added, none changed.
 *
 * What it is for: writing the RGB pictures of a decode (aivc_amd/png.py, decode.py --png_coder device) without one host core
 * running zlib per picture.  The device produces, per picture, the bytes of a complete zlib stream but for its last four -- the
 * Adler-32, which the host folds from per-segment partial sums -- and the host wraps them into the container: signature, IHDR,
 * one IDAT, IEND, the CRC-32 of each chunk (aivc_amd/png.py: assemble).  Reading PNGs is aivc_hip_png_read.h.  Out of scope:
 * 16-bit samples, palette, alpha, Adam7, general LZ77 matching.
 *
 * THE FILTERED STREAM.  pix [n][h][w][c] uint8, c = 1 (grey) or 3 (RGB).  With rb = w c, row r of a picture becomes the 1 + rb
 * bytes `type, x[0] - pred(0), ..., x[rb - 1] - pred(rb - 1)` (mod 256), where a = x[i - c] (0 for i < c), b = the byte above
 * (0 in row 0), d = the byte above a, and pred is 0 (type 0, None), a (1, Sub), b (2, Up), floor((a + b) / 2) (3, Average) or
 * Paeth's (4): with p = a + b - d the first of a, b, d in that order whose distance to p is smallest.  filter 0 ... 4 gives
 * every row that type; filter 5 gives each row the type whose residuals, read as signed bytes, have the smallest sum of
 * absolute values, the lowest type among equals.
 *
 * SEGMENTS.  The filtered stream of a picture is cut into segments of rows_per_segment whole rows (the last one holds what is
 * left), nseg = ceil(h / rows_per_segment) of them.  rows_per_segment is the caller's (>= 1); aivc_amd/png.py uses
 * max(1, 16384 / (1 + rb)).  Each segment is coded on its own by one workgroup into its own slot: one deflate block of dynamic
 * Huffman codes whose tokens are literals and matches of distance 1 (runs, 3 ... AIVC_PNG_RUN bytes; a run does not cross a
 * multiple of AIVC_PNG_RUN bytes counted from the segment's start), code lengths from the segment's own histogram limited to
 * 15 bits (7 for the code-length code, whose header uses the repeat symbols 16 ... 18), closed by an empty stored block (zlib's
 * sync flush) -- or, where that is not smaller, stored blocks of at most 65535 bytes.  Either way a segment's bytes end on a
 * byte boundary in a non-final block, so the segments of a picture concatenate.  Sizes, with len = the bytes of a full segment:
 *     seg_stride = len rounded up to 16           bytes between segments in `filt`
 *     slot_bytes = (len + 5 ceil(len / 65535) + 4) rounded up to 16       bytes between slots in `slots`
 * A picture's bytes depend on its pixels, filter and rows_per_segment alone.
 */
#ifndef AIVC_HIP_PNG_H
#define AIVC_HIP_PNG_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define AIVC_PNG_RUN 32        /* the longest run match, and the bytes one lane tokenizes */
#define AIVC_PNG_SEG_WORDS 4   /* uint32 per segment in seg_info: coded bytes, Adler s1, Adler s2, 0 */

/* pix -> the coded segments.
 *   pix       [n][h][w][c] uint8, contiguous, any alignment.
 *   filt      workspace, n * nseg * seg_stride bytes, 16-byte aligned: the filtered stream, each segment at a multiple of
 *             seg_stride.  Every byte of a segment is written before it is read; the bytes behind a segment up to the next
 *             multiple of 4 are read and ignored.
 *   slots     n * nseg * slot_bytes bytes, 16-byte aligned: segment s of picture p is coded to slots + (p nseg + s) slot_bytes.
 *   seg_info  [n * nseg][AIVC_PNG_SEG_WORDS] uint32: the coded bytes of the segment; s1 = sum b_i mod 65521 and
 *             s2 = sum (len - i) b_i mod 65521 over its len filtered bytes b_0 ..., from which the host folds the Adler-32 in
 *             segment order: B += len A + s2, A += s1 (mod 65521, A = 1 and B = 0 at the start); 0.
 * Two launches: the filter (a wavefront per row) and the coder (a workgroup per segment).  No global atomics, no memset.
 * AIVC_ERR_ARG: a NULL pointer, n, h, w or rows_per_segment < 1, c not 1 or 3, filter outside 0 ... 5.  AIVC_ERR_UNSUPPORTED:
 * a segment of 2^31 bytes or more, or more than 2^31 - 1 rows or segments in the batch. */
int aivc_png_deflate(const uint8_t *pix, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter, int32_t rows_per_segment,
                     uint8_t *filt, uint8_t *slots, uint32_t *seg_info, aivc_stream_t stream);

/* the coded segments -> zlib streams without their Adler-32.
 *   dst       [n * nseg] uint64, 8-byte aligned: where in `out` the bytes of each segment go (the host's prefix sum over
 *             seg_info: a picture takes 2 + the sum of its segments' bytes + 5 + 4).
 *   out       the streams.  In front of a picture's first segment (dst - 2) the launch writes 78 01, behind its last one the
 *             final empty stored block 01 00 00 FF FF; the four bytes behind that are the host's.
 * One launch, a workgroup per segment.  Errors as above. */
int aivc_png_gather(const uint8_t *slots, const uint32_t *seg_info, const uint64_t *dst, int32_t n, int32_t h, int32_t w,
                    int32_t c, int32_t rows_per_segment, uint8_t *out, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_PNG_H */
