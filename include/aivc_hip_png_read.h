/*
 * aivc_hip_png_read.h -- reading PNG pictures on the device: a batched zlib inflate and the inverse of the row filters (part of
 * the C ABI of libaivc_hip.so; conventions, types and error codes: aivc_hip.h).  ABI 26: entry points were added, none changed.
 *
 * What it is for: the encoder's picture folders (aivc_amd/png.py: read_pictures, encode.py --png_reader device) without one host
 * core inflating every picture.  The host walks each file's chunks, checks their CRC-32 and hands the concatenated IDAT payloads
 * over (aivc_amd/png.py: parse); the device inflates every stream of a batch at once, a workgroup per stream, and undoes the
 * filters, a wavefront per picture.  8-bit grey and 8-bit RGB, not interlaced.  Out of scope: palette, alpha, 16-bit, sub-byte
 * and Adam7 pictures (the host reads those with Pillow), one stream split over several workgroups, a CRC-32 on the device.
 *
 * THE FILTERED STREAM is the one aivc_hip_png.h states for the writer: per row a type byte 0 ... 4 and rb = w c residuals, with
 * a, b, d the bytes to the left (c bytes back), above and above-left (0 outside the picture) and pred = 0, a, b,
 * floor((a + b) / 2) or Paeth's.  The pixel is residual + pred (mod 256).
 */
#ifndef AIVC_HIP_PNG_READ_H
#define AIVC_HIP_PNG_READ_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* info[k][0] of aivc_inflate: what became of stream k */
#define AIVC_INFLATE_OK 0
#define AIVC_INFLATE_SRC_EXHAUSTED 1    /* the stream needs more bytes than its source range holds */
#define AIVC_INFLATE_BAD_HEADER 2       /* zlib header: CM is not 8, a window above 32 KiB, check bits wrong, or FDICT set */
#define AIVC_INFLATE_BAD_BLOCK_TYPE 3   /* the reserved block type 3 */
#define AIVC_INFLATE_STORED_MISMATCH 4  /* a stored block whose NLEN is not ~LEN */
#define AIVC_INFLATE_BAD_LENGTHS 5      /* the code lengths of a dynamic block: more than 286 literal/length or 30 distance
                                           codes, a set that is over-subscribed, or incomplete other than where zlib takes it (no
                                           code at all; one code of one bit, but not for the code-length code), a repeat with
                                           nothing before it, a run past HLIT + HDIST, or no end-of-block code */
#define AIVC_INFLATE_BAD_SYMBOL 6       /* bits that are no code of the block's set, literal/length symbol 286 or 287, distance
                                           symbol 30 or 31 */
#define AIVC_INFLATE_BAD_DISTANCE 7     /* a match that starts before the start of the output */
#define AIVC_INFLATE_TOO_LONG 8         /* more output than the destination range expects */
#define AIVC_INFLATE_TOO_SHORT 9        /* the final block ended with less */
#define AIVC_INFLATE_BAD_ADLER 10       /* the Adler-32 behind the blocks is not the sum of the output */
#define AIVC_INFLATE_TOO_LARGE 11       /* a table row that states 2^31 bytes or more: nothing was read or written */

/* zlib streams -> their bytes: one launch for a batch of n streams of any mix of sizes, a workgroup (one wavefront) per stream.
 *   src     the bytes of all streams, any alignment.
 *   table   [n][4] uint64 in device memory, 8-byte aligned: source offset in src, source bytes, destination offset in dst, the
 *           destination bytes expected EXACTLY (a PNG's h (1 + w c)).  The ranges of different streams do not overlap.
 *   max_src_bytes, max_dst_bytes   the caller's statement of the largest source and destination range in the table, checked
 *           here; a row that states more than 2^31 - 1 all the same gets AIVC_INFLATE_TOO_LARGE.
 *   dst     the output.
 *   info    [n][4] uint32: status (above), bytes produced, source bytes consumed up to and with the Adler-32 (where the status
 *           is AIVC_INFLATE_OK; bytes behind the trailer are ignored), 0.
 * A stream is decoded as RFC 1950 / 1951 state it: stored, fixed and dynamic blocks, matches of every length 3 ... 258 and
 * distance 1 ... 32768, the overlapping kind included; the Adler-32 is summed on the device over what was produced.  Whatever the
 * source bytes are, a stream's workgroup reads src only inside [offset, offset + bytes), writes dst only inside its destination
 * range (a failed stream leaves there what it had produced) and writes its own row of info.  No global atomics, no memset.
 * AIVC_ERR_ARG: a NULL pointer, n < 1.  AIVC_ERR_UNSUPPORTED: max_src_bytes or max_dst_bytes of 2^31 or more. */
int aivc_inflate(const uint8_t *src, const uint64_t *table, int32_t n, uint64_t max_src_bytes, uint64_t max_dst_bytes, uint8_t *dst,
                 uint32_t *info, aivc_stream_t stream);

/* status[k] of aivc_png_unfilter */
#define AIVC_PNG_UNFILTER_OK 0
#define AIVC_PNG_UNFILTER_BAD_TYPE 1   /* a row whose type byte is above 4 (such a row is taken as type 0) */
#define AIVC_PNG_UNFILTER_BAD_SHAPE 2  /* a table row with h or w < 1, c not 1 or 3, or 2^31 filtered bytes or more: nothing done */

/* filtered streams -> pixels: one launch for a batch of n pictures of any mix of sizes, a wavefront per picture.
 *   filt    the filtered streams (what aivc_inflate produced).
 *   table   [n][4] uint64 in device memory, 8-byte aligned: offset of the picture's h (1 + w c) filtered bytes in filt, offset of
 *           its h w c pixel bytes in pix, h << 32 | w, c (1 or 3).
 *   max_bytes  the caller's statement of the largest h (1 + w c) in the table, checked here.
 *   pix     the pixels, [h][w][c] per picture.
 *   status  [n] uint32, above.
 * Lane k of the wavefront takes row r0 + k of a band of 64 rows, one pixel behind lane k - 1, so that the bytes above and
 * above-left arrive from the neighbouring lane; the first row of a band reads the row above from pix.  A picture's wavefront
 * reads and writes only that picture's ranges and its own status word.
 * AIVC_ERR_ARG: a NULL pointer, n < 1.  AIVC_ERR_UNSUPPORTED: max_bytes of 2^31 or more. */
int aivc_png_unfilter(const uint8_t *filt, const uint64_t *table, int32_t n, uint64_t max_bytes, uint8_t *pix, uint32_t *status,
                      aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_PNG_READ_H */
