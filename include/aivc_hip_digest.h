/*
 * aivc_hip_digest.h -- MD5 of many equal-sized device buffers in one launch (part of the C ABI of libaivc_hip.so since ABI 23;
 * conventions, types and error codes: aivc_hip.h).
 *
 * What it is for: the frame digests of the sidecar manifest `<bitstream>.md5` (aivc_amd/digests.py).  The encoder digests every
 * reconstructed 8-bit plane where it lies, on the device, the decoder does the same with what it decoded, and 16 bytes per plane
 * travel to the host instead of the plane.  The always-on detector of a foreign stream, the range decoder's bit count, sees the
 * entropy stage only; a synthesis transform that computes other bits than the encoder's changes samples and references without
 * moving one CDF bound.
 *
 * Replaces: the host digests of src/real_life/decode.py:304-326 (md5 of a PNG file per plane); here the digest is of the raw plane.
 *
 * MD5 is a serial chain over the 64-byte blocks of a message, so the parallelism is ACROSS messages: one message per lane, 64
 * messages per wavefront, as in range_encode_lanes_kernel.  All messages of a call have one length, so a wavefront never diverges
 * on the block count; callers digest the planes of one kind (all Y, all U, all V) per call.
 *
 * The statement of this entry point is RFC 1321 itself: it has no `_ref` twin in the CPU oracle, tests/test_gpu_digest.py compares
 * it with hashlib.
 */
#ifndef AIVC_HIP_DIGEST_H
#define AIVC_HIP_DIGEST_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* digests[i] = MD5(msgs[i][0 .. len - 1]) for i < n, 16 bytes each in RFC 1321 byte order (what hashlib's digest() returns).
 *   msgs     device table of n device pointers (the table 8-byte aligned).  A message may start at ANY byte address: a plane is
 *            a view into a batch stack.  The kernel reads aligned 16-byte chunks only, and only chunks that hold at least one
 *            message byte.  With len == 0 the pointers are not read through at all.
 *   len      common length in bytes, 0 <= len < 2^31.  len == 0: the digest of the empty string.
 *   digests  device, [n][16]; written with one 16-byte store per message when 16-byte aligned, byte by byte otherwise.
 * n == 0 does nothing and returns AIVC_OK.  AIVC_ERR_ARG: n < 0, len < 0, len >= 2^31, or a NULL table / output with n > 0.
 * The 64-bit bit count of the padding goes in as (uint32)(len << 3) and (uint32)(len >> 29).  No GPU test reaches
 * len >= 2^29, where the high word is not zero: one lane walks its message alone at a few bytes per cycle, so such a message
 * would take seconds. */
int aivc_md5_batch(const uint8_t *const *msgs, int64_t len, int32_t n, uint8_t *digests, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_DIGEST_H */
