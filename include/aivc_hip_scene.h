/*
 * aivc_hip_scene.h -- sums of absolute differences between consecutive luma planes of a clip (part of the C ABI of
 * libaivc_hip.so since ABI 24; conventions, types and error codes: aivc_hip.h).
 *
 * What it is for: the encoder's scene-cut detection (aivc_amd/scene.py).  The clip lies on the device as separate planes
 * (real_life.encode.read_yuv), one number per pair of consecutive frames travels to the host, and the decision and the unit
 * layout that follows from it are integer arithmetic there.  The reference has no counterpart: its encoder cuts a clip by
 * counting frames.
 *
 * The sums are exact integer arithmetic: they depend on neither the grid nor how a clip is batched, nor on the GPU or the
 * number of ranks, so every rank of a distributed encode derives the same layout from them without a collective.
 * This entry point has no `_ref` twin in the CPU oracle; its CPU statement is numpy (tests/test_gpu_pair_sad.py).
 */
#ifndef AIVC_HIP_SCENE_H
#define AIVC_HIP_SCENE_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* workgroups per pair of aivc_pair_sad_u8, and the 64-bit words of scratch it needs for n planes */
#define AIVC_SAD_BLOCKS 128
#define AIVC_SAD_SCRATCH_WORDS(n) ((n) > 1 ? ((size_t)(n) - 1) * AIVC_SAD_BLOCKS : (size_t)0)

/* sad[i] = sum over j < len of |planes[i + 1][j] - planes[i][j]|   for i = 0 ... n - 2.
 *   planes    device table of n device pointers (the table 8-byte aligned), each to len bytes: a luma plane as a flat
 *             buffer.  A pointer may have ANY alignment, and the alignments of one table may differ.
 *   len       bytes per plane, > 0.
 *   partials  AIVC_SAD_SCRATCH_WORDS(n) uint64 of scratch; sad: [n - 1] uint64.  Both 8-byte aligned.
 * Two launches, no atomics and no memset: AIVC_SAD_BLOCKS workgroups per pair leave one partial each (a workgroup owns every
 * AIVC_SAD_BLOCKS-th stripe of 256 16-byte chunks, the SAME stripes of the plane for every pair, so the second read of a
 * plane is the read of a range that the same workgroup slot fetched one pair earlier), then one wavefront per pair adds
 * them.  The totals are 64-bit (a pair of 16 843 010 bytes, all 0 against all 255, exceeds 2^32).
 * Loads: the first plane of a pair is read in aligned 16-byte chunks, the bytes in front of its first 16-byte boundary and
 * behind its last one by one.  Where the second plane shares that alignment it is read the same way; otherwise its bytes come
 * out of two aligned chunks through a byte funnel whose shift is uniform over the pair.  Only chunks that hold at least
 * one byte of a plane are read.  The path is chosen pair by pair, from the two pointers.
 * n <= 1 writes nothing and returns AIVC_OK.  AIVC_ERR_ARG: n < 0; with n > 1: len <= 0 or a NULL table, scratch or
 * output.  AIVC_ERR_UNSUPPORTED: n - 1 > 65535 (grid.y). */
int aivc_pair_sad_u8(const uint8_t *const *planes, int32_t n, int64_t len, uint64_t *partials, uint64_t *sad,
                     aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_SCENE_H */
