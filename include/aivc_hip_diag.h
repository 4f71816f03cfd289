/*
 * aivc_hip_diag.h -- a diagnostic of libaivc_hip.so for the tests and tools of the persistent kernels (conventions, types and
 * error codes: aivc_hip.h).  Nothing on the coded path calls it, and it has no `_ref` twin in the CPU oracle.
 *
 * What it is for: the Winograd kernels (aivc_amd/csrc/conv_wino.hip) take nearly all of a CU's LDS per workgroup, so a workgroup
 * starts only on a CU that holds no other LDS user, and in a codec step the entropy coders' kernels, which ask for 100 KB, are
 * such users on other streams.  tests/test_gpu_winograd_dynamic_walk.py and tools/bench_wino_beside_holder.py need one that
 * is there when they want it and gone after a bounded time.
 */
#ifndef AIVC_HIP_DIAG_H
#define AIVC_HIP_DIAG_H

#include "aivc_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One workgroup of 64 lanes that holds lds_bytes of LDS while every lane follows a chain of `iterations` dependent LDS reads
 * (a few hundred nanoseconds each), then writes where its chain ended to out[lane].  It waits for nothing: its duration is
 * bounded by `iterations` alone.
 *   lds_bytes   256 .. 160 KB, a multiple of 4
 *   iterations  1 .. 2^20
 *   out         device, 64 x uint32; every value is below lds_bytes / 4
 * Anything else: AIVC_ERR_ARG. */
int aivc_diag_hold_lds(uint32_t lds_bytes, uint32_t iterations, uint32_t *out, aivc_stream_t stream);

#ifdef __cplusplus
}
#endif

#endif /* AIVC_HIP_DIAG_H */
