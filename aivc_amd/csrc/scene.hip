// scene.hip -- sums of absolute differences between consecutive luma planes of a clip (include/aivc_hip_scene.h): the one number
// per frame pair the encoder's scene-cut detection decides on (aivc_amd/scene.py).
//
// A streaming reduction, HBM-bound: four bytes per v_sad_u8 against 16-byte loads.  The grid runs over (stripe owner, pair):
// workgroup (bx, p) reads the stripes bx, bx + AIVC_SAD_BLOCKS, ... of planes p and p + 1.  The workgroups of a pair are dispatched
// together and pair p + 1 follows pair p, so the range of plane p + 1 that slot bx reads as a pair's FIRST plane was fetched as the
// previous pair's SECOND plane by the slot of the same number -- AIVC_SAD_BLOCKS is a multiple of the XCD count, so the same L2 --
// a pair earlier: the clip leaves HBM once, the second read is a cache's.  (The other design, a workgroup that owns a byte range and
// walks the frames with the previous frame's bytes in registers, reads every byte once by construction but has one workgroup per
// range for the whole clip: experiments/scene_cut.md.)
//
// Every sum is integer arithmetic, so the result depends on neither the grid nor the path a pair takes.
#include "reduce.h"
#include "../../include/aivc_hip_scene.h"

namespace aivc {

constexpr int SAD_THREADS = 256;
constexpr int SAD_UNROLL = 4;  // 16-byte chunks of each plane a thread has in flight: 1080p luma is one such round per thread

__device__ __forceinline__ uint32_t sad16(const chunk16_t &x, const chunk16_t &y, uint32_t acc) {  // adds <= 16 * 255
  acc = __builtin_amdgcn_sad_u8(x.x, y.x, acc);
  acc = __builtin_amdgcn_sad_u8(x.y, y.y, acc);
  acc = __builtin_amdgcn_sad_u8(x.z, y.z, acc);
  return __builtin_amdgcn_sad_u8(x.w, y.w, acc);
}

// The 16-byte part of a pair: chunks t, t + T, ... of va against the bytes shift .. of vb's chunks.  FUNNEL: shift != 0.
template <bool FUNNEL>
__device__ __forceinline__ uint64_t sad_chunks(chunk16_ptr va, chunk16_ptr vb, size_t nvec, size_t t, size_t T, uint32_t shift) {
  uint64_t acc = 0;
  const uint32_t ws = shift >> 2, bs = shift & 3u;
  for (size_t i0 = t; i0 < nvec; i0 += (size_t)SAD_UNROLL * T) {
    chunk16_t x[SAD_UNROLL], y[SAD_UNROLL], z[SAD_UNROLL];
#pragma unroll
    for (int k = 0; k < SAD_UNROLL; ++k) {  // every load of the round is issued before the first sum
      const size_t i = i0 + (size_t)k * T;
      const bool in = i < nvec;
      x[k] = y[k] = z[k] = chunk16_t{0u, 0u, 0u, 0u};
      if (in) {
        x[k] = va[i];
        y[k] = vb[i];
        if (FUNNEL) z[k] = vb[i + 1];  // holds byte 16 i + 15 of the second plane's part: inside the plane
      }
    }
    uint32_t s = 0;  // <= SAD_UNROLL * 16 * 255
#pragma unroll
    for (int k = 0; k < SAD_UNROLL; ++k) s = sad16(x[k], FUNNEL ? funnel16(y[k], z[k], ws, bs) : y[k], s);
    acc += s;
  }
  return acc;
}

// grid (AIVC_SAD_BLOCKS, n - 1): workgroup (bx, p) leaves the sum over its stripes of planes p and p + 1
__global__ void __launch_bounds__(SAD_THREADS) pair_sad_u8_kernel(const uint8_t *const *__restrict__ planes, size_t len,
                                                                  uint64_t *__restrict__ partials) {
  const uint8_t *a = planes[blockIdx.y], *b = planes[blockIdx.y + 1];
  const size_t t = (size_t)blockIdx.x * SAD_THREADS + threadIdx.x, T = (size_t)AIVC_SAD_BLOCKS * SAD_THREADS;
  const ByteSplit sp(a, len);
  const uint32_t shift = (uint32_t)((uintptr_t)(b + sp.head) & 15);  // where b's bytes lie in ITS aligned chunks: uniform
  chunk16_ptr va = (chunk16_ptr)(a + sp.head), vb = (chunk16_ptr)(b + sp.head - shift);
  uint64_t acc = shift == 0 ? sad_chunks<false>(va, vb, sp.nvec, t, T, 0) : sad_chunks<true>(va, vb, sp.nvec, t, T, shift);
  sp.outside(t, T, [&](size_t j) {
    const int d = (int)a[j] - (int)b[j];
    acc += (uint32_t)(d < 0 ? -d : d);
  });
  block_partial_u64<SAD_THREADS>(acc, partials + (size_t)blockIdx.y * AIVC_SAD_BLOCKS + blockIdx.x);
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_pair_sad_u8(const uint8_t *const *planes, int32_t n, int64_t len, uint64_t *partials, uint64_t *sad,
                                 aivc_stream_t stream) {
  if (n < 0) return AIVC_ERR_ARG;
  if (n <= 1) return AIVC_OK;
  if (!planes || !partials || !sad || len <= 0) return AIVC_ERR_ARG;
  if (n - 1 > 65535) return AIVC_ERR_UNSUPPORTED;  // grid.y
  hipLaunchKernelGGL(pair_sad_u8_kernel, dim3(AIVC_SAD_BLOCKS, n - 1), dim3(SAD_THREADS), 0, to_stream(stream), planes, (size_t)len,
                     partials);
  // one wavefront per pair: the AIVC_SAD_BLOCKS partials -> sad[p]
  hipLaunchKernelGGL(fold_partials_u64_kernel<AIVC_SAD_BLOCKS>, dim3(n - 1), dim3(64), 0, to_stream(stream), partials, sad);
  return check_launch("pair_sad_u8");
}
