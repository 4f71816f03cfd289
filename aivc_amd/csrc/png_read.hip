// png_read.hip -- reading PNG pictures: a batched zlib inflate and the inverse of the row filters (include/aivc_hip_png_read.h,
// where the tables, the statuses and the guarantees are stated).
//
// inflate_kernel: a workgroup of ONE wavefront per stream runs inflate_core.h -- the text a host program runs under the
// sanitizers (tools/inflate_host.cpp) -- with its State in LDS: the 32 KiB window of deflate as a ring (a match never reads
// global memory the wave has just written), 4 KiB of the source at a time, a primary lookup table per code (10 bits for
// literals and lengths, 8 for distances; a longer code walks the canonical counts), about 40 KiB in all, so four streams share
// a CU.  Symbol decoding is the same in every lane (readfirstlane where a value comes out of LDS); the lanes share out the
// source window, the tables (a ballot ranks the symbols of a length), match copies and the flush of the ring to dst, where
// the Adler sums accumulate.
// png_unfilter_kernel: a wavefront per picture.  Lane k takes row r0 + k of a band of 64 rows, one pixel behind lane k - 1, so
// the bytes above and above-left come from that lane by a shuffle; the next residual is loaded a step ahead.  Lane 0 reads
// the row above from pix: the last row of the band before, made visible by a fence and a barrier between bands.
#include "reduce.h"
#include "inflate_core.h"
#include "../../include/aivc_hip_png_read.h"

namespace aivc {

namespace inf = inflate_core;
static_assert(inf::ST_OK == AIVC_INFLATE_OK && inf::ST_SRC_EXHAUSTED == AIVC_INFLATE_SRC_EXHAUSTED && inf::ST_BAD_HEADER == AIVC_INFLATE_BAD_HEADER &&
              inf::ST_BAD_BLOCK_TYPE == AIVC_INFLATE_BAD_BLOCK_TYPE && inf::ST_STORED_MISMATCH == AIVC_INFLATE_STORED_MISMATCH &&
              inf::ST_BAD_LENGTHS == AIVC_INFLATE_BAD_LENGTHS && inf::ST_BAD_SYMBOL == AIVC_INFLATE_BAD_SYMBOL &&
              inf::ST_BAD_DISTANCE == AIVC_INFLATE_BAD_DISTANCE && inf::ST_TOO_LONG == AIVC_INFLATE_TOO_LONG &&
              inf::ST_TOO_SHORT == AIVC_INFLATE_TOO_SHORT && inf::ST_BAD_ADLER == AIVC_INFLATE_BAD_ADLER &&
              inf::ST_TOO_LARGE == AIVC_INFLATE_TOO_LARGE, "the statuses of the header are the core's");
static_assert(sizeof(inf::State) <= 40 * 1024 + 256, "four streams to a CU");

struct WaveEnv {  // a workgroup that is one wavefront
  static __device__ __forceinline__ uint32_t lane() { return threadIdx.x; }
  static __device__ __forceinline__ constexpr uint32_t lanes() { return 64; }
  static __device__ __forceinline__ void sync() { __syncthreads(); }
  static __device__ __forceinline__ uint32_t uniform(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
  static __device__ __forceinline__ uint64_t ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
  static __device__ __forceinline__ uint64_t sum(uint64_t v) {
    v = wave_sum_u64(v);
    return ((uint64_t)uniform((uint32_t)(v >> 32)) << 32) | uniform((uint32_t)v);
  }
};

__global__ void __launch_bounds__(64) inflate_kernel(const uint8_t *src, const uint64_t *__restrict__ table, uint8_t *dst, uint32_t *info) {
  __shared__ inf::State S;
  const size_t k = blockIdx.x;
  const uint64_t src_off = table[4 * k], src_n = table[4 * k + 1], dst_off = table[4 * k + 2], dst_n = table[4 * k + 3];
  uint32_t status = inf::ST_TOO_LARGE, produced = 0, consumed = 0;
  if (src_n < (1ull << 31) && dst_n < (1ull << 31))
    status = inf::inflate_stream<WaveEnv>(S, src + src_off, (uint32_t)src_n, dst + dst_off, (uint32_t)dst_n, produced, consumed);
  if (threadIdx.x == 0) info[4 * k] = status, info[4 * k + 1] = produced, info[4 * k + 2] = consumed, info[4 * k + 3] = 0;
}

// ---- the filters, undone ----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t unfilter_pred(uint32_t type, uint32_t a, uint32_t b, uint32_t d) {
  const int p = (int)a + (int)b - (int)d;
  const int pa = p > (int)a ? p - (int)a : (int)a - p, pb = p > (int)b ? p - (int)b : (int)b - p, pd = p > (int)d ? p - (int)d : (int)d - p;
  const uint32_t paeth = pa <= pb && pa <= pd ? a : pb <= pd ? b : d;
  return type == 0 ? 0u : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth;
}

// one picture by one wavefront -> whether a type byte above 4 was met
template <int C>
__device__ __forceinline__ bool unfilter_picture(const uint8_t *filt, uint8_t *pix, int64_t h, int64_t w) {
  const int lane = threadIdx.x;
  const int64_t rb = w * C;
  bool bad = false;
  for (int64_t r0 = 0; r0 < h; r0 += 64) {
    const int64_t row = r0 + lane;
    const bool active = row < h;
    const int64_t rows = h - r0 < 64 ? h - r0 : 64;
    const uint8_t *in = filt + (active ? row : r0) * (rb + 1) + 1;  // the row's residuals (an idle lane points at a row of the picture)
    uint8_t *out = pix + (active ? row : r0) * rb;
    const bool has_up = active && row > 0;
    const uint8_t *up = out - (has_up ? rb : 0);
    uint32_t type = active ? in[-1] : 0u;
    if (type > 4u) bad = true, type = 0u;
    uint32_t a[C], d[C], f[C], above[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) a[ch] = 0, d[ch] = 0, f[ch] = 0, above[ch] = 0;
    if (active && lane == 0) {  // what lane 0 needs at step 0
#pragma unroll
      for (int ch = 0; ch < C; ++ch) f[ch] = in[ch], above[ch] = has_up ? up[ch] : 0u;
    }
    const int64_t steps = w + rows - 1;
    for (int64_t t = 0; t < steps; ++t) {
      const int64_t x = t - lane;  // this lane's pixel of the step; lane - 1 made pixel x of the row above in step t - 1
      const bool now = active && x >= 0 && x < w, next = active && x + 1 >= 0 && x + 1 < w;
      uint32_t fn[C], an[C], from_lane[C];
#pragma unroll
      for (int ch = 0; ch < C; ++ch) {
        from_lane[ch] = (uint32_t)__shfl_up((int)a[ch], 1, 64);  // (a: the lane's last pixel)
        fn[ch] = next ? in[(x + 1) * C + ch] : 0u;
        an[ch] = next && lane == 0 && has_up ? up[(x + 1) * C + ch] : 0u;
      }
      if (now) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) {
          const uint32_t b = lane == 0 ? above[ch] : from_lane[ch];
          const uint32_t v = (f[ch] + unfilter_pred(type, x > 0 ? a[ch] : 0u, b, x > 0 ? d[ch] : 0u)) & 255u;
          out[x * C + ch] = (uint8_t)v;
          a[ch] = v, d[ch] = b;
        }
      }
#pragma unroll
      for (int ch = 0; ch < C; ++ch) f[ch] = fn[ch], above[ch] = an[ch];
    }
    __threadfence();  // the band's last row is the next band's row above
    __syncthreads();
  }
  return bad;
}

__global__ void __launch_bounds__(64) png_unfilter_kernel(const uint8_t *filt, const uint64_t *__restrict__ table, uint8_t *pix, uint32_t *status) {
  const size_t k = blockIdx.x;
  const uint64_t filt_off = table[4 * k], pix_off = table[4 * k + 1], hw = table[4 * k + 2], c = table[4 * k + 3];
  const uint64_t h = hw >> 32, w = hw & 0xffffffffull;
  uint32_t st = AIVC_PNG_UNFILTER_BAD_SHAPE;
  if (h >= 1 && w >= 1 && (c == 1 || c == 3) && 1 + w * c < (1ull << 31) && h * (1 + w * c) < (1ull << 31)) {  // (h < 2^32, a row < 2^31: no wrap)
    const bool bad = c == 1 ? unfilter_picture<1>(filt + filt_off, pix + pix_off, (int64_t)h, (int64_t)w)
                            : unfilter_picture<3>(filt + filt_off, pix + pix_off, (int64_t)h, (int64_t)w);
    st = __builtin_amdgcn_ballot_w64(bad) ? AIVC_PNG_UNFILTER_BAD_TYPE : AIVC_PNG_UNFILTER_OK;
  }
  if (threadIdx.x == 0) status[k] = st;
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_inflate(const uint8_t *src, const uint64_t *table, int32_t n, uint64_t max_src_bytes, uint64_t max_dst_bytes,
                             uint8_t *dst, uint32_t *info, aivc_stream_t stream) {
  if (!src || !table || !dst || !info || n < 1) return AIVC_ERR_ARG;
  if (max_src_bytes >= (1ull << 31) || max_dst_bytes >= (1ull << 31)) return AIVC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(inflate_kernel, dim3((unsigned)n), dim3(64), 0, to_stream(stream), src, table, dst, info);
  return check_launch("inflate");
}

AIVC_EXPORT int aivc_png_unfilter(const uint8_t *filt, const uint64_t *table, int32_t n, uint64_t max_bytes, uint8_t *pix, uint32_t *status,
                                  aivc_stream_t stream) {
  if (!filt || !table || !pix || !status || n < 1) return AIVC_ERR_ARG;
  if (max_bytes >= (1ull << 31)) return AIVC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)n), dim3(64), 0, to_stream(stream), filt, table, pix, status);
  return check_launch("png_unfilter");
}
