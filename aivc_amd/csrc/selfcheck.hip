// selfcheck.hip -- device-side check of the lean square root / division of the fused GDN epilogues (common.h) against
// the compiler's full IEEE sequences, and the element-by-element evaluator of the deterministic transcendentals
// (include/aivc_detmath.h) whose device bits the tests compare with the host's, and a workgroup that holds LDS for a bounded
// time (include/aivc_hip_diag.h).  Diagnostic entry points: nothing on the coded path calls them.
#include "common.h"

#include "../../include/aivc_hip_diag.h"

namespace aivc {

// every float in [GDN_SAFE_LO, GDN_SAFE_HI] (120 binades x 2^23 values): sqrt_rn_safe(s) == __builtin_sqrtf(s)
__global__ __launch_bounds__(256) void selfcheck_sqrt_kernel(uint32_t first, uint32_t last, unsigned long long *bad) {
  unsigned long long n = 0;
  for (uint64_t b = (uint64_t)first + (uint64_t)blockIdx.x * 256 + threadIdx.x; b <= last; b += (uint64_t)gridDim.x * 256) {
    const float s = __uint_as_float((uint32_t)b);
    n += __float_as_uint(sqrt_rn_safe(s)) != __float_as_uint(__builtin_sqrtf(s));
  }
  if (n) atomicAdd(bad, n);
}

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// random (numerator, denominator) pairs: numerators of either sign with |v| in [2^-60, 2^60], denominators the square
// roots' range [2^-30, 2^30]; every fourth pair shares the numerator's mantissa neighbourhood with the denominator's
// (quotients near 1 and near powers of two, where the last correction step decides the rounding)
__global__ __launch_bounds__(256) void selfcheck_div_kernel(uint64_t n_pairs, uint32_t seed, unsigned long long *bad) {
  unsigned long long n = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n_pairs; i += (uint64_t)gridDim.x * 256) {
    const uint64_t h = mix64(i + ((uint64_t)seed << 32) + 0x9E3779B97F4A7C15ull), h2 = mix64(h);
    const uint32_t ev = 127u - 60u + (uint32_t)((h >> 23) % 120u), ed = 127u - 30u + (uint32_t)((h2 >> 23) % 60u);
    uint32_t mv = (uint32_t)h & 0x7FFFFFu;
    const uint32_t md = (uint32_t)h2 & 0x7FFFFFu;
    if ((i & 3) == 3) mv = (md + (uint32_t)((h >> 50) & 7u) - 3u) & 0x7FFFFFu;
    const float v = __uint_as_float(((uint32_t)(h >> 63) << 31) | (ev << 23) | mv);
    const float d = __uint_as_float((ed << 23) | md);
    n += __float_as_uint(div_rn_safe(v, d)) != __float_as_uint(v / d);
  }
  if (n) atomicAdd(bad, n);
}

}  // namespace aivc

AIVC_EXPORT int aivc_selfcheck_gdn_math(uint64_t n_div_pairs, uint32_t seed, uint64_t *mismatch, aivc_stream_t stream) {
  if (!mismatch) return AIVC_ERR_ARG;
  hipStream_t s = aivc::to_stream(stream);
  if (hipMemsetAsync(mismatch, 0, 2 * sizeof(uint64_t), s) != hipSuccess) return aivc::check_launch("selfcheck memset");
  const uint32_t first = __builtin_bit_cast(uint32_t, aivc::GDN_SAFE_LO), last = __builtin_bit_cast(uint32_t, aivc::GDN_SAFE_HI);
  hipLaunchKernelGGL(aivc::selfcheck_sqrt_kernel, dim3(4096), dim3(256), 0, s, first, last, reinterpret_cast<unsigned long long *>(mismatch));
  if (n_div_pairs)
    hipLaunchKernelGGL(aivc::selfcheck_div_kernel, dim3(4096), dim3(256), 0, s, n_div_pairs, seed, reinterpret_cast<unsigned long long *>(mismatch) + 1);
  return aivc::check_launch("selfcheck_gdn_math");
}

namespace aivc {

// out[i] = fn(a[i] [, b[i]]) for one function of include/aivc_detmath.h: nothing but the header's own functions
template <typename T>
__global__ __launch_bounds__(256) void detmath_eval_kernel(int fn, const T *__restrict__ a, const T *__restrict__ b, size_t n, T *__restrict__ out) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    if constexpr (sizeof(T) == 8) {
      const double x = a[i];
      double r;
      switch (fn) {
        case AIVC_DETMATH_EXP: r = aivc_det_exp(x); break;
        case AIVC_DETMATH_EXPM1: r = aivc_det_expm1(x); break;
        case AIVC_DETMATH_LOG: r = aivc_det_log(x); break;
        default: r = aivc_det_log1p(x); break;
      }
      out[i] = r;
    } else {
      const float x = a[i];
      float r;
      switch (fn) {
        case AIVC_DETMATH_EXPF: r = aivc_expf_det(x); break;
        case AIVC_DETMATH_EXPM1F: r = aivc_expm1f_det(x); break;
        case AIVC_DETMATH_SIGMOIDF: r = aivc_sigmoidf_det(x); break;
        case AIVC_DETMATH_TANHF: r = aivc_tanhf_det(x); break;
        case AIVC_DETMATH_SOFTPLUSF: r = aivc_softplusf_det(x); break;
        case AIVC_DETMATH_POWF: r = aivc_powf_det(x, b[i]); break;
        default: r = aivc_laplace_cdf(x, b[i]); break;
      }
      out[i] = r;
    }
  }
}

}  // namespace aivc

AIVC_EXPORT int aivc_detmath_eval(int32_t fn, const void *a, const void *b, size_t n, void *out, aivc_stream_t stream) {
  if (fn < 0 || fn >= AIVC_DETMATH_COUNT) return AIVC_ERR_ARG;
  if (n == 0) return AIVC_OK;
  const bool two = fn == AIVC_DETMATH_POWF || fn == AIVC_DETMATH_LAPLACE_CDF;
  if (!a || !out || (two && !b)) return AIVC_ERR_ARG;
  hipStream_t s = aivc::to_stream(stream);
  const unsigned blocks = aivc::cdiv(n, 256) < 8192u ? aivc::cdiv(n, 256) : 8192u;
  if (fn <= AIVC_DETMATH_LOG1P)
    hipLaunchKernelGGL(aivc::detmath_eval_kernel<double>, dim3(blocks), dim3(256), 0, s, (int)fn, static_cast<const double *>(a),
                       static_cast<const double *>(b), n, static_cast<double *>(out));
  else
    hipLaunchKernelGGL(aivc::detmath_eval_kernel<float>, dim3(blocks), dim3(256), 0, s, (int)fn, static_cast<const float *>(a),
                       static_cast<const float *>(b), n, static_cast<float *>(out));
  return aivc::check_launch("detmath_eval");
}

namespace aivc {

// one workgroup, `words` uint32 of LDS: held[i] = i, then every lane follows held[] for `iterations` dependent reads (each index
// is reduced below `words` before it is used)
__global__ __launch_bounds__(64) void hold_lds_kernel(uint32_t words, uint32_t iterations, uint32_t *__restrict__ out) {
  extern __shared__ uint32_t held[];
  for (uint32_t i = threadIdx.x; i < words; i += 64u) held[i] = i;
  __syncthreads();
  uint32_t at = threadIdx.x % words;
  for (uint32_t k = 0; k < iterations; ++k) at = (held[at] * 2654435761u + k) % words;
  out[threadIdx.x] = at;
}

}  // namespace aivc

AIVC_EXPORT int aivc_diag_hold_lds(uint32_t lds_bytes, uint32_t iterations, uint32_t *out, aivc_stream_t stream) {
  if (!out || lds_bytes < 256u || lds_bytes > 160u * 1024u || (lds_bytes & 3u) || iterations < 1u || iterations > (1u << 20)) return AIVC_ERR_ARG;
  static aivc::LdsOptIn opt_in;
  if (!opt_in.raise(reinterpret_cast<const void *>(aivc::hold_lds_kernel), 160u * 1024u)) return aivc::check_launch("diag_hold_lds lds attribute");
  hipLaunchKernelGGL(aivc::hold_lds_kernel, dim3(1), dim3(64), lds_bytes, aivc::to_stream(stream), lds_bytes / 4u, iterations, out);
  return aivc::check_launch("diag_hold_lds");
}
