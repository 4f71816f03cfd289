// reduce.h -- device helpers of the streaming passes (quality.hip, scene.hip, rate.hip, rawvideo.hip): exact 64-bit integer sums
// over a wave, a workgroup and a row of per-workgroup partials, the split of a byte range around its 16-byte aligned part, the
// byte funnel that reads 16 bytes at any address out of two aligned chunks, and the fixed fp64 tree of the rate and quality logs.  Integer sums do not depend on their grouping; the fp64 tree's order is part of the
// result (the CPU oracle walks the same one).
#pragma once
#include "common.h"

namespace aivc {

__device__ __forceinline__ uint64_t wave_sum_u64(uint64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += (uint64_t)__shfl_down((unsigned long long)v, s, 64);
  return v;  // (lane 0 holds the sum)
}

// the sum of acc over a workgroup of THREADS -> *dst (stored by thread 0): wave sums, then THREADS / 64 words of LDS
template <int THREADS>
__device__ __forceinline__ void block_partial_u64(uint64_t acc, uint64_t *dst) {
  __shared__ uint64_t wave_part[THREADS / 64];
  acc = wave_sum_u64(acc);
  if ((threadIdx.x & 63) == 0) wave_part[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint64_t s = 0;
    for (int k = 0; k < THREADS / 64; ++k) s += wave_part[k];
    *dst = s;
  }
}

// one wavefront per result: partials[r][0 .. BLOCKS) -> out[r]
template <int BLOCKS>
__global__ void __launch_bounds__(64) fold_partials_u64_kernel(const uint64_t *__restrict__ partials, uint64_t *__restrict__ out) {
  static_assert(BLOCKS % 64 == 0, "whole rounds of one partial per lane");
  uint64_t s = 0;
#pragma unroll
  for (int k = 0; k < BLOCKS; k += 64) s += partials[(size_t)blockIdx.x * BLOCKS + k + threadIdx.x];
  s = wave_sum_u64(s);
  if (threadIdx.x == 0) out[blockIdx.x] = s;
}

// The len bytes at a: [0, head) in front of a's first 16-byte boundary, nvec aligned 16-byte chunks, [tail0, len) behind them.
// bytewise: no 16-byte part, every byte lies outside it.
struct ByteSplit {
  size_t head, nvec, tail0, len;
  __device__ __forceinline__ ByteSplit(const uint8_t *a, size_t len_, bool bytewise = false) : len(len_) {
    head = (size_t)(-(uintptr_t)a & 15);
    if (bytewise || head > len) head = len;
    nvec = (len - head) / 16;
    tail0 = head + nvec * 16;
  }
  // thread t of T walks the bytes outside the 16-byte part: f(byte index)
  template <typename F>
  __device__ __forceinline__ void outside(size_t t, size_t T, F f) const {
    const size_t n_scalar = head + (len - tail0);
    for (size_t i = t; i < n_scalar; i += T) f(i < head ? i : tail0 + (i - head));
  }
};

typedef uint32_t chunk16_t __attribute__((ext_vector_type(4)));            // one aligned 16-byte chunk
typedef const chunk16_t __attribute__((address_space(1))) *chunk16_ptr;    // in global memory: global_load, not flat_load

// bytes s .. s + 15 of the 32 bytes {lo, hi}, 0 <= s < 16 (ws = s / 4, bs = s % 4; scene.hip: uniform over
// the workgroup, rawvideo.hip: the lane's own).  s = 0 gives lo.
__device__ __forceinline__ chunk16_t funnel16(const chunk16_t &lo, const chunk16_t &hi, uint32_t ws, uint32_t bs) {
  const uint32_t w[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t t[7];
#pragma unroll
  for (int j = 0; j < 7; ++j) t[j] = __builtin_amdgcn_alignbyte(w[j + 1], w[j], bs);  // ({hi, lo} >> 8 bs), low word
  chunk16_t r;
  r.x = ws == 0 ? t[0] : ws == 1 ? t[1] : ws == 2 ? t[2] : t[3];
  r.y = ws == 0 ? t[1] : ws == 1 ? t[2] : ws == 2 ? t[3] : t[4];
  r.z = ws == 0 ? t[2] : ws == 1 ? t[3] : ws == 2 ? t[4] : t[5];
  r.w = ws == 0 ? t[3] : ws == 1 ? t[4] : ws == 2 ? t[5] : t[6];
  return r;
}

// lanes[j] += lanes[j + s] for s = L/2, L/4, ..., 1 over the L = AIVC_RATE_LANES fixed lanes, by a workgroup of 1024: the sum
// is left in lanes[0] for every thread to read
__device__ __forceinline__ void fixed_tree_sum(double *lanes) {
  for (int s = AIVC_RATE_LANES / 2; s >= 1; s >>= 1) {
    for (int j = threadIdx.x; j < s; j += 1024) lanes[j] = lanes[j] + lanes[j + s];
    __syncthreads();
  }
}

}  // namespace aivc
