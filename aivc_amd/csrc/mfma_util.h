// mfma_util.h -- device helpers shared by the matrix-core kernels (conv_mfma_kernel.h, conv_wino.hip, gdn.hip,
// conv_images.hip): each defined once.
#pragma once
#include <type_traits>

#include "common.h"

namespace aivc {

typedef float floatx16 __attribute__((ext_vector_type(16)));  // accumulator block of a 32x32 MFMA

// LDS-DMA of 16 bytes per lane (global_load_lds_dwordx4): LDS destination = lds_dst (wave-uniform, through M0) +
// lane * 16, source = base (SGPR pair) + voff (per-lane byte offset).  Counts on vmcnt like a load; no VGPR result.
__device__ __forceinline__ void glds16(const float *base, uint32_t voff, uint32_t lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" : : "v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
}

// LDS-DMA of a contiguous 4 KB piece (256 slots of 16 bytes, slot s of instruction k = 64 k + lane), or of its lower / upper
// half: up to four instructions off ONE M0 -- the instruction offset advances the global and the LDS address alike.
enum GldsPiece { GLDS_BOTH, GLDS_LO, GLDS_HI };
template <GldsPiece PIECE>
__device__ __forceinline__ void glds_piece(const float *base, uint32_t voff, uint32_t lds_dst) {
  if constexpr (PIECE == GLDS_BOTH)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:1024\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:3072"
                 : : "v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
  else if constexpr (PIECE == GLDS_LO)
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:1024"
                 : : "v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
  else
    asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:2048\n\t"
                 "global_load_lds_dwordx4 %0, %1 offset:3072"
                 : : "v"(voff), "s"(base), "s"(lds_dst) : "memory", "m0");
}

// NONE / LEAKY / RELU of act_apply() without branches
__device__ __forceinline__ float act_cheap(int act, float v) {
  const float neg = act == AIVC_ACT_LEAKY ? v * 0.01f : (act == AIVC_ACT_RELU ? 0.0f : v);
  return v > 0.0f ? v : neg;
}

// One octet of a reduction on v_mfma_f32_32x32x2_f32: af[i] / bf[j] hold the lane's four consecutive k of row block i /
// column block j (lane half h: k = 8 o + 4 h ..), step S multiplies component S -- AIVC_K_ORDER over the octet's four steps.
template <int S>
__device__ __forceinline__ float f4_at(const float4 &v) {
  if constexpr (S == 0) return v.x;
  else if constexpr (S == 1) return v.y;
  else if constexpr (S == 2) return v.z;
  else return v.w;
}
template <int S, int TM, int TN>
__device__ __forceinline__ void mfma_oct_step(const float4 (&af)[TM], const float4 (&bf)[TN], floatx16 (&c)[TM][TN]) {
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) c[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(f4_at<S>(af[i]), f4_at<S>(bf[j]), c[i][j], 0, 0, 0);
}
// the four steps on ONE accumulator block, in a row
__device__ __forceinline__ floatx16 mfma_oct1(const float4 &a, const float4 &b, floatx16 c) {
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.x, b.x, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.y, b.y, c, 0, 0, 0);
  c = __builtin_amdgcn_mfma_f32_32x32x2f32(a.z, b.z, c, 0, 0, 0);
  return __builtin_amdgcn_mfma_f32_32x32x2f32(a.w, b.w, c, 0, 0, 0);
}
// the four steps; skip3 (wave-uniform) leaves out step 3 where k % 4 == 3 multiplies a zero (AIVC_CONV_SPARSE4)
template <int TM, int TN>
__device__ __forceinline__ void mfma_oct(const float4 (&af)[TM], const float4 (&bf)[TN], floatx16 (&c)[TM][TN], bool skip3 = false) {
  mfma_oct_step<0>(af, bf, c);
  mfma_oct_step<1>(af, bf, c);
  mfma_oct_step<2>(af, bf, c);
  if (!skip3) mfma_oct_step<3>(af, bf, c);
}

}  // namespace aivc
