// conv_bf16x3.hip -- the bf16x3 precision mode (aivc_conv_params.precision = 1): dispatch over the PREC 1 / 2 instantiations of
// conv_mfma_kernel (conv_mfma_kernel.h) and the kernel that splits weights ahead of a launch.
#include "conv_mfma_kernel.h"

namespace aivc {

// The precision mode covers the layers that carry the FLOPs: conv / transposed conv with c_in % 32 == 0 and c_out of 64
// or a multiple of 128, with or without fused (I)GDN (its second GEMM stays fp32), no fused 1x1 tail.  Wave tile 64x64
// (128x128 / 256x64 workgroup tiles): the six products of a 64x64x16 slab are 24 MFMAs of 32 cycles against ~180 vector
// instructions of operand splitting -- smaller wave tiles are bound by the splitting.
bool conv2d_bf16x3_supported(const aivc_conv_params &p) {
  if (p.mode != AIVC_MODE_CONV && p.mode != AIVC_MODE_TCONV) return false;
  if (p.c_in % BK != 0) return false;
  // fused 1x1 tail (its GEMM stays fp32, like the fused GDN's): the bottleneck blocks' 3x3 64 -> 64 + 1x1 64 -> 128
  if (p.tail_c_out && (p.tail_c_out != TAIL_N || p.c_out != 64 || p.mode != AIVC_MODE_CONV || p.gdn || p.mul || !p.bias || !p.tail_bias)) return false;
  if (p.c_out != 64 && p.c_out % 128 != 0) return false;
  if (p.gdn && p.c_out != 64 && p.c_out != 128) return false;
  // short reductions (the 1x1 convs: two to four K tiles) are prologue / epilogue work on the mode's big tiles: they stay
  // on the fp32 kernels' small tiles (measured: 109-121 TFLOP/s fp32-equivalent against 125-133 there)
  const int taps = p.mode == AIVC_MODE_TCONV ? (p.ksize * p.ksize + 3) / 4 : p.ksize * p.ksize;
  if (taps * p.c_in < 512) return false;
  if ((uint64_t)p.ksize * p.ksize * p.c_in >= 65536ull) return false;
  // one image and the weights inside the loader's 32-bit byte offsets
  return loader_addressable((uint64_t)p.h_in * p.w_in * p.c_in * 4ull) && loader_addressable((uint64_t)p.c_out * p.ksize * p.ksize * p.c_in * 4ull);
}

// weights split ahead of the launch (aivc_split_weights_bf16x3) or by the K loop: the same terms, the same bits
static bool split_ahead(const aivc_conv_params &p) {
  return p.w_bf16x3 != nullptr && loader_addressable((uint64_t)p.c_out * p.ksize * p.ksize * p.c_in * 6ull);
}

// Tile of a launch of the mode (ids of TILE_MENU).  Weights
// split in the K loop: wave tile 64x64 (the split is 44 vector instructions per fragment: smaller wave tiles are bound
// by it).  Weights split ahead (w_bf16x3): measured per layer class on the bench's shapes (tools/bf16x3_probe.py,
// TFLOP/s fp32-equivalent, in-loop | 64x64 wave tile | 32x64 wave tile): conv to 128 channels 163-181 | 174-204 | 161-182,
// conv to 64 160 | 162 | 173, transposed to 128 153 | 153 | 162, transposed to 64 149 | 139 | 151 (the 256x64 tile's ring
// grows to 88 KB with the three weight planes: one workgroup per CU).
int conv2d_bf16x3_tile(const aivc_conv_params &p) {
  static const int force = getenv("AIVC_BF16X3_TILE") ? atoi(getenv("AIVC_BF16X3_TILE")) : 0;  // tuning aid: 1 = wave tile 64x64 everywhere
  if (p.tail_c_out) return 6;  // fused tail: 128x64 either way (64 rows of 128 tail channels per wave would not fit the registers)
  if (!split_ahead(p) || force == 1) return p.c_out == 64 ? 2 : 0;
  if (p.c_out == 64) return 6;
  return p.mode == AIVC_MODE_TCONV ? 5 : 0;
}

// The mode's tiles are those of TILE_MENU, except that its 128x64 stacks the four waves along M (wave tile 32x64).
constexpr ConvTile bf16x3_tile(int id) { return id == 6 ? ConvTile{6, 4, 1, 1, 2, false} : TILE_MENU[tile_index(id)]; }

// one tile of the mode, with or without fused (I)GDN
template <int MODE, int PREC, int ID>
static int launch_bf16x3_tile(const aivc_conv_params &p, hipStream_t s) {
  constexpr ConvTile t = bf16x3_tile(ID);
  return p.gdn ? launch_cfg2<MODE, t.wm, t.wn, t.tm, t.tn, true, true, false, PREC>(p, s)
               : launch_cfg2<MODE, t.wm, t.wn, t.tm, t.tn, false, true, false, PREC>(p, s);
}

template <int MODE, int PREC>
static int launch_bf16x3_prec(const aivc_conv_params &p, hipStream_t s) {
  if constexpr (MODE == AIVC_MODE_CONV) {
    constexpr ConvTile t = bf16x3_tile(6);
    if (p.tail_c_out) return launch_cfg2<MODE, t.wm, t.wn, t.tm, t.tn, false, true, true, PREC>(p, s);
  }
  const int tile = conv2d_bf16x3_tile(p);
  if constexpr (PREC == 2) {  // the 32x64 wave tiles: instantiated for weights split ahead only
    if (tile == 6) return launch_bf16x3_tile<MODE, 2, 6>(p, s);
    if (tile == 5) return launch_bf16x3_tile<MODE, 2, 5>(p, s);
  }
  return tile == 2 ? launch_bf16x3_tile<MODE, PREC, 2>(p, s) : launch_bf16x3_tile<MODE, PREC, 0>(p, s);
}

template <int MODE>
static int launch_bf16x3(const aivc_conv_params &p, hipStream_t s) {
  return split_ahead(p) ? launch_bf16x3_prec<MODE, 2>(p, s) : launch_bf16x3_prec<MODE, 1>(p, s);
}

__global__ __launch_bounds__(256) void split_weights_kernel(const float *__restrict__ w, size_t pairs, int k_total, uint32_t *__restrict__ out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;  // pair (k, k + 1) of one row
  if (i >= pairs) return;
  const size_t half = (size_t)k_total / 2, co = i / half;
  const int k = 2 * (int)(i - co * half);
  const float2 x = *reinterpret_cast<const float2 *>(w + 2 * i);
  uint32_t h, m, l;
  bf16x3_split2(x.x, x.y, h, m, l);
  uint32_t *dst = out + ((co * (size_t)(k_total / 32) + (size_t)(k / 32)) * 3) * 16 + (size_t)((k % 32) / 2);
  dst[0] = h;
  dst[16] = m;
  dst[32] = l;
}

int split_weights_bf16x3(const float *w, int c_out, int k_total, void *out, hipStream_t s) {
  const size_t pairs = (size_t)c_out * (size_t)k_total / 2;
  hipLaunchKernelGGL(split_weights_kernel, dim3((unsigned)((pairs + 255) / 256)), dim3(256), 0, s, w, pairs, k_total, reinterpret_cast<uint32_t *>(out));
  return check_launch("split_weights_bf16x3");
}

int conv2d_bf16x3(const aivc_conv_params &p, hipStream_t s) {
  if (!conv2d_bf16x3_supported(p)) return AIVC_ERR_UNSUPPORTED;
  return for_sub_batches(p, [&](const aivc_conv_params &q) {
    return p.mode == AIVC_MODE_CONV ? launch_bf16x3<AIVC_MODE_CONV>(q, s) : launch_bf16x3<AIVC_MODE_TCONV>(q, s);
  });
}

}  // namespace aivc
