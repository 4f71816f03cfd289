// conv_mfma.hip -- fp32 dispatch of the implicit-GEMM convolution family (kernel: conv_mfma_kernel.h): the tile rules,
// what the kernels can address, sub-batching beyond 4 GB.
#include <utility>

#include "conv_mfma_kernel.h"

namespace aivc {

// one tile of the menu: the reduction is a run of whole K tiles (c_in % 32 == 0) or generic
template <int MODE, int T, bool FUSE>
static int launch_cfg(const aivc_conv_params &p, hipStream_t s) {
  constexpr ConvTile t = TILE_MENU[T];
  if (p.c_in % BK == 0) return launch_cfg2<MODE, t.wm, t.wn, t.tm, t.tn, FUSE, true>(p, s);
  if constexpr (!t.generic_k) return AIVC_ERR_UNSUPPORTED;  // pick_tile never sends a generic reduction here
  else return launch_cfg2<MODE, t.wm, t.wn, t.tm, t.tn, FUSE, false>(p, s);
}

static int pick_tile_auto(const aivc_conv_params &p);
static int pick_tile(const aivc_conv_params &p) {
  // tuning aid: AIVC_FORCE_TILE=<id of TILE_MENU> overrides the choice when that tile can run the shape
  if (const char *e = getenv("AIVC_FORCE_TILE")) {
    const int i = tile_index(atoi(e));
    if (i >= 0 && (TILE_MENU[i].generic_k || p.c_in % BK == 0) && (!p.gdn || TILE_MENU[i].bn() == p.c_out)) return TILE_MENU[i].id;
  }
  return pick_tile_auto(p);
}
static int pick_tile_auto(const aivc_conv_params &p) {
  const bool t = p.mode == AIVC_MODE_TCONV;
  const long M = t ? (long)p.n * p.h_in * p.w_in : (long)p.n * p.h_out * p.w_out;
  const int z = t ? 4 : 1;
  const int co = p.c_out;
  auto blocks = [&](int bm, int bn) { return ((M + bm - 1) / bm) * ((co + bn - 1) / bn) * z; };
  const int taps = t ? (p.ksize * p.ksize + 3) / 4 : p.ksize * p.ksize;
  const long kred = (long)taps * p.c_in;
  // Measured on MI355X (tools/bench_conv.py, batch 8): every tile saturates at 105-117 TFLOP/s on
  // long reductions; what differs is how well short reductions / few blocks are hidden, where
  // the small 64x64 tile (6 workgroups per CU) wins.  Rules:
  //   c_out <= 64            -> 64x64 (also with fused GDN: BN == c_out)
  //   c_out  = 32            -> 128x32
  //   fused GDN, c_out = 128 -> 128x128, or 64x128 for the short reductions of a transposed 3x3
  //   otherwise score the candidates by efficiency class x block-count balance
  if (co <= 32) return 3;
  // attention gates (sigmoid): their per-output pass wants many small tiles (16 outputs per thread)
  if ((p.act1 == AIVC_ACT_SIGMOID || p.act2 == AIVC_ACT_SIGMOID) && !p.gdn) return 1;
  // c_out = 64: 256x64 (four waves stacked along M, 4 accumulators each) once there are >= ~1000 such tiles and
  // the reduction is long; else the small tile (r02 sweep, tools/_tile_sweep.sh: 109 vs 107, 94 vs 91 TFLOP/s)
  // 128x64 (id 6: 126 registers, four waves per SIMD) is ahead where the epilogue weighs most against a short or
  // loader-heavy reduction: the image layers (c_in of 4 / 8 / 12), 1x1 and stride-2 convs (r02: 4080 vs 4232 us,
  // 114 vs 119, 548 vs 582); transposed convs and the 3x3 stay on 256x64 / 64x64
  // Round 3, LDS-DMA loop (c_in % 32 == 0; tools/bench_conv.py with AIVC_FORCE_TILE, same box): 64x128 (three
  // workgroups per CU: 48 KB of ring, <= 172 registers) beats 128x128 (two) wherever BN = 128 fits -- 5x5 s2 64->128
  // + GDN 135.3 -> 137.8, 3x3 128->128 138.4 -> 140.3 (+ GDN 131.9 -> 133.5), transposed 5x5 128->128 122.6 -> 132.9
  // (+ GDN 114.6 -> 127.4), transposed 3x3 115.0 -> 118.5 TFLOP/s; for c_out = 64 the transposed 5x5 + GDN runs
  // 121.5 on 256x64, 125.1 on 128x64, 125.6 on 64x64.
  if (p.c_in % BK == 0 && (p.mode == AIVC_MODE_CONV || t)) {
    // Round 4: few tiles (a single frame's 1/16-resolution layers: 8160 pixels = 128 tiles of 64x128 for 256 CUs): the 64x64
    // tile doubles the workgroup count -- 3x3 128->128 at 68x120, batch 1: 53 -> 90 TFLOP/s, transposed 5x5 94 -> 104, equal
    // from ~512 tiles on (tools/_ab_tiles_n4.sh at BATCH=1 / 4).  Not with a fused GDN (its tile must hold all channels).
    if (co % 128 == 0) return (!p.gdn && blocks(64, 128) <= 512) ? 1 : 5;
    if (co <= 64 && t) return 1;
  }
  if (co <= 64 && !t && M >= 65536 && (p.c_in % BK != 0 || p.ksize == 1 || p.stride == 2)) return 6;
  if (co <= 64) return (M >= 250000 && kred >= 96 && p.c_in % BK == 0) ? 2 : 1;
  if (p.gdn) return (t && p.ksize == 3) ? 5 : 0;  // BN must equal c_out = 128
  // c_out above 64 that is no multiple of 128 (models of other widths: 96, 144, 192 ...; round 6, bench.py --widths): the
  // score also counts the columns a tile pads -- 192 channels are 1.5 tiles of 128 (a quarter of the matrix work wasted)
  // but exactly three of 64 -- and the 64-column tiles with four accumulators per wave (256x64 / 128x64) and the 64x128
  // LDS-DMA tile join the candidates.
  auto score = [&](int bm, int bn, int slots, double base) {
    const long b = blocks(bm, bn);
    const long rounds = (b + slots - 1) / slots;
    const double cols = (double)co / (double)(((co + bn - 1) / bn) * bn);
    return base * cols * (double)b / (double)(rounds * slots);
  };
  // stand-alone (I)GDN launch (K = C: bound by its memory traffic): with 128 channels the 128-column tile reads the input
  // once as the GEMM operand instead of once per 64-column tile (round 6: the second launch of a Winograd-covered layer,
  // 4.0 -> see experiments/r06.md)
  if (p.mode == AIVC_MODE_GDN || p.mode == AIVC_MODE_IGDN) return co == 128 ? 5 : 1;
  double best = score(128, 128, 512, 0.80);  // 176 registers: two workgroups per CU
  int tile = 0;
  const double s1 = score(64, 64, 1536, kred <= 256 ? 0.85 : 0.74);
  if (s1 > best) best = s1, tile = 1;
  if ((t && p.ksize == 3) || (p.c_in % BK == 0 && co % 128 != 0)) {
    const double s5 = score(64, 128, 1024, t && p.ksize == 3 ? 0.75 : 0.80);
    if (s5 > best) best = s5, tile = 5;
  }
  if (co % 128 != 0) {
    const double s6 = score(128, 64, 1024, 0.76);
    if (s6 > best) best = s6, tile = 6;
    if (p.c_in % BK == 0) {
      const double s2 = score(256, 64, 512, 0.78);
      if (s2 > best) best = s2, tile = 2;
    }
  }
  return tile;
}

// the ladder over TILE_MENU: every tile, with and without fused (I)GDN (the GDN mode itself has nothing to fuse)
template <int MODE, bool FUSE, int... T>
static int launch_tile(int tile, const aivc_conv_params &p, hipStream_t s, std::integer_sequence<int, T...>) {
  int rc = AIVC_ERR_UNSUPPORTED;
  (void)((TILE_MENU[T].id == tile && ((rc = launch_cfg<MODE, T, FUSE>(p, s)), true)) || ...);
  return rc;
}
template <int MODE>
static int launch_mode(const aivc_conv_params &p, hipStream_t s) {
  constexpr auto menu = std::make_integer_sequence<int, N_TILES>();
  if constexpr (MODE != AIVC_MODE_GDN) {
    if (p.gdn) return launch_tile<MODE, true>(pick_tile(p), p, s, menu);
  }
  return launch_tile<MODE, false>(pick_tile(p), p, s, menu);
}

// fused 1x1 tail: a conv with c_out = 64 (one 128x64 tile owns every channel of its pixels), TAIL_N tail channels,
// bias on both, cheap activations
bool conv2d_mfma_tail_supported(const aivc_conv_params &p) {
  return p.mode == AIVC_MODE_CONV && !p.gdn && !p.mul && p.c_out == 64 && p.tail_c_out == TAIL_N && p.c_in % BK == 0 &&
         p.bias && p.tail_bias && p.tail_w && p.act1 != AIVC_ACT_SIGMOID && p.act2 != AIVC_ACT_SIGMOID &&
         conv2d_mfma_supported(p);
}

int conv2d_mfma_variant(const aivc_conv_params &p) {
  if (p.tail_c_out) return 190;
  const int mode = p.mode == AIVC_MODE_TCONV ? 1 : (p.mode == AIVC_MODE_CONV ? 0 : 2);
  return 100 + 10 * mode + pick_tile(p) + (p.gdn ? 50 : 0);
}

// what the kernels can index and address (ALGO_MFMA is held to this too)
bool conv2d_mfma_addressable(const aivc_conv_params &p) {
  // 32-bit element offsets inside the kernel
  const uint64_t in_elems = (uint64_t)p.n * p.h_in * p.w_in * p.c_in;
  const uint64_t w_elems = (uint64_t)p.c_out * p.ksize * p.ksize * p.c_in;
  if (in_elems >= 0xFFFFFFFFull || w_elems >= 0xFFFFFFFFull) return false;
  if ((uint64_t)p.ksize * p.ksize * p.c_in >= 65536ull) return false;
  // the LDS-DMA loop's 32-bit BYTE offsets: ONE image's input (a larger batch goes out as sub-batches) and the weights.
  // These modes have no other MFMA loop: the router sends a larger tensor to the scalar kernel.  No codec tensor comes
  // near (an 8K frame's half-resolution 64-channel map is 2.1 GB).
  if (lds_dma_loop(p.mode, p.c_in % BK == 0) &&
      !(loader_addressable((uint64_t)p.h_in * p.w_in * p.c_in * 4ull) && loader_addressable(w_elems * 4ull)))
    return false;
  return true;
}

bool conv2d_mfma_supported(const aivc_conv_params &p) {
  if (p.gdn && p.c_out != 32 && p.c_out != 64 && p.c_out != 128) return false;
  // thin outputs (c_out of 3 / 6): N is padded to 32, still ~6x faster than the scalar kernel once
  // the reduction is long; tiny reductions stay scalar
  if (p.c_out < 16 && p.c_in * p.ksize * p.ksize < 256) return false;
  return conv2d_mfma_addressable(p);
}

static int launch_one(const aivc_conv_params &p, hipStream_t s) {
  if (p.tail_c_out) {
    if (!conv2d_mfma_tail_supported(p)) return AIVC_ERR_UNSUPPORTED;
    constexpr ConvTile t = TILE_MENU[tile_index(6)];
    return launch_cfg2<AIVC_MODE_CONV, t.wm, t.wn, t.tm, t.tn, false, true, true>(p, s);
  }
  switch (p.mode) {
    case AIVC_MODE_CONV: return launch_mode<AIVC_MODE_CONV>(p, s);
    case AIVC_MODE_TCONV: return launch_mode<AIVC_MODE_TCONV>(p, s);
    case AIVC_MODE_GDN:
    case AIVC_MODE_IGDN: return launch_mode<AIVC_MODE_GDN>(p, s);
    default: return AIVC_ERR_UNSUPPORTED;
  }
}

int conv2d_mfma(const aivc_conv_params &p, hipStream_t s) {
  if (!lds_dma_loop(p.mode, p.c_in % BK == 0)) return launch_one(p, s);  // register-staged: 32-bit ELEMENT offsets, one launch
  return for_sub_batches(p, [&](const aivc_conv_params &q) { return launch_one(q, s); });
}

}  // namespace aivc
