// conv_wino.hip -- version 2 of the fp32 arithmetic contract (AIVC_PREC_FP32_WINO, include/aivc_hip.h): the stride-1 3x3
// convolutions with c_in % 32 == 0 and c_out % 64 == 0 as Winograd F(2x2, 3x3) on the gfx950 matrix cores -- 16 multiplications
// per 2x2 output pixels and channel pair instead of 36 on the scarce fp32 matrix pipe -- and, on the same kernel, the 5x5
// stride-2 convolutions (polyphase form) and transposed convolutions (class by class).  What was tried on the way and what it
// measured: experiments/r06.md (designs), experiments/wino_phases.md (phase offset), experiments/wino5_issue.md (5x5 forms),
// experiments/wino_class_walk.md (the transposed form's classes dealt round), experiments/wino_dynamic_walk.md (blocks claimed
// at run time).
//
//   work split     a workgroup = a block of 8 x 8 output tiles (16 x 16 pixels) x 64 output channels, 8 waves: (4 x 8 tiles)
//                  x 32 channels x 8 of the 16 positions each -- 8 accumulator blocks (128 registers) per wave, two waves per
//                  SIMD.  The reduction runs over chunks of 8 input channels (one octet of AIVC_K_ORDER = four
//                  v_mfma_f32_32x32x2_f32 steps per position); M_p = a fixed-order fmaf chain over ci per position, as the
//                  contract says.  After the last chunk a wave folds its 8 positions into the partial sums S0 / S1 of the
//                  four outputs of every tile, the two waves of a pair exchange halves through LDS and each finishes one
//                  output row (a = 0 / a = 1) of the tiles.  Persistent workgroups, one per CU, walk the block list and claim
//                  their blocks at run time (wino_dynamic_walk.h: a workgroup that starts late takes what is left).
//   per chunk      raw patch (18 x 18 pixels x 8 channels, 10 KB: replicate-clamped on the global side of the LDS-DMA, stored
//                  as four parity planes so that the transform's reads are contiguous), fetched ONCE per block and chunk; U
//                  image (16 positions x 64 channels x 8, 32 KB: aivc_winograd_weights lays it out as it is staged, one
//                  contiguous copy); V (16 positions x 64 tiles x 8, by a cooperative transform: 8 ds_read_b128 + 32 v_fma +
//                  4 ds_write_b128 per thread).
//   pipeline       everything double-buffered (158 KB of LDS, one workgroup per CU) and ONE barrier per chunk: in chunk c a
//                  wave issues the DMAs of raw(c + 2) and U(c + 1), transforms raw(c + 1) into the other V buffer and
//                  multiplies chunk c: one instruction stream in which the transform's steps follow the MFMAs of a position
//                  pair.  The raw pixels of a transform step are read BEFORE the pair's MFMAs and combined behind them (4
//                  float4 in flight); the transform runs every step in every chunk and has no run-time flag.  Chunk indices
//                  run on through the workgroup's blocks, so the pipeline is filled once per workgroup.
//   phase offset   the two waves of a SIMD (w and w + 4, the position halves) run that stream in the same order and are kept
//                  one window of non-matrix work apart: behind the chunk's barrier the upper half issues its 5-6 DMA
//                  instructions first, the lower half goes straight to its first pair and issues them behind that pair's
//                  MFMAs -- with both heads at the same place the matrix pipe stands idle for their length.  The barrier
//                  re-aligns the waves, so the offset is made again in every chunk.
//   three forms    MODE 0, stride-1 3x3: issue_raw / issue_u (address arithmetic and DMA instructions together), offset.
//                  MODE 1, polyphase 5x5 stride 2: 4 phases x c_in channels; the per-lane patch offsets change on phase entry,
//                  so the issue is split into prepare() (every wave at the chunk head: all address arithmetic) and fire_*()
//                  (the DMA instructions alone, placed by position half): the offset costs no second copy of the arithmetic.
//                  MODE 2, transposed 5x5 stride 2: 4 classes in the block list, dealt round among the workgroups
//                  (wino_class_walk.h: the classes issue 16 / 12 / 12 / 9 positions per chunk, and the plain walk hands a
//                  workgroup one class for the whole launch), zero extension through 64-bit per-lane addresses, issue_raw /
//                  issue_u with both heads at the barrier (no offset), 2 x 2 output stride in the epilogue.
//                  In the 5x5 forms a position whose U is zero by construction (wino_zero_pos) is neither fetched nor
//                  multiplied; its V is computed and never read.
#include <stdlib.h>

#include <mutex>
#include <unordered_map>

#include "mfma_util.h"
#include "wino_class_walk.h"
#include "wino_dynamic_walk.h"

namespace aivc {

// TH, TW, poly: read by no kernel; dropping them moves the polyphase kernel's code, so they stay (EXPERIMENTS.md, "Conv kernel sources", reverted pieces)
struct WinoArgs {
  aivc_conv_params p;
  int TH, TW;    // output tiles per image column / row
  int nby, nbx;  // blocks of 8 x 8 tiles per image
  int gy;        // blocks of 64 output channels
  int total;     // blocks in all: n * nby * nbx * gy
  int poly;      // 1: the 5x5 stride-2 convolution as four stride-1 3x3 convolutions of the input's polyphase components
  int cpp_shift; // log2 of the chunks per phase (c_in / 8)
};

constexpr int WINO_RAW_STAGE = 11 * 1024;  // 648 slots of 16 bytes (4 parity planes x 81 pixels x 2 channel quads), 11 DMA instructions
constexpr int WINO_U_STAGE = 32 * 1024;    // [16 positions][2 quads][64 channels][4 floats]
constexpr int WINO_V_QUAD = 1152;          // [64 tiles][4 floats] + 128: the second quad starts 32 banks further
constexpr int WINO_V_POS = 2 * WINO_V_QUAD;
constexpr int WINO_V_STAGE = 16 * WINO_V_POS;
constexpr int WINO_STAGES = 2 * (WINO_RAW_STAGE + WINO_U_STAGE + WINO_V_STAGE);
constexpr int WINO_LDS = WINO_STAGES + 16;  // + the word through which the workgroup learns the entry its lane 0 has claimed

// The counters of the block walk (wino_dynamic_walk.h): one slot set per stream that has launched the kernel, all zero between
// launches (the last workgroup out cleans its set)
constexpr unsigned WINO_WALK_SETS = 256;
__device__ uint32_t wino_walk_slots[WINO_WALK_SETS * WINO_WALK_SLOTS];

// 4 KB of zeros: the source of the patch pixels outside the image in the transposed form (zero extension; an LDS-DMA cannot fill)
__device__ __attribute__((aligned(4096))) float wino_zeros[1024];

// Zero-by-construction positions, the one statement of the rule.  Both 5x5 forms run 3x3 kernels that are 5 taps padded with
// zeros to 6: a row or column of zeros in g makes a row or column of U = G g G^T zero.  MODE 1, phase pc = 2 py + px: the taps
// 2 r + py / 2 l + px reach 5 for r = 2 (py = 1) / l = 2 (px = 1), so positions with i == 3 / j == 3 are zero (49 instead of 64 of
// the 4 x 16 position products).  MODE 2, class pc = 2 pyc + pxc: the taps pyc + 4 - 2 r / pxc + 4 - 2 l reach 5 for r = 0 (pyc = 1)
// / l = 0 (pxc = 1), so positions with i == 0 / j == 0 are zero.  Such a position is neither fetched nor multiplied.
template <int MODE>
__host__ __device__ constexpr bool wino_zero_pos(int pc, int i, int j) {
  if constexpr (MODE == 1) return ((pc >> 1) && i == 3) || ((pc & 1) && j == 3);
  if constexpr (MODE == 2) return ((pc >> 1) && i == 0) || ((pc & 1) && j == 0);
  return false;
}
// the positions q of position half `half` (i = 2 half + (q >> 2), j = q & 3) that phase / class pc issues, bit q set = issued
template <int MODE>
__host__ __device__ constexpr uint32_t wino_pos_mask(int pc, int half) {
  uint32_t m = 0u;
  for (int q = 0; q < 8; ++q) m |= wino_zero_pos<MODE>(pc, 2 * half + (q >> 2), q & 3) ? 0u : 1u << q;
  return m;
}

// The block walk of a persistent workgroup (wino_dynamic_walk.h): workgroup b sits on XCD b & 7 and claims entries of that XCD's
// contiguous eighth of the block list, one at a time, from the XCD's ticket counter in slot set `set`.  ONE lane of the workgroup
// claims; the others learn the entry through the LDS word claim_lds.  Which entries a workgroup takes is decided here; what
// an entry means is make_desc's business (the transposed form reads it through wino_class_walk.h).
struct WinoWalk {
  // (the XCD's range and its counter are worked out at every claim, once per block: nothing of them is kept in registers across
  // the chunk loop)
  uint32_t total, set;
  __device__ __forceinline__ uint32_t claim() const {  // (one lane)
    const uint32_t xcd = blockIdx.x & 7u;
    uint32_t *ticket = wino_walk_slots + set * WINO_WALK_SLOTS + xcd;
    return wino_ticket_entry(wino_xcd_range(total, xcd), __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
  }
  // one lane, after the workgroup's last claim has returned: count the workgroup out; the last one of the launch zeroes the set.
  // Every other workgroup's claims returned before it counted itself out, so nothing is added behind the zeroes, and the end of
  // the kernel orders them before the next launch on the stream
  __device__ __forceinline__ void leave() const {
    uint32_t *set0 = wino_walk_slots + set * WINO_WALK_SLOTS;
    if (wino_last_out(__hip_atomic_fetch_add(set0 + WINO_WALK_EXIT, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT), gridDim.x)) {
#pragma unroll
      for (uint32_t i = 0; i <= WINO_WALK_EXIT; ++i) __hip_atomic_store(set0 + i, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
};

// MODE 0: stride-1 3x3.  MODE 1 (POLY): the polyphase form of the 5x5 stride-2 convolutions.  MODE 2 (TC): the 5x5 stride-2
// TRANSPOSED convolutions: each of the four output parity classes is a stride-1 3x3 correlation of the (zero-extended) input with
// the class's taps padded with zeros -- a block of the list is (pixel block, class, 64 output channels), the outputs of class
// (pyc, pxc) land on pixels (2 y + pyc, 2 x + pxc).
// Separate instantiations: the stride-1 3x3 kernel pays nothing for the others.
template <int MODE>
__global__ __launch_bounds__(512) void conv_wino_kernel(WinoArgs a, uint32_t walk_set) {
  constexpr bool POLY = MODE == 1, TC = MODE == 2;
  extern __shared__ __attribute__((aligned(16))) char wsmem[];
  char *raw = wsmem, *Us = wsmem + 2 * WINO_RAW_STAGE, *Vs = Us + 2 * WINO_U_STAGE;
  const uint32_t lds0 = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) char *)wsmem;

  const aivc_conv_params &p = a.p;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ph = wave >> 2, wm = (wave >> 1) & 1, wn = wave & 1;  // waves w and w + 4 (one SIMD) = the two position halves of a sub-tile
  // H x W: the pixel grid the blocks walk = the OUTPUT's (stride 1: also the input's); Hi x Wi: the input's.  Polyphase form
  // (MODE 1, 5x5 stride 2, include/aivc_hip.h): the reduction runs over 4 phases x c_in channels, chunk c belongs to phase
  // c >> cpp_shift = 2 py + px, whose patch pixel (y, x) is input pixel (clamp(2 y + py), clamp(2 x + px)) -- the replicate
  // padding of the ORIGINAL image -- and whose 3x3 kernel is the phase's taps padded with zeros (wino_zero_pos).
  const int H = TC ? p.h_in : p.h_out, W = TC ? p.w_in : p.w_out, Hi = p.h_in, Wi = p.w_in, Cin = p.c_in, Cout = p.c_out;
  const int gyc = TC ? 4 * a.gy : a.gy;  // entries of the block list per pixel block: channel blocks (x 4 classes)
  const int cpp_shift = a.cpp_shift, cpp_mask = (1 << a.cpp_shift) - 1;

  // ---- block walk: persistent workgroups (gridDim.x of them: one per CU, or one per block of a short list) ------------------
  // Lane 0 of wave 0 claims the first block here and, in the first chunk of every block, the next one: a workgroup never holds
  // more than ONE block it has not started (with two, the workgroups that come first would take a list of about two blocks per CU
  // between them, and every launch would end on up to two blocks of imbalance instead of one).  The loader wants the next block
  // from chunk nch - 2 >= 2 on, so nxt is made behind chunk 1.  blk_nxt == WINO_WALK_END: the block being computed is the
  // workgroup's last
  const WinoWalk walk = {(uint32_t)a.total, walk_set};
  volatile uint32_t *claim_lds = reinterpret_cast<volatile uint32_t *>(wsmem + WINO_STAGES);
  if (tid == 0) claim_lds[0] = walk.claim();
  __syncthreads();
  const uint32_t blk_cur = __builtin_amdgcn_readfirstlane(claim_lds[0]);
  uint32_t blk_nxt = WINO_WALK_END;
  if (blk_cur == WINO_WALK_END) {  // (a workgroup that started late, or an empty range)
    if (tid == 0) walk.leave();
    return;
  }
  // descriptor of a block: what the loader needs (image base, chunk images of its channel block, per-lane patch offsets) and
  // what the epilogue needs (coordinates)
  struct Desc {
    const float *xbase, *ubase;
    uint32_t r_off[2];  // stride-1 form: per-lane byte offsets of the block's raw patch (the polyphase form keeps those of the phase being issued)
    int img, byi, bxi, cb;  // cb: channel block (transposed form: class * gy + channel block)
  };
  // raw: instruction k of 11 writes slots 64 k .. 64 k + 63; wave w issues k = w and, for w < 3, k = w + 8.  slot = (plane *
  // 81 + hy * 9 + hx) * 2 + quad with plane = (py & 1) * 2 + (px & 1), hy = py >> 1, hx = px >> 1 for patch pixel (py, px)
  int s_quad[2], s_py[2], s_px[2];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    int sl = 64 * (wave + 8 * k) + lane;
    sl = sl < 648 ? sl : 647;  // (pad lanes of the last instruction fetch the last slot again)
    const int q2 = sl >> 1, plane = q2 / 81, rem = q2 - plane * 81, hy = rem / 9, hx = rem - hy * 9;
    s_quad[k] = sl & 1;
    s_py[k] = 2 * hy + (plane >> 1);
    s_px[k] = 2 * hx + (plane & 1);
  }
  const int nch = POLY ? 4 * (Cin >> 3) : (Cin >> 3);  // chunks of 8 (virtual) input channels per block
  auto make_desc = [&](uint32_t blk) {
    Desc d;
    uint32_t rest;
    if constexpr (TC) {  // the classes of a pixel block are dealt round among the workgroups (wino_class_walk.h)
      const WinoClassEntry e = wino_class_entry(blk, (uint32_t)gyc, (uint32_t)a.total, gridDim.x);
      d.cb = (int)e.cb;
      rest = e.pb;
    } else {
      d.cb = (int)(blk % (uint32_t)gyc);
      rest = blk / (uint32_t)gyc;
    }
    d.bxi = (int)(rest % (uint32_t)a.nbx);
    rest /= (uint32_t)a.nbx;
    d.byi = (int)(rest % (uint32_t)a.nby);
    d.img = (int)(rest / (uint32_t)a.nby);
    d.xbase = p.x + (size_t)d.img * (size_t)Hi * Wi * Cin;                       // this image (32-bit byte offsets inside it)
    d.ubase = p.w_wino + (size_t)d.cb * (size_t)nch * (WINO_U_STAGE / 4);        // this channel block's chunk images
    if constexpr (MODE == 0) {
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        const int iy = max(min(16 * d.byi - 1 + s_py[k], Hi - 1), 0), ix = max(min(16 * d.bxi - 1 + s_px[k], Wi - 1), 0);
        d.r_off[k] = ((uint32_t)(iy * Wi + ix) * (uint32_t)Cin + (uint32_t)(4 * s_quad[k])) * 4u;
      }
    }
    return d;
  };
  // ---- load: the LDS-DMA issue of a chunk's raw patch and U image -------------------------------------------------------------
  // polyphase form: per-lane byte offsets of the raw patch of block d_ in phase ph2 = 2 py + px, recomputed when the issue stream
  // enters a phase (every c_in / 8 chunks), kept in two registers in between
  uint32_t iss_off[2];
  auto patch_offsets = [&](const Desc &d_, int ph2) {
    const int st = POLY ? 2 : 1, py = ph2 >> 1, px = ph2 & 1;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int iy = max(min(st * (16 * d_.byi - 1 + s_py[k]) + py, Hi - 1), 0), ix = max(min(st * (16 * d_.bxi - 1 + s_px[k]) + px, Wi - 1), 0);
      iss_off[k] = ((uint32_t)(iy * Wi + ix) * (uint32_t)Cin + (uint32_t)(4 * s_quad[k])) * 4u;
    }
  };
  // transposed form: per-lane 64-bit source addresses of the chunk being issued (a pixel outside the image reads zeros), advanced
  // by the 32 bytes of a chunk after every issue, recomputed when the issue stream enters a block
  uint64_t iss_addr[2];
  auto tc_addresses = [&](const Desc &d_) {
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      const int iy = 16 * d_.byi - 1 + s_py[k], ix = 16 * d_.bxi - 1 + s_px[k];
      const bool in = iy >= 0 && iy < Hi && ix >= 0 && ix < Wi;
      const uint64_t a_in = (uint64_t)(uintptr_t)d_.xbase + ((uint64_t)((uint32_t)(iy * Wi + ix)) * (uint32_t)Cin + (uint32_t)(4 * s_quad[k])) * 4u;
      const uint64_t a_z = (uint64_t)(uintptr_t)wino_zeros + (uint32_t)(16 * s_quad[k]);
      iss_addr[k] = in ? a_in : a_z;
    }
  };
  Desc cur = make_desc(blk_cur), nxt = cur;

  const uint32_t r_dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)wave * 1024u);
  const uint32_t u_dst = __builtin_amdgcn_readfirstlane(lds0 + (uint32_t)(2 * WINO_RAW_STAGE) + (uint32_t)wave * 4096u);
  const uint32_t u_off = (uint32_t)(wave * 4096 + lane * 16);
  auto uniform_ptr = [](const float *q) -> const float * {  // (wave-uniform by construction: tell the compiler, the DMA wants a scalar base)
    const uint64_t v = (uint64_t)(uintptr_t)q;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
    return reinterpret_cast<const float *>((uintptr_t)(((uint64_t)hi << 32) | lo));
  };
  // stride-1 and transposed forms: issue_raw / issue_u hold the address arithmetic and the DMA instructions of a chunk together
  // (the polyphase form issues through prepare / fire_* below)
  auto issue_raw = [&](const Desc &d_, int c) {  // chunk c of block d_ -> raw stage c & 1 (chunks are issued in order)
    const uint32_t d = r_dst + (uint32_t)((c & 1) * WINO_RAW_STAGE);
    if constexpr (TC) {
      if (c == 0) tc_addresses(d_);
      const uint32_t du = __builtin_amdgcn_readfirstlane(d);
      asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(iss_addr[0]), "s"(du) : "memory", "m0");
      if (wave < 3) asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" : : "v"(iss_addr[1]), "s"(du + 8192u) : "memory", "m0");
      iss_addr[0] += 32u;
      iss_addr[1] += 32u;
    } else {
      const float *src = d_.xbase + 8 * c;
      glds16(src, d_.r_off[0], d);
      if (wave < 3) glds16(src, d_.r_off[1], d + 8192u);
    }
  };
  // U chunk images are straight copies; this wave's 4 KB piece holds positions 2 wave and 2 wave + 1 = (i, j) and (i, j + 1)
  auto issue_u = [&](const Desc &d_, int c) {  // chunk c of block d_ -> U stage c & 1
    const float *src = TC ? uniform_ptr(d_.ubase + (size_t)c * (WINO_U_STAGE / 4)) : d_.ubase + (size_t)c * (WINO_U_STAGE / 4);
    const uint32_t d = TC ? __builtin_amdgcn_readfirstlane(u_dst + (uint32_t)((c & 1) * WINO_U_STAGE)) : u_dst + (uint32_t)((c & 1) * WINO_U_STAGE);
    bool lo = true, hi = true;
    if constexpr (TC) {
      const int cls = d_.cb / a.gy, i = wave >> 1, j = 2 * (wave & 1);
      lo = !wino_zero_pos<MODE>(cls, i, j);
      hi = !wino_zero_pos<MODE>(cls, i, j + 1);
    }
    if (lo && hi) glds_piece<GLDS_BOTH>(src, u_off, d);
    else if (lo) glds_piece<GLDS_LO>(src, u_off, d);
    else if (hi) glds_piece<GLDS_HI>(src, u_off, d);
  };

  // polyphase form: the issue of a chunk in two parts.  prepare(cr, cu), run by every wave at the chunk head, does everything
  // of the issue of raw chunk cr and U chunk cu (of this workgroup's current block, possibly beyond its chunks: the next block's first
  // ones) that is no DMA instruction: cur or nxt, the per-lane patch offsets on phase entry, the wave-uniform sources, which
  // pieces are issued.  fire_raw / fire_u hold the DMA instructions alone, under their guards (the LDS stage is the caller's
  // compile-time constant), so that placing them by position half costs no second copy of the address arithmetic.
  struct Prep {
    const float *r_src, *u_src;  // wave-uniform sources: the raw chunk, the U chunk image
    uint32_t flags;              // 1: the raw chunk is issued; 2 / 4: the lo / hi pieces of the U image are
  };
  auto prepare = [&](int cr, int cu) -> Prep {
    Prep q;
    const bool more = blk_nxt != WINO_WALK_END;
    uint32_t fl = 0u;
    {
      const bool own = cr < nch;
      const int c = own ? cr : cr - nch;
      const Desc &d_ = own ? cur : nxt;
      if (own || more) {
        fl |= 1u;
        if ((c & cpp_mask) == 0) patch_offsets(d_, c >> cpp_shift);  // the issue stream enters a phase
      }
      q.r_src = uniform_ptr(d_.xbase + 8 * (c & cpp_mask));
    }
    {
      const bool own = cu < nch;
      const int c = own ? cu : cu - nch;
      const Desc &d_ = own ? cur : nxt;
      q.u_src = uniform_ptr(d_.ubase + (size_t)c * (WINO_U_STAGE / 4));
      if (own || more) {
        const int pc = c >> cpp_shift, i = wave >> 1, j = 2 * (wave & 1);
        if (!wino_zero_pos<MODE>(pc, i, j)) fl |= 2u;
        if (!wino_zero_pos<MODE>(pc, i, j + 1)) fl |= 4u;
      }
    }
    q.flags = __builtin_amdgcn_readfirstlane(fl);
    return q;
  };
  auto fire_raw = [&](auto STAGE, const Prep &q) {
    const uint32_t d = r_dst + (uint32_t)(decltype(STAGE)::value * WINO_RAW_STAGE);
    if (q.flags & 1u) {
      glds16(q.r_src, iss_off[0], d);
      if (wave < 3) glds16(q.r_src, iss_off[1], d + 8192u);
    }
  };
  auto fire_u = [&](auto STAGE, const Prep &q) {
    const uint32_t d = u_dst + (uint32_t)(decltype(STAGE)::value * WINO_U_STAGE);
    const uint32_t both = q.flags & 6u;
    if (both == 6u) glds_piece<GLDS_BOTH>(q.u_src, u_off, d);
    else if (both == 2u) glds_piece<GLDS_LO>(q.u_src, u_off, d);
    else if (both == 4u) glds_piece<GLDS_HI>(q.u_src, u_off, d);
  };

  // ---- transform plan: thread = (tile, channel quad, row i of the 4 x 4 positions) -----------------------------------------
  // Which (tile, channel quad) unit of the wave's 4 tile rows x 8 tiles x 2 quads a lane transforms is chosen for the LDS
  // (MI355X_MICROARCH.md, LDS):  ds_read_b128 is served in the lane groups {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} (and
  // + 32), banks of 4 bytes mod 64 -- a group reads ONE tile row of a parity plane: 16 consecutive slots = 256 contiguous
  // bytes, every bank once;  ds_write_b128 is served 8 consecutive lanes at a time, banks mod 32 -- such an octet holds four
  // lanes of each of two read groups: the row of the first group hands it tiles 0-3 (or 4-7) of one quad, the row of the
  // second group tiles 4-7 (0-3) of the same quad: 2 x 64 bytes that differ in address bit 6.  With (quad, tx, ty) read off
  // the lane id directly a third of the kernel's LDS cycles were bank conflicts (profiles/r06_pmc_wino_before_lane_map.json).
  const int l32 = lane & 31;
  const int t_grp = (l32 < 4 || (l32 >= 12 && l32 < 16) || (l32 >= 20 && l32 < 28)) ? 0 : 1;
  const int t_pos = t_grp == 0 ? (l32 < 4 ? l32 : (l32 < 16 ? l32 - 8 : l32 - 12)) : (l32 < 12 ? l32 - 4 : (l32 < 20 ? l32 - 8 : l32 - 16));
  const int t_quad = t_pos >> 3, t_tx = (t_pos & 7) ^ (t_grp << 2), t_ty = ((tid >> 6) & 1) * 4 + (lane >> 5) * 2 + t_grp;
  const int t_i = __builtin_amdgcn_readfirstlane(tid >> 7);
  const int t_ra = t_i == 0 ? 0 : (t_i == 2 ? 2 : 1), t_rb = t_i == 3 ? 3 : (t_i == 2 ? 1 : 2);  // rows A[i], B[i] of the patch
  const float t_si = t_i == 1 ? 1.0f : -1.0f;
  const int t_base = ((t_ty * 9 + t_tx) * 2 + t_quad) * 16;
  // byte offset of patch pixel (2 ty + r, 2 tx + c) relative to t_base
  auto pix_off = [](int r, int c) { return (((r & 1) * 2 + (c & 1)) * 81 + (r >> 1) * 9 + (c >> 1)) * 32; };
  int t_oa[4], t_ob[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    t_oa[c] = t_base + pix_off(t_ra, c);
    t_ob[c] = t_base + pix_off(t_rb, c);
  }
  const int t_vdst = (4 * t_i) * WINO_V_POS + t_quad * WINO_V_QUAD + (t_ty * 8 + t_tx) * 16;
  // the transform of one chunk in 8 steps (interleaved with the 8 positions of the multiply): steps 0-3 combine the rows of
  // patch column cc = step (R[cc] = d[A_i][cc] + S_i d[B_i][cc]), steps 4-7 write V_j = R[A_j] + S_j R[B_j], j = step - 4
  float4 R[4];
  auto comb = [](const float4 &u, const float4 &v, float sgn) {
    float4 o;
    o.x = __builtin_fmaf(sgn, v.x, u.x);
    o.y = __builtin_fmaf(sgn, v.y, u.y);
    o.z = __builtin_fmaf(sgn, v.z, u.z);
    o.w = __builtin_fmaf(sgn, v.w, u.w);
    return o;
  };
  auto transform_step = [&](auto STAGE, auto STEP) {  // raw stage -> V stage of the same parity (a compile-time constant: the
    // chunk loop is unrolled by two, so every LDS access of the loop is a per-thread base + an immediate)
    constexpr int st = decltype(STEP)::value, stage = decltype(STAGE)::value;
    const char *rs = raw + stage * WINO_RAW_STAGE;
    char *vd = Vs + stage * WINO_V_STAGE + t_vdst;
    if constexpr (st < 4) {
      const float4 xa = *reinterpret_cast<const float4 *>(rs + t_oa[st]), xb = *reinterpret_cast<const float4 *>(rs + t_ob[st]);
      R[st] = comb(xa, xb, t_si);
    } else if constexpr (st == 4) {
      *reinterpret_cast<float4 *>(vd) = comb(R[0], R[2], -1.0f);
    } else if constexpr (st == 5) {
      *reinterpret_cast<float4 *>(vd + WINO_V_POS) = comb(R[1], R[2], 1.0f);
    } else if constexpr (st == 6) {
      *reinterpret_cast<float4 *>(vd + 2 * WINO_V_POS) = comb(R[2], R[1], -1.0f);
    } else {
      *reinterpret_cast<float4 *>(vd + 3 * WINO_V_POS) = comb(R[1], R[3], -1.0f);
    }
  };
  auto transform0 = [&]() {  // chunk 0 of the workgroup's first block
    using std::integral_constant;
    using Z = integral_constant<int, 0>;
    transform_step(Z{}, integral_constant<int, 0>{});
    transform_step(Z{}, integral_constant<int, 1>{});
    transform_step(Z{}, integral_constant<int, 2>{});
    transform_step(Z{}, integral_constant<int, 3>{});
    transform_step(Z{}, integral_constant<int, 4>{});
    transform_step(Z{}, integral_constant<int, 5>{});
    transform_step(Z{}, integral_constant<int, 6>{});
    transform_step(Z{}, integral_constant<int, 7>{});
  };

  // ---- multiply plan -------------------------------------------------------------------------------------------------------
  floatx16 acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[q][r] = 0.0f;
  const int hh = lane >> 5, l31 = lane & 31;
  const int a_rd = (8 * ph) * WINO_V_POS + hh * WINO_V_QUAD + (32 * wm + l31) * 16;
  const int b_rd = (8 * ph) * 2048 + hh * 1024 + (32 * wn + l31) * 16;
  // chunk c multiplied (8 positions x 4 MFMAs) with the transform of chunk c + 1 dealt out between the positions: one
  // instruction stream per wave in which matrix and vector / LDS work alternate.  dma(): the chunk's LDS-DMA issues, which the
  // stride-1 kernel and the polyphase form place by position half (the file header's phase offset); the transposed form has
  // issued them already
  // FIRST: the block's first chunk starts its accumulators from the inline constant 0 (no clearing pass after the fold)
  // pm: bit q set = position q of this wave's half is issued (chunk() derives it from wino_zero_pos)
  // The transform of the NEXT chunk runs every step in every chunk, in all three forms.  Behind the last chunk of a workgroup's
  // last block it reads the stale raw stage 0 and writes V stage 0, which nobody reads again (the pair exchange uses V stage 1);
  // in the 5x5 forms it also computes the V positions whose U is zero by construction: rd() is guarded by pm and the transposed
  // form's first chunk clears such an accumulator with an MFMA of zeros, so they are never read
  auto multiply = [&](auto STAGE, auto FIRST, uint32_t pm, auto &&dma) {
    constexpr int stage = decltype(STAGE)::value;
    constexpr bool first = decltype(FIRST)::value;
    using NEXT = std::integral_constant<int, 1 - stage>;
    const char *va = Vs + stage * WINO_V_STAGE + a_rd, *ub = Us + stage * WINO_U_STAGE + b_rd;
    // positions in pairs: the MFMAs of two accumulators alternate (a dependent MFMA waits for its predecessor's last pass),
    // the fragments of the next pair are read while this pair multiplies, the transform steps follow the pair's MFMAs (the
    // first MFMAs behind the chunk's barrier then wait for two LDS round trips only); the raw pixels of the
    // pair's read steps are asked for in front of its MFMAs, so that the combination behind them does not wait for LDS
    float4 af[2][2], bf[2][2];
    auto rd = [&](int set, int q) {
      af[set][0] = *reinterpret_cast<const float4 *>(va + q * WINO_V_POS);
      bf[set][0] = *reinterpret_cast<const float4 *>(ub + q * 2048);
      af[set][1] = *reinterpret_cast<const float4 *>(va + (q + 1) * WINO_V_POS);
      bf[set][1] = *reinterpret_cast<const float4 *>(ub + (q + 1) * 2048);
    };
    if constexpr (!TC) {
      if (ph) dma();  // (the lower half issues them behind its first pair)
    }
    rd(0, 0);
    auto pair = [&](auto Q) {
      constexpr int q = decltype(Q)::value, set = (q >> 1) & 1;
      using std::integral_constant;
      if constexpr (q + 2 < 8) {
        if (MODE == 0 || (first && !TC) || (pm & (0xCu << q))) rd(1 - set, q + 2);
      }
      float4 ta[2], tb[2];  // the raw pixels of two read steps of the transform, in flight under the pair's MFMAs
      auto reads = [&](auto S) {
        constexpr int st = decltype(S)::value;
        const char *rs = raw + (1 - stage) * WINO_RAW_STAGE;
        ta[0] = *reinterpret_cast<const float4 *>(rs + t_oa[st]);
        tb[0] = *reinterpret_cast<const float4 *>(rs + t_ob[st]);
        ta[1] = *reinterpret_cast<const float4 *>(rs + t_oa[st + 1]);
        tb[1] = *reinterpret_cast<const float4 *>(rs + t_ob[st + 1]);
      };
      auto finish = [&](auto S) {
        constexpr int st = decltype(S)::value;
        if constexpr (st < 4) {
          R[st] = comb(ta[0], tb[0], t_si);
          R[st + 1] = comb(ta[1], tb[1], t_si);
        } else {
          transform_step(NEXT{}, integral_constant<int, st>{});
          transform_step(NEXT{}, integral_constant<int, st + 1>{});
        }
      };
      if constexpr (q < 4) reads(Q);
      __builtin_amdgcn_sched_barrier(0);
      const float4 x0 = af[set][0], y0 = bf[set][0], x1 = af[set][1], y1 = bf[set][1];
      if constexpr (first && TC) {
        // the block's first chunk: a position the class does not issue gets a cleared accumulator (one MFMA of zeros), the others
        // start from the inline zero
        const floatx16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if ((pm >> q) & 1u) acc[q] = mfma_oct1(x0, y0, zero);
        else acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(0.0f, 0.0f, zero, 0, 0, 0);
        if ((pm >> (q + 1)) & 1u) acc[q + 1] = mfma_oct1(x1, y1, zero);
        else acc[q + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(0.0f, 0.0f, zero, 0, 0, 0);
      } else if constexpr (first) {
        const floatx16 zero = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.x, y0.x, zero, 0, 0, 0);
        acc[q + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.x, y1.x, zero, 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.y, y0.y, acc[q], 0, 0, 0);
        acc[q + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.y, y1.y, acc[q + 1], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.z, y0.z, acc[q], 0, 0, 0);
        acc[q + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.z, y1.z, acc[q + 1], 0, 0, 0);
        acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(x0.w, y0.w, acc[q], 0, 0, 0);
        acc[q + 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(x1.w, y1.w, acc[q + 1], 0, 0, 0);
      } else {
        // (wave-uniform tests; the four MFMAs of a position in a row: alternating two accumulators measured the same, experiments/r06.md 2)
        if (MODE == 0 || ((pm >> q) & 1u)) acc[q] = mfma_oct1(x0, y0, acc[q]);
        if (MODE == 0 || ((pm >> (q + 1)) & 1u)) acc[q + 1] = mfma_oct1(x1, y1, acc[q + 1]);
      }
      __builtin_amdgcn_sched_barrier(0);
      if constexpr (!TC && q == 0) {
        if (!ph) dma();
      }
      finish(Q);
      __builtin_amdgcn_sched_barrier(0);
    };
    using std::integral_constant;
    pair(integral_constant<int, 0>{});
    pair(integral_constant<int, 2>{});
    pair(integral_constant<int, 4>{});
    pair(integral_constant<int, 6>{});
  };

  // ---- the reduction, pipelined ACROSS blocks: chunk indices run on through the workgroup's blocks (c_in / 8 is even, so
  // the stage parity of a chunk is its index inside its block) -------------------------------------------------------------
  // (stride-1 and transposed forms; the polyphase form's prepare() does the same choice of cur / nxt)
  auto issue_raw_at = [&](int c) {  // chunk c of this workgroup's current block, c possibly beyond the block's chunks
    if (c < nch) issue_raw(cur, c);
    else if (blk_nxt != WINO_WALK_END) issue_raw(nxt, c - nch);
  };
  auto issue_u_at = [&](int c) {
    if (c < nch) issue_u(cur, c);
    else if (blk_nxt != WINO_WALK_END) issue_u(nxt, c - nch);
  };
  if constexpr (POLY) {
    const Prep q0 = prepare(0, 0);
    fire_raw(std::integral_constant<int, 0>{}, q0);
    fire_u(std::integral_constant<int, 0>{}, q0);
    fire_raw(std::integral_constant<int, 1>{}, prepare(1, 0));
  } else {
    issue_raw(cur, 0);
    issue_u(cur, 0);
    issue_raw_at(1);
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  transform0();
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();
  const int act1 = p.act1, act2 = p.act2;
  for (;;) {
    // two chunks per trip (stage parities 0, 1: compile-time LDS offsets); the block's first chunk starts the accumulators
    auto chunk = [&](auto STAGE, auto FIRST, int c) {
      // here: V(c) complete, U(c) and raw(c + 1) in LDS; raw stage c & 1, U stage (c + 1) & 1 and V stage (c + 1) & 1 are free
      // (chunks beyond this block's are the first ones of the next block): the DMA targets are free from here to the closing
      // s_waitcnt + barrier, wherever in the chunk a wave issues them.  The transform of chunk c + 1 rides along
      Prep q;
      if constexpr (POLY) q = prepare(c + 2, c + 1);  // every wave, here: fire() is placed by position half
      auto dma = [&]() {
        if constexpr (POLY) {
          fire_raw(STAGE, q);  // raw(c + 2) -> raw stage c & 1, U(c + 1) -> the other U stage
          fire_u(std::integral_constant<int, 1 - decltype(STAGE)::value>{}, q);
        } else {
          issue_raw_at(c + 2);
          issue_u_at(c + 1);
        }
      };
      // pm: the positions of this wave's half that the chunk's phase / the block's class issues (wino_zero_pos).  Bit 0 of pc
      // takes a column j away in both halves, bit 1 a row i, i.e. one half's q = 0 .. 3 or q = 4 .. 7.  (Transposed form: the
      // block's FIRST chunk multiplies the others by zeros to clear their accumulators)
      uint32_t pm = 0xFFu;
      if constexpr (MODE != 0) {
        constexpr uint32_t ZCOL = 0xFFu ^ wino_pos_mask<MODE>(1, 0), ZROW = 0xFFu ^ wino_pos_mask<MODE>(2, POLY ? 1 : 0);
        static_assert(wino_pos_mask<MODE>(1, 1) == (0xFFu ^ ZCOL) && wino_pos_mask<MODE>(2, POLY ? 0 : 1) == 0xFFu &&
                      wino_pos_mask<MODE>(3, POLY ? 1 : 0) == (0xFFu ^ (ZCOL | ZROW)), "pm's two terms are the whole rule");
        const int pc = POLY ? c >> cpp_shift : cur.cb / a.gy;
        pm = 0xFFu & ~((pc & 1) ? ZCOL : 0u) & ~(((pc >> 1) && (POLY ? ph : !ph)) ? ZROW : 0u);
      }
      if constexpr (TC) dma();  // (transposed form: both heads at the barrier)
      multiply(STAGE, FIRST, pm, dma);
      asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
    };
    {
      using std::integral_constant;
      using S0 = integral_constant<int, 0>;
      using S1 = integral_constant<int, 1>;
      // the claim of the next block rides in the block's first chunk: asked for at its head, in hand when the chunk's closing
      // s_waitcnt has run, published behind its barrier (every wave has read the previous one by then), read behind the
      // second chunk's barrier.  (Chunks 0 and 1 issue raw chunks 2, 3 and U chunks 1, 2 of THIS block: nch >= 4.)  Nothing of
      // it stands inside a chunk: with the publication and make_desc at the chunks' ends, under the last pair's MFMAs, or with
      // the workgroup's first block its own without a claim, the compiler moved the 2-chunk loop and every launch was slower
      // (experiments/wino_dynamic_walk.md)
      uint32_t ahead = WINO_WALK_END;
      if (tid == 0) ahead = walk.claim();
      chunk(S0{}, std::true_type{}, 0);
      if (tid == 0) claim_lds[0] = ahead;
      chunk(S1{}, std::false_type{}, 1);
      blk_nxt = __builtin_amdgcn_readfirstlane(claim_lds[0]);
      if (blk_nxt != WINO_WALK_END) nxt = make_desc(blk_nxt);
      for (int c = 2; c < nch; c += 2) {
        chunk(S0{}, std::false_type{}, c);
        chunk(S1{}, std::false_type{}, c + 1);
      }
    }

    // ---- fold: S[a][b] = sum over this wave's positions (ascending, from +0) of T[a][i] T[b][j] M_p -------------------------------
    // keep[b]: output row a = ph (this wave finishes it), give[b]: row 1 - ph (handed to the partner).  The position half is a
    // compile-time constant inside each instantiation: the coefficients are, and the fold is the 18 block additions /
    // subtractions it needs (with ph a run-time value the compiler built every term of both signs and selected: 308 v_cndmask +
    // 224 v_sub + 136 v_pk_add per block and wave)
    floatx16 keep[2], give[2];
    auto fold = [&](auto PH) {
      constexpr int phc = decltype(PH)::value;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb)
#pragma unroll
        for (int r = 0; r < 16; ++r) keep[bb][r] = give[bb][r] = 0.0f;
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int i = 2 * phc + (q >> 2), j = q & 3;
        const int t0i = i < 3 ? 1 : 0, t1i = i == 0 ? 0 : (i == 1 ? 1 : -1);
        const int t0j = j < 3 ? 1 : 0, t1j = j == 0 ? 0 : (j == 1 ? 1 : -1);
#pragma unroll
        for (int o = 0; o < 4; ++o) {
          const int cf = ((o >> 1) ? t1i : t0i) * ((o & 1) ? t1j : t0j);
          floatx16 &dst = (o >> 1) == phc ? keep[o & 1] : give[o & 1];
          if (cf > 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = dst[r] + acc[q][r];
          } else if (cf < 0) {
#pragma unroll
            for (int r = 0; r < 16; ++r) dst[r] = dst[r] - acc[q][r];
          }
        }
      }
    };
    if (ph) fold(std::integral_constant<int, 1>{});
    else fold(std::integral_constant<int, 0>{});
    // exchange: the wave of half ph finishes output row a = ph of the tiles; it hands its partial sums of the other row to its
    // partner (wave ^ 4), one output column b at a time, through the V stage the reduction does not touch before the next
    // chunk's transform (stage 1: the last chunk's V went to stage (nch - 1) & 1 = 1; the next block's chunk 0 sits in stage 0)
    {
      float *xch = reinterpret_cast<float *>(Vs + WINO_V_STAGE) + wave * 1024;  // [16 registers][64 lanes] per wave: 32 KB
      const float *theirs = reinterpret_cast<const float *>(Vs + WINO_V_STAGE) + (wave ^ 4) * 1024;
#pragma unroll
      for (int bb = 0; bb < 2; ++bb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) xch[r * 64 + lane] = give[bb][r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
#pragma unroll
        for (int r = 0; r < 16; ++r) keep[bb][r] = keep[bb][r] + theirs[r * 64 + lane];  // acc[a][b] = S0 + S1 (one fp32 addition:
        // the same bits whichever of the two operands is this wave's)
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
    }

    // ---- epilogue: the contract's order (Epilogue::finish, common.h) on output row a = ph of every tile -------------------
    {
      const float *__restrict__ g_mul = p.mul;
      const float *__restrict__ g_res = p.res;
      float *__restrict__ g_y = p.y;
      // transposed form: this block's class (pyc, pxc); output pixel of grid pixel (y, x) = (2 y + pyc, 2 x + pxc) of a 2 H x 2 W image
      const int cls = TC ? cur.cb / a.gy : 0, pyc = cls >> 1, pxc = cls & 1;
      const int OS = TC ? 2 : 1;                     // output pixels per grid pixel and axis
      const int Wo_ = OS * W, Ho_ = OS * H;
      const int co = (TC ? cur.cb - cls * a.gy : cur.cb) * 64 + 32 * wn + l31;
      const bool has_bias = p.bias != nullptr;
      const float cbias = has_bias ? p.bias[co] : 0.0f;
      const int oy_w = 2 * (8 * cur.byi + 4 * wm) + ph;  // output row of the wave's first tile row (wave-uniform)
      const bool inside_x = 16 * cur.bxi + 16 <= W;
      if (!g_mul && act1 != AIVC_ACT_SIGMOID) {
        // fast path: one wave-uniform 64-bit base per tile row, one 32-bit byte offset per lane, tile column and output column as
        // immediates -- no per-element address arithmetic; lane masks only in the right-edge column of an image whose width is
        // no multiple of 16 (EDGE: the general path below made every output of such a block one dependent residual round
        // trip -- 160 instead of 43 us per block, which is what kept the kernel at the tap kernel's pace on the 68 x 120 layers)
        const int cols_left = W - 16 * cur.bxi;  // output columns of this block that exist (wave-uniform)
        typedef __attribute__((address_space(1))) char gchar;
        typedef __attribute__((address_space(1))) float gfloat;
        typedef __attribute__((address_space(1))) const float cgfloat;
        const uint32_t c4 = (uint32_t)Cout * 4u, sx = (uint32_t)OS * c4;  // bytes per output pixel / per grid pixel along x
        uint32_t lane_b = (uint32_t)(2 * (8 * cur.bxi + 4 * hh)) * sx + (uint32_t)pxc * c4 + (uint32_t)co * 4u;
        asm volatile("" : "+v"(lane_b));
        const size_t img_b = (size_t)cur.img * (size_t)Ho_ * Wo_ * c4;
        auto rows = [&](auto RES, auto KIND, auto INSIDE) {
          constexpr bool has_res = decltype(RES)::value;
          constexpr bool edge = !decltype(INSIDE)::value;  // the block's right columns lie outside the image
          constexpr int kind = decltype(KIND)::value;  // act1 / act2 combination, see below
          bool ok[8];  // column 2 (4 hh + rr) + b of the block exists
#pragma unroll
          for (int rr = 0; rr < 4; ++rr)
#pragma unroll
            for (int b = 0; b < 2; ++b) ok[rr * 2 + b] = !edge || 2 * (4 * hh + rr) + b < cols_left;
#pragma unroll
          for (int rq = 0; rq < 4; ++rq) {
            const int oy = oy_w + 2 * rq;
            if (oy >= H) continue;  // wave-uniform
            const size_t row_b = img_b + (size_t)(OS * oy + pyc) * Wo_ * c4;
            gchar *yb = (gchar *)(uintptr_t)(reinterpret_cast<char *>(g_y) + row_b);
            const gchar *rb = (const gchar *)(uintptr_t)(reinterpret_cast<const char *>(g_res) + row_b);
            float rv[8];
            if constexpr (has_res) {
#pragma unroll
              for (int rr = 0; rr < 4; ++rr)
#pragma unroll
                for (int b = 0; b < 2; ++b)
                  rv[rr * 2 + b] = ok[rr * 2 + b] ? *reinterpret_cast<cgfloat *>(rb + lane_b + (uint32_t)((2 * rr + b) * 512) * (sx / 512u)) : 0.0f;
            }
#pragma unroll
            for (int rr = 0; rr < 4; ++rr)
#pragma unroll
              for (int b = 0; b < 2; ++b) {
                const int r = rq * 4 + rr;
                float v = keep[b][r];
                if (has_bias) v = v + cbias;
                if constexpr (kind == 1) v = __builtin_fmaxf(v, v * 0.01f);       // act1 leaky (same bits as the select: common.h)
                if constexpr (kind == 2) v = v > 0.0f ? v : 0.0f;                 // act1 relu
                if constexpr (has_res) v = v + rv[rr * 2 + b];
                if constexpr (kind == 3) v = v > 0.0f ? v : 0.0f;                 // act2 relu
                if constexpr (kind == 4) v = __builtin_fmaxf(v, v * 0.01f);       // act2 leaky
                if (ok[rr * 2 + b]) *reinterpret_cast<gfloat *>(yb + lane_b + (uint32_t)((2 * rr + b) * 512) * (sx / 512u)) = v;
              }
          }
        };
        using std::integral_constant;
        // kinds: 0 none; 1 / 2: act1 leaky / relu (act2 none); 3 / 4: act2 relu / leaky (act1 none); anything else -> slow path
        int kind = -1;
        if (act1 == AIVC_ACT_NONE && act2 == AIVC_ACT_NONE) kind = 0;
        else if (act2 == AIVC_ACT_NONE) kind = act1 == AIVC_ACT_LEAKY ? 1 : 2;
        else if (act1 == AIVC_ACT_NONE) kind = act2 == AIVC_ACT_RELU ? 3 : 4;
        if (kind >= 0 && sx % 512u == 0u) {
          auto go = [&](auto RES, auto INSIDE) {
            switch (kind) {
              case 0: rows(RES, integral_constant<int, 0>{}, INSIDE); break;
              case 1: rows(RES, integral_constant<int, 1>{}, INSIDE); break;
              case 2: rows(RES, integral_constant<int, 2>{}, INSIDE); break;
              case 3: rows(RES, integral_constant<int, 3>{}, INSIDE); break;
              default: rows(RES, integral_constant<int, 4>{}, INSIDE); break;
            }
          };
          if (inside_x) {
            if (g_res) go(integral_constant<bool, true>{}, integral_constant<bool, true>{});
            else go(integral_constant<bool, false>{}, integral_constant<bool, true>{});
          } else {
            if (g_res) go(integral_constant<bool, true>{}, integral_constant<bool, false>{});
            else go(integral_constant<bool, false>{}, integral_constant<bool, false>{});
          }
          goto epilogue_done;
        }
      }
      {
        const size_t ybase = (size_t)cur.img * (size_t)Ho_ * Wo_ * Cout + (size_t)co;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int t = (r & 3) + 8 * (r >> 2) + 4 * hh;  // tile of the wave's 4 x 8
          const int oy = oy_w + 2 * (t >> 3), ox0 = 2 * (8 * cur.bxi + (t & 7));
          if (oy >= H) continue;
#pragma unroll
          for (int b = 0; b < 2; ++b) {
            const int ox = ox0 + b;
            if (ox >= W) continue;
            const size_t o = ybase + ((size_t)(OS * oy + pyc) * Wo_ + (size_t)(OS * ox + pxc)) * (size_t)Cout;
            float v = keep[b][r];
            if (has_bias) v = v + cbias;
            v = act_cheap(act1, v);
            if (g_mul) v = g_mul[o] * v;
            if (g_res) v = v + g_res[o];
            v = act_cheap(act2, v);
            g_y[o] = v;
          }
        }
      }
    epilogue_done:;
    }
    if (blk_nxt == WINO_WALK_END) break;
    cur = nxt;
  }
  if (tid == 0) walk.leave();
}

// U = G g G^T per (c_out, c_in), fp64 in the order of include/aivc_hip.h, rounded once
__device__ __forceinline__ void wino_g(double g0, double g1, double g2, double (&out)[4]) {
  out[0] = g0;
  out[1] = 0.5 * ((g0 + g1) + g2);
  out[2] = 0.5 * ((g0 - g1) + g2);
  out[3] = g2;
}

// The three forms of the weight transform differ in where thread idx finds its 3x3 kernel g[r][l] and where its U goes
// (AIVC_WINO_U_INDEX: the staging order of the product kernel); COUNT = transforms per (c_out, c_in) pair.
struct WinoForm3x3 {  // stride-1 3x3: the kernel itself
  static constexpr int COUNT = 1;
  int co, ci, c_in;
  __device__ WinoForm3x3(size_t idx, int, int c_in_) : co((int)(idx / c_in_)), ci((int)(idx % c_in_)), c_in(c_in_) {}
  __device__ double tap(const float *w, int r, int l) const { return (double)w[(((size_t)co * 3 + r) * 3 + l) * c_in + ci]; }
  __device__ size_t out(int pos) const { return AIVC_WINO_U_INDEX(co, pos, ci, c_in); }
};
// 5x5 taps (ky, kx) of (co, ci); zero where ky or kx would be 5
__device__ __forceinline__ double wino_tap5(const float *w, int co, int ci, int c_in, int ky, int kx) {
  return ky < 5 && kx < 5 ? (double)w[(((size_t)co * 5 + ky) * 5 + kx) * c_in + ci] : 0.0;
}
// Polyphase form of the 5x5 stride-2 kernel (include/aivc_hip.h): phase 2 py + px holds the taps ky = 2 r + py, kx = 2 l + px;
// virtual input channel phase * c_in + ci of a 4 c_in-channel layer.
struct WinoFormPoly5 {
  static constexpr int COUNT = 4;
  int co, ci, c_in, phase;
  __device__ WinoFormPoly5(size_t idx, int, int c_in_)
      : co((int)(idx / ((size_t)4 * c_in_))), ci((int)((idx / 4) % c_in_)), c_in(c_in_), phase((int)(idx % 4)) {}
  __device__ double tap(const float *w, int r, int l) const { return wino_tap5(w, co, ci, c_in, 2 * r + (phase >> 1), 2 * l + (phase & 1)); }
  __device__ size_t out(int pos) const { return AIVC_WINO_U_INDEX(co, pos, phase * c_in + ci, 4 * c_in); }
};
// Transposed 5x5 stride-2 kernel, class by class (include/aivc_hip.h): class 2 pyc + pxc holds the taps ky = pyc + 4 - 2 r,
// kx = pxc + 4 - 2 l (r = 0 is zero for pyc = 1); output channel block class * (c_out / 64) + co / 64 of a layer of 4 c_out
// "virtual" output channels.
struct WinoFormTconv5 {
  static constexpr int COUNT = 4;
  int co, ci, c_in, c_out, cls;
  __device__ WinoFormTconv5(size_t idx, int c_out_, int c_in_)
      : co((int)((idx / c_in_) % c_out_)), ci((int)(idx % c_in_)), c_in(c_in_), c_out(c_out_), cls((int)(idx / ((size_t)c_in_ * c_out_))) {}
  __device__ double tap(const float *w, int r, int l) const { return wino_tap5(w, co, ci, c_in, (cls >> 1) + 4 - 2 * r, (cls & 1) + 4 - 2 * l); }
  __device__ size_t out(int pos) const { return AIVC_WINO_U_INDEX(cls * c_out + co, pos, ci, c_in); }
};

template <class FORM>
__global__ void __launch_bounds__(256) winograd_weights_kernel(const float *w, int c_out, int c_in, float *u) {
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (size_t)c_out * c_in * FORM::COUNT) return;
  const FORM f(idx, c_out, c_in);
  double t[4][3], uu[4][4];
#pragma unroll
  for (int l = 0; l < 3; ++l) {
    double col[4];
    wino_g(f.tap(w, 0, l), f.tap(w, 1, l), f.tap(w, 2, l), col);
#pragma unroll
    for (int i = 0; i < 4; ++i) t[i][l] = col[i];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) wino_g(t[i][0], t[i][1], t[i][2], uu[i]);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) u[f.out(4 * i + j)] = (float)uu[i][j];
}

template <class FORM>
static int winograd_weights_launch(const char *what, const float *w, int c_out, int c_in, float *u, hipStream_t s) {
  hipLaunchKernelGGL(winograd_weights_kernel<FORM>, dim3(cdiv((size_t)c_out * c_in * FORM::COUNT, 256)), dim3(256), 0, s, w, c_out, c_in, u);
  return check_launch(what);
}
int winograd_weights(const float *w, int c_out, int c_in, float *u, hipStream_t s) {
  return winograd_weights_launch<WinoForm3x3>("winograd_weights", w, c_out, c_in, u, s);
}
int winograd_weights_poly5(const float *w, int c_out, int c_in, float *u, hipStream_t s) {
  return winograd_weights_launch<WinoFormPoly5>("winograd_weights_poly5", w, c_out, c_in, u, s);
}
int winograd_weights_tconv5(const float *w, int c_out, int c_in, float *u, hipStream_t s) {
  return winograd_weights_launch<WinoFormTconv5>("winograd_weights_tconv5", w, c_out, c_in, u, s);
}

// The block list of a launch: the pixel grid the blocks walk (the output's; transposed form: the input's) in blocks of 16 x 16
// pixels, times the blocks of 64 output channels (transposed form: times the 4 classes)
struct WinoGrid {
  int gh, gw, nby, nbx;  // pixel grid; blocks per image column / row
  uint64_t blocks;       // entries of the block list
};
static WinoGrid wino_grid(const aivc_conv_params &p) {
  const bool tc = p.mode == AIVC_MODE_TCONV;
  const int gh = tc ? p.h_in : p.h_out, gw = tc ? p.w_in : p.w_out, nby = (gh + 15) / 16, nbx = (gw + 15) / 16;
  return {gh, gw, nby, nbx, (uint64_t)p.n * nby * nbx * ((uint64_t)p.c_out / 64) * (tc ? 4 : 1)};
}

// what the kernel can address: 32-bit byte offsets inside one image, a block list that an int counts
bool conv2d_wino_supported(const aivc_conv_params &p) {
  if (!aivc_winograd_covers(&p) || p.gdn) return false;
  if ((uint64_t)p.h_in * p.w_in * p.c_in * 4u >= 0xFFFF0000ull) return false;
  if (p.mode == AIVC_MODE_TCONV && p.c_in > 960) return false;  // (a pixel outside the image reads c_in floats of the 4 KB zero page, one chunk after the other)
  return wino_grid(p).blocks < 0x7FFFFFFFull;
}

int conv2d_wino_variant(const aivc_conv_params &p) { return p.mode == AIVC_MODE_TCONV ? 303 : (p.ksize == 5 ? 302 : 301); }

// The slot set of stream s: launches on one stream run one after the other and share a set (each leaves it zeroed), launches on
// different streams may run at the same time and get different ones.  The sets are zero from the load of the module on, so a
// launch costs no memset and no synchronisation.  When all sets are taken, the set of a stream that has nothing pending (or no
// longer exists) changes hands; -1: WINO_WALK_SETS streams all have work in flight
static int wino_walk_set(hipStream_t s) {
  static std::mutex mu;
  static std::unordered_map<hipStream_t, unsigned> set_of;
  std::lock_guard<std::mutex> lock(mu);
  const auto it = set_of.find(s);
  if (it != set_of.end()) return (int)it->second;
  unsigned set = (unsigned)set_of.size();
  if (set >= WINO_WALK_SETS) {
    auto idle = set_of.begin();
    while (idle != set_of.end() && hipStreamQuery(idle->first) == hipErrorNotReady) ++idle;
    (void)hipGetLastError();  // (a destroyed stream's error is not this launch's)
    if (idle == set_of.end()) return -1;
    set = idle->second;
    set_of.erase(idle);
  }
  set_of.emplace(s, set);
  return (int)set;
}

template <int MODE>
static int wino_launch(const WinoArgs &a, unsigned grid, hipStream_t s) {
  static LdsOptIn opt_in;
  if (!opt_in.raise(reinterpret_cast<const void *>(conv_wino_kernel<MODE>), WINO_LDS)) return check_launch("conv_wino lds attribute");
  const int set = wino_walk_set(s);
  if (set < 0) {
    set_last_error("conv_wino: more streams with launches in flight than block-walk slot sets");
    return AIVC_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(conv_wino_kernel<MODE>, dim3(grid), dim3(512), WINO_LDS, s, a, (uint32_t)set);
  return check_launch("conv_wino");
}

int conv2d_wino(const aivc_conv_params &p, hipStream_t s) {
  if (!conv2d_wino_supported(p) || !p.w_wino) return AIVC_ERR_UNSUPPORTED;
  const bool tc = p.mode == AIVC_MODE_TCONV;
  WinoArgs a;
  a.p = p;
  a.poly = !tc && p.ksize == 5 ? 1 : 0;
  a.cpp_shift = 0;
  while ((8 << a.cpp_shift) < p.c_in) ++a.cpp_shift;  // (polyphase form: c_in / 8 is a power of two, aivc_winograd_covers)
  const WinoGrid g = wino_grid(p);
  a.TH = (g.gh + 1) / 2;
  a.TW = (g.gw + 1) / 2;
  a.nby = g.nby;
  a.nbx = g.nbx;
  a.gy = p.c_out / 64;
  a.total = (int)g.blocks;
  static std::atomic<int> n_cu{0};
  if (n_cu.load(std::memory_order_relaxed) == 0) {
    int dev = 0, cus = 0;
    n_cu = hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0 ? cus : 256;
  }
  // persistent workgroups: min(CUs, blocks) -- one per CU (158 KB of LDS each), or one per block of a list shorter than that
  unsigned grid = (unsigned)n_cu.load(std::memory_order_relaxed);
  if ((unsigned)a.total < grid) grid = (unsigned)a.total;
  if (tc) return wino_launch<2>(a, grid, s);
  return a.poly ? wino_launch<1>(a, grid, s) : wino_launch<0>(a, grid, s);
}

}  // namespace aivc
