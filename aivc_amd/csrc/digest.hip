// digest.hip -- MD5 of many equal-sized device buffers, one message per lane (include/aivc_hip_digest.h).
//
// VALU-bound by construction: a step of RFC 1321 is a chain of about five dependent 32-bit operations (round function, two adds,
// rotate, add), 64 steps per 64-byte block, and nothing of one message runs in parallel.  About 350 vector instructions per block
// and wavefront against four 16-byte loads per lane: the memory system idles, only its LATENCY has to stay out of the chain.  A
// wavefront is alone on its SIMD (64 messages are one wavefront), so nothing else hides a miss: every lane keeps the chunks of the
// next two blocks in registers (a ring of three block images, the loop unrolled by three so that the ring is indexed statically),
// which puts two blocks of arithmetic, more than an HBM miss takes, between a load and its first use.
//
// Each lane streams its own message with aligned 16-byte loads.  A 128-byte line serves two blocks of its lane; the 64 lines a
// wavefront works on are 8 KiB and stay in the vector L1.
//
// A message may start at any byte: lane-private shift = address % 16.  The 64 message bytes of a block are then bytes
// shift .. shift + 63 of five consecutive chunks (the first one left over from the previous block): a per-lane byte funnel
// (v_alignbyte_b32) followed by a per-lane word select in two stages.  Wavefronts whose lanes are all 16-byte aligned (every
// plane stack whose plane size is a multiple of 16, 1080p among them) skip that under one uniform branch.
#include "common.h"
#include "../../include/aivc_hip_digest.h"

namespace aivc {

constexpr int MD5_THREADS = 64;  // one wavefront per workgroup: the wavefronts of a call spread over the CUs

// floor(2^32 * |sin(i + 1)|), RFC 1321 section 3.4
__device__ constexpr uint32_t MD5_K[64] = {
    0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u,
    0x698098d8u, 0x8b44f7afu, 0xffff5bb1u, 0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u,
    0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u, 0xd8a1e681u, 0xe7d3fbc8u,
    0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au,
    0xfffa3942u, 0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u,
    0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u, 0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u,
    0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du, 0x85845dd1u,
    0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
__device__ constexpr int MD5_S[4][4] = {{7, 12, 17, 22}, {5, 9, 14, 20}, {4, 11, 16, 23}, {6, 10, 15, 21}};

// one step: a = b + rotl(a + f(b, c, d) + m + K, s), in the RFC's order of the four registers
template <int I>
__device__ __forceinline__ void md5_step(uint32_t &a, uint32_t b, uint32_t c, uint32_t d, const uint32_t (&m)[16]) {
  constexpr int R = I >> 4;
  constexpr int G = R == 0 ? I : R == 1 ? (5 * I + 1) & 15 : R == 2 ? (3 * I + 5) & 15 : (7 * I) & 15;
  uint32_t f;
  if (R == 0) f = d ^ (b & (c ^ d));       // F: (b & c) | (~b & d)
  else if (R == 1) f = c ^ (d & (b ^ c));  // G: (b & d) | (c & ~d)
  else if (R == 2) f = b ^ c ^ d;          // H
  else f = c ^ (b | ~d);                   // I
  a = b + __builtin_rotateleft32(a + f + m[G] + MD5_K[I], MD5_S[R][I & 3]);
}

template <int I>
__device__ __forceinline__ void md5_steps4(uint32_t &a, uint32_t &b, uint32_t &c, uint32_t &d, const uint32_t (&m)[16]) {
  md5_step<I>(a, b, c, d, m);
  md5_step<I + 1>(d, a, b, c, m);
  md5_step<I + 2>(c, d, a, b, m);
  md5_step<I + 3>(b, c, d, a, m);
}

__device__ __forceinline__ void md5_block(uint32_t (&h)[4], const uint32_t (&m)[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3];
  md5_steps4<0>(a, b, c, d, m), md5_steps4<4>(a, b, c, d, m), md5_steps4<8>(a, b, c, d, m), md5_steps4<12>(a, b, c, d, m);
  md5_steps4<16>(a, b, c, d, m), md5_steps4<20>(a, b, c, d, m), md5_steps4<24>(a, b, c, d, m), md5_steps4<28>(a, b, c, d, m);
  md5_steps4<32>(a, b, c, d, m), md5_steps4<36>(a, b, c, d, m), md5_steps4<40>(a, b, c, d, m), md5_steps4<44>(a, b, c, d, m);
  md5_steps4<48>(a, b, c, d, m), md5_steps4<52>(a, b, c, d, m), md5_steps4<56>(a, b, c, d, m), md5_steps4<60>(a, b, c, d, m);
  h[0] += a, h[1] += b, h[2] += c, h[3] += d;
}

typedef uint32_t chunk_t __attribute__((ext_vector_type(4)));  // one aligned 16-byte chunk
typedef const chunk_t __attribute__((address_space(1))) *chunk_ptr;  // in global memory: global_load, not flat_load

// Four consecutive chunks of a lane's stream starting at chunk c.  A chunk at or past n_chunks holds no message byte and is not
// read: the lane's last chunk is read in its place (no branch; pad_words() overwrites whatever lies behind the message's end).
// n_chunks > 0.
__device__ __forceinline__ void load_chunks(chunk_t (&dst)[4], chunk_ptr base, int32_t c, int32_t n_chunks) {
#pragma unroll
  for (int q = 0; q < 4; ++q) dst[q] = base[min(c + q, n_chunks - 1)];
}

// the 16 message words of a block from the chunk before it (`carry`) and its own four: bytes shift .. shift + 63 of the 80
__device__ __forceinline__ void block_words(uint32_t (&m)[16], const chunk_t &carry, const chunk_t (&cur)[4], uint32_t shift, bool any_shift) {
  uint32_t src[20] = {carry.x,  carry.y,  carry.z,  carry.w,  cur[0].x, cur[0].y, cur[0].z, cur[0].w, cur[1].x, cur[1].y,
                      cur[1].z, cur[1].w, cur[2].x, cur[2].y, cur[2].z, cur[2].w, cur[3].x, cur[3].y, cur[3].z, cur[3].w};
  if (!any_shift) {  // (wave-uniform)
#pragma unroll
    for (int i = 0; i < 16; ++i) m[i] = src[i];
    return;
  }
  const uint32_t bs = shift & 3u;
  // word shift of 0 .. 3 as two bit selects (v_bfi_b32) under lane masks: written as selects of array elements, the compiler
  // turns the pair into a dynamically indexed private array, which lives in scratch memory
  const uint32_t w1 = 0u - ((shift >> 2) & 1u), w2 = 0u - ((shift >> 3) & 1u);
  uint32_t t[19], s[18];
#pragma unroll
  for (int j = 0; j < 19; ++j) t[j] = __builtin_amdgcn_alignbyte(src[j + 1], src[j], bs);  // ({hi, lo} >> 8 bs), low word
#pragma unroll
  for (int j = 0; j < 18; ++j) s[j] = (t[j + 1] & w1) | (t[j] & ~w1);
#pragma unroll
  for (int i = 0; i < 16; ++i) m[i] = (s[i + 2] & w2) | (s[i] & ~w2);
}

// RFC 1321 section 3.1 / 3.2 on the words of block `blk` (one that holds the message's end or lies behind it): the byte 0x80
// behind the last message byte, zeros, and in the last block the bit count.  len is uniform: scalar control flow.
__device__ __forceinline__ void pad_words(uint32_t (&m)[16], int64_t blk, int64_t len, bool last) {
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int64_t rem = len - (blk * 64 + 4 * i);  // message bytes from this word on
    if (rem >= 4) continue;
    if (rem <= 0) {
      m[i] = rem == 0 ? 0x80u : 0u;
    } else {
      const uint32_t bits = 8u * (uint32_t)rem;
      m[i] = (m[i] & ((1u << bits) - 1u)) | (0x80u << bits);
    }
  }
  if (last) {
    m[14] = (uint32_t)((uint64_t)len << 3);
    m[15] = (uint32_t)((uint64_t)len >> 29);
  }
}

__global__ __launch_bounds__(MD5_THREADS) void md5_lanes_kernel(const uint8_t *const *__restrict__ msgs, int64_t len, int n,
                                                                uint8_t *__restrict__ digests) {
  const int lane_msg = blockIdx.x * MD5_THREADS + threadIdx.x;
  if (lane_msg >= n) return;
  const uintptr_t addr = len > 0 ? reinterpret_cast<uintptr_t>(msgs[lane_msg]) : 0;
  const uint32_t shift = (uint32_t)(addr & 15u);
  chunk_ptr base = (chunk_ptr)(addr - shift);
  const int32_t n_chunks = (int32_t)(((int64_t)shift + len + 15) >> 4);  // chunks with at least one message byte: <= 2^27 + 1
  const int64_t n_full = len >> 6;                             // blocks of message bytes only
  const int64_t n_blocks = ((len + 8) >> 6) + 1;               // ... and with 0x80, the zeros and the bit count
  const bool any_shift = __builtin_amdgcn_ballot_w64(shift != 0) != 0;

  uint32_t h[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
  // ring[k] holds chunks 4 b + 1 .. 4 b + 4 of the block b with b % 3 == k; chunk 4 b, its first, is the last of block b - 1
  chunk_t ring[3][4] = {};
  chunk_t carry = {};
  if (len > 0) {  // (uniform)
    carry = base[0];
    load_chunks(ring[0], base, 1, n_chunks);
    load_chunks(ring[1], base, 5, n_chunks);
  }
  for (int64_t b0 = 0; b0 < n_blocks; b0 += 3) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int64_t b = b0 + k;
      if (b >= n_blocks) break;
      uint32_t m[16];
      block_words(m, carry, ring[k], shift, any_shift);
      carry = ring[k][3];
      if (len > 0) load_chunks(ring[(k + 2) % 3], base, (int32_t)(4 * (b + 2) + 1), n_chunks);  // (the slot of block b - 1: free)
      if (b >= n_full) pad_words(m, b, len, b == n_blocks - 1);
      md5_block(h, m);
    }
  }

  uint8_t *out = digests + (size_t)lane_msg * 16;
  if ((reinterpret_cast<uintptr_t>(digests) & 15u) == 0) {
    *reinterpret_cast<uint4 *>(out) = make_uint4(h[0], h[1], h[2], h[3]);
  } else {
#pragma unroll
    for (int i = 0; i < 16; ++i) out[i] = (uint8_t)(h[i >> 2] >> (8 * (i & 3)));
  }
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_md5_batch(const uint8_t *const *msgs, int64_t len, int32_t n, uint8_t *digests, aivc_stream_t stream) {
  if (n < 0) return AIVC_ERR_ARG;
  if (n == 0) return AIVC_OK;
  if (!msgs || !digests || len < 0 || len >= ((int64_t)1 << 31)) return AIVC_ERR_ARG;
  hipLaunchKernelGGL(md5_lanes_kernel, dim3(cdiv((size_t)n, MD5_THREADS)), dim3(MD5_THREADS), 0, to_stream(stream), msgs, len, n,
                     digests);
  return check_launch("md5_batch");
}
