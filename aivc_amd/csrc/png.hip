// png.hip -- PNG coding of 8-bit pictures: row filters and a per-segment dynamic-Huffman deflate (include/aivc_hip_png.h, where the
// filtered stream, the segments and the sizes are stated).
//
// Three kernels.  png_filter_kernel: a wavefront per row writes the filtered row into its segment of `filt` (filter 5 first sums
// the five candidates' absolute residuals over the wave).  png_segment_kernel: a workgroup of 256 per segment.  It walks the
// segment in tiles of 256 chunks of AIVC_PNG_RUN bytes held in LDS, a lane per chunk -- once for the histogram (LDS atomics)
// and the Adler sums, then, with the code tables built, once to code.  A lane tokenizes its chunk serially: a literal, then a
// distance-1 match for the rest of a run of equal bytes where that is 3 or more; runs end with the chunk, so lanes need nothing
// from each other but the bit offset of their first token, a workgroup prefix sum.  The tokens are OR-ed into a window of
// zeroed LDS words at their bit offset and the window's whole words go to the slot after every tile, the partial word carried
// over.  The tables are one lane's work between two barriers: the symbols arrive sorted by count (a rank sort by all lanes), the
// tree is the two-queue merge, depths beyond the limit are folded by moving leaves down until the Kraft sum is exact, and the
// lengths go back to the symbols in sorted order.  png_gather_kernel packs the slots of a picture behind one another.
// The header's size and the body's size follow from the histogram and the lengths, so stored-or-coded is decided before a bit of
// the body is written and a slot is never overrun.
#include "reduce.h"
#include "../../include/aivc_hip_png.h"

namespace aivc {

constexpr int PNG_THREADS = 256;
constexpr int PNG_CHUNK = AIVC_PNG_RUN;                 // bytes per lane and tile
constexpr int PNG_CHUNK_WORDS = PNG_CHUNK / 4 + 1;      // a chunk's stride in LDS: odd, so the lanes' byte reads spread over the banks
constexpr int PNG_TILE = PNG_THREADS * PNG_CHUNK;       // bytes per tile
constexpr int PNG_OUT_WORDS = PNG_TILE * 15 / 32 + 8;   // a tile codes to at most 15 bits per byte (a match: 18 bits for >= 3 bytes)
constexpr int PNG_SYMS = 286, PNG_EOB = 256;
constexpr int PNG_CL_SYMS = 19;
constexpr uint32_t ADLER_MOD = 65521;
static_assert(PNG_CHUNK >= 4 && PNG_CHUNK % 4 == 0 && PNG_CHUNK <= 34, "run lengths 3 ... 34 take the codes 257 ... 272, at most 2 extra bits");

struct PngGeom {
  int32_t n, h, c, rps, nseg;
  int64_t rb;          // w c
  int64_t seg_stride, slot_bytes;
  int64_t rows, segs;  // of the batch
};

// ---- filter -------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t paeth(int a, int b, int d) {
  const int p = a + b - d;
  const int pa = p > a ? p - a : a - p, pb = p > b ? p - b : b - p, pd = p > d ? p - d : d - p;
  return (uint32_t)(pa <= pb && pa <= pd ? a : pb <= pd ? b : d);
}

__device__ __forceinline__ uint32_t predict(int type, uint32_t a, uint32_t b, uint32_t d) {
  return type == 0 ? 0u : type == 1 ? a : type == 2 ? b : type == 3 ? (a + b) >> 1 : paeth((int)a, (int)b, (int)d);
}

__device__ __forceinline__ uint32_t abs_s8(uint32_t v) { v &= 255u; return v < 128u ? v : 256u - v; }

__global__ void __launch_bounds__(PNG_THREADS) png_filter_kernel(const uint8_t *__restrict__ pix, PngGeom g, int filter, uint8_t *__restrict__ filt) {
  const int64_t row = (int64_t)blockIdx.x * (PNG_THREADS / 64) + (threadIdx.x >> 6);
  if (row >= g.rows) return;  // (whole wavefronts leave; no barrier follows)
  const int lane = threadIdx.x & 63;
  const int64_t p = row / g.h;
  const int32_t r = (int32_t)(row % g.h);
  const uint8_t *cur = pix + (size_t)row * g.rb;
  const uint8_t *up = cur - g.rb;  // read only where r > 0
  const bool has_up = r > 0;
  const int c = g.c;
  int type = filter;
  if (filter == 5) {
    uint64_t sum[5] = {0, 0, 0, 0, 0};
    for (int64_t i = lane; i < g.rb; i += 64) {
      const uint32_t x = cur[i], a = i >= c ? cur[i - c] : 0u, b = has_up ? up[i] : 0u, d = has_up && i >= c ? up[i - c] : 0u;
#pragma unroll
      for (int t = 0; t < 5; ++t) sum[t] += abs_s8(x - predict(t, a, b, d));
    }
    uint64_t best = 0;
#pragma unroll
    for (int t = 0; t < 5; ++t) {
      const uint64_t s = (uint64_t)__shfl((unsigned long long)wave_sum_u64(sum[t]), 0, 64);
      if (t == 0 || s < best) best = s, type = t;  // (the lowest type among equals)
    }
  }
  uint8_t *dst = filt + ((size_t)p * g.nseg + r / g.rps) * g.seg_stride + (size_t)(r % g.rps) * (g.rb + 1);
  if (lane == 0) dst[0] = (uint8_t)type;
  for (int64_t i = lane; i < g.rb; i += 64) {
    const uint32_t x = cur[i], a = i >= c ? cur[i - c] : 0u, b = has_up ? up[i] : 0u, d = has_up && i >= c ? up[i - c] : 0u;
    dst[1 + i] = (uint8_t)(x - predict(type, a, b, d));
  }
}

// ---- code tables (one lane) -----------------------------------------------------------------------------------------------------
// n >= 2 symbols, sorted[0 .. n) ascending by (count, symbol): optimal code lengths limited to maxlen -> len[symbol]; bl[l]: how
// many symbols got length l.  w, parent: 2 n scratch words each.  n <= 2^maxlen.
__device__ void code_lengths(int n, const uint16_t *sorted, const uint32_t *freq, int maxlen, uint8_t *len, uint32_t *bl,
                             uint32_t *w, uint16_t *parent) {
  for (int i = 0; i < n; ++i) w[i] = freq[sorted[i]];
  int leaf = 0, inner = n;  // the two queues: leaves by count, inner nodes in the order they were made (their weights ascend)
  for (int next = n; next < 2 * n - 1; ++next) {
    uint32_t sum = 0;
    for (int k = 0; k < 2; ++k) {
      const int pick = (leaf < n && (inner >= next || w[leaf] <= w[inner])) ? leaf++ : inner++;
      sum += w[pick];
      parent[pick] = (uint16_t)next;
    }
    w[next] = sum;
  }
  w[2 * n - 2] = 0;  // w becomes the depth of the inner nodes
  for (int k = 2 * n - 3; k >= n; --k) w[k] = w[parent[k]] + 1;
  for (int l = 0; l <= maxlen; ++l) bl[l] = 0;
  for (int i = 0; i < n; ++i) {
    const uint32_t d = w[parent[i]] + 1;
    bl[d < (uint32_t)maxlen ? d : maxlen] += 1;
  }
  // the Kraft sum in units of 2^-maxlen: folding deep leaves up to maxlen made it too large.  Each step takes one leaf off the
  // last level and hangs it, with a leaf of the deepest level above that has one, under a new node in that leaf's place: -1.
  uint32_t total = 0;
  for (int l = 1; l <= maxlen; ++l) total += bl[l] << (maxlen - l);
  while (total > (1u << maxlen)) {
    bl[maxlen] -= 1;
    for (int l = maxlen - 1; l >= 1; --l)
      if (bl[l]) {
        bl[l] -= 1;
        bl[l + 1] += 2;
        break;
      }
    total -= 1;
  }
  int at = 0;
  for (int l = maxlen; l >= 1; --l)
    for (uint32_t k = 0; k < bl[l]; ++k) len[sorted[at++]] = (uint8_t)l;
}

// canonical codes of len[0 .. nsym), bit-reversed (deflate packs a code from its most significant bit, everything else from the least)
__device__ void canonical_codes(int nsym, const uint8_t *len, const uint32_t *bl, int maxlen, uint32_t *next, uint16_t *code) {
  uint32_t c = 0;
  for (int l = 1; l <= maxlen; ++l) {
    c = (c + (l > 1 ? bl[l - 1] : 0u)) << 1;
    next[l] = c;
  }
  for (int s = 0; s < nsym; ++s)
    if (len[s]) code[s] = (uint16_t)(__brev(next[len[s]]++) >> (32 - len[s]));
}

__device__ __forceinline__ uint32_t length_symbol(uint32_t run, uint32_t &extra_bits, uint32_t &extra) {  // run 3 ... 34
  const uint32_t l = run - 3;
  extra_bits = l < 8 ? 0u : (uint32_t)(31 - __clz((int)l)) - 2u;
  extra = l & ((1u << extra_bits) - 1u);
  return 257u + 4u * extra_bits + (l >> extra_bits);
}

__device__ __forceinline__ uint32_t length_extra_bits(int sym) { return sym < 265 || sym == 285 ? 0u : (uint32_t)(sym - 261) >> 2; }

// nbits <= 25 bits at bit `pos` of the zeroed words out[]
__device__ __forceinline__ void put_bits(uint32_t *out, uint32_t pos, uint32_t bits, uint32_t nbits) {
  const uint32_t word = pos >> 5, sh = pos & 31u;
  atomicOr(&out[word], bits << sh);
  if (sh + nbits > 32u) atomicOr(&out[word + 1], bits >> (32u - sh));
}

// the tokens of the nb bytes at chunk[]: lit(value), match(run of 3 ... PNG_CHUNK - 1 bytes at distance 1)
template <typename L, typename M>
__device__ __forceinline__ void tokenize(const uint8_t *chunk, int nb, L lit, M match) {
  int i = 0;
  while (i < nb) {
    const uint32_t v = chunk[i];
    int j = i + 1;
    while (j < nb && chunk[j] == v) ++j;
    const int run = j - i - 1;
    lit(v);
    if (run >= 3) {
      match((uint32_t)run);
    } else {
      for (int k = 0; k < run; ++k) lit(v);
    }
    i = j;
  }
}

struct PngTables {
  uint32_t hist[PNG_SYMS + 2];
  uint16_t code[PNG_SYMS + 2];
  uint8_t len[PNG_SYMS + 2];
  uint16_t sorted[PNG_SYMS + 2];
  uint32_t w[2 * PNG_SYMS];
  uint16_t parent[2 * PNG_SYMS];
  uint32_t bl[16], next[16];
  uint8_t cl_sym[PNG_SYMS + 4], cl_ext[PNG_SYMS + 4];  // the header's code-length tokens
  uint32_t cl_freq[PNG_CL_SYMS];
  uint16_t cl_sorted[PNG_CL_SYMS], cl_code[PNG_CL_SYMS];
  uint8_t cl_len[PNG_CL_SYMS];
  uint32_t n_used, coded, header_bits, scan[PNG_THREADS / 64];
  uint64_t red[2][PNG_THREADS / 64];
};

// lane 0: everything between the histogram and the first body bit.  -> T.coded (0: stored blocks), T.header_bits, header in out[]
__device__ void build_block_header(PngTables &T, uint32_t *out, uint32_t seg_len) {
  const int n = (int)T.n_used;
  for (int s = 0; s < PNG_SYMS + 2; ++s) T.len[s] = 0;
  code_lengths(n, T.sorted, T.hist, 15, T.len, T.bl, T.w, T.parent);
  canonical_codes(PNG_SYMS, T.len, T.bl, 15, T.next, T.code);
  int hlit = PNG_SYMS;
  while (hlit > 257 && T.len[hlit - 1] == 0) --hlit;
  uint32_t n_match = 0;
  uint64_t body_bits = 0;
  for (int s = 0; s < hlit; ++s) {
    body_bits += (uint64_t)T.hist[s] * (T.len[s] + length_extra_bits(s));
    if (s > PNG_EOB) n_match += T.hist[s];
  }
  body_bits += n_match;  // the one distance code, 1 bit
  // the lengths the header states: hlit literal/length codes, then the one distance code (1 bit if a match uses it, else none)
  const uint8_t keep = T.len[hlit];
  T.len[hlit] = n_match ? 1 : 0;
  const int n_len = hlit + 1;
  for (int s = 0; s < PNG_CL_SYMS; ++s) T.cl_freq[s] = 0, T.cl_len[s] = 0;
  int n_tok = 0;
  for (int i = 0; i < n_len;) {
    const uint8_t v = T.len[i];
    int run = 1;
    while (i + run < n_len && T.len[i + run] == v) ++run;
    i += run;
    if (v == 0) {
      while (run >= 11) {
        const int take = run < 138 ? run : 138;
        T.cl_sym[n_tok] = 18, T.cl_ext[n_tok++] = (uint8_t)(take - 11), run -= take;
      }
      if (run >= 3) T.cl_sym[n_tok] = 17, T.cl_ext[n_tok++] = (uint8_t)(run - 3), run = 0;
    } else {
      T.cl_sym[n_tok] = v, T.cl_ext[n_tok++] = 0, run -= 1;
      while (run >= 3) {
        const int take = run < 6 ? run : 6;
        T.cl_sym[n_tok] = 16, T.cl_ext[n_tok++] = (uint8_t)(take - 3), run -= take;
      }
    }
    for (; run > 0; --run) T.cl_sym[n_tok] = v, T.cl_ext[n_tok++] = 0;
  }
  T.len[hlit] = keep;
  for (int t = 0; t < n_tok; ++t) T.cl_freq[T.cl_sym[t]] += 1;
  int n_cl = 0;
  for (int s = 0; s < PNG_CL_SYMS; ++s) {  // insertion sort by (count, symbol)
    if (!T.cl_freq[s]) continue;
    int at = n_cl++;
    while (at > 0 && T.cl_freq[T.cl_sorted[at - 1]] > T.cl_freq[s]) T.cl_sorted[at] = T.cl_sorted[at - 1], --at;
    T.cl_sorted[at] = (uint16_t)s;
  }
  // (257 or more lengths that are not all zero always give two token kinds -- a length and a repeat or a zero -- so this guard
  // is not expected to fire; code_lengths needs n >= 2, and inflate a complete code: a second, unused symbol of 1 bit)
  if (n_cl == 1) {
    T.cl_len[T.cl_sorted[0]] = 1, T.cl_len[T.cl_sorted[0] == 0 ? 1 : 0] = 1;
    for (int l = 0; l <= 7; ++l) T.bl[l] = l == 1 ? 2 : 0;
  } else {
    code_lengths(n_cl, T.cl_sorted, T.cl_freq, 7, T.cl_len, T.bl, T.w, T.parent);
  }
  canonical_codes(PNG_CL_SYMS, T.cl_len, T.bl, 7, T.next, T.cl_code);
  const uint8_t order[PNG_CL_SYMS] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
  int hclen = PNG_CL_SYMS;
  while (hclen > 4 && T.cl_len[order[hclen - 1]] == 0) --hclen;
  uint32_t header_bits = 3 + 5 + 5 + 4 + 3 * hclen;
  for (int t = 0; t < n_tok; ++t) {
    const int s = T.cl_sym[t];
    header_bits += T.cl_len[s] + (s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0);
  }
  const uint64_t coded_bytes = (header_bits + body_bits + 3 + 7) / 8 + 4;  // ... the empty stored block: 3 bits, to the byte, 00 00 FF FF
  const uint64_t stored_bytes = (uint64_t)seg_len + 5ull * ((seg_len + 65534u) / 65535u);
  T.coded = coded_bytes < stored_bytes;
  T.header_bits = header_bits;
  if (!T.coded) return;
  uint32_t pos = 0;
  put_bits(out, pos, 0u, 1), pos += 1;  // not the final block
  put_bits(out, pos, 2u, 2), pos += 2;  // dynamic codes
  put_bits(out, pos, (uint32_t)(hlit - 257), 5), pos += 5;
  put_bits(out, pos, 0u, 5), pos += 5;  // one distance code
  put_bits(out, pos, (uint32_t)(hclen - 4), 4), pos += 4;
  for (int k = 0; k < hclen; ++k) put_bits(out, pos, T.cl_len[order[k]], 3), pos += 3;
  for (int t = 0; t < n_tok; ++t) {
    const int s = T.cl_sym[t];
    put_bits(out, pos, T.cl_code[s], T.cl_len[s]), pos += T.cl_len[s];
    const uint32_t eb = s == 16 ? 2 : s == 17 ? 3 : s == 18 ? 7 : 0;
    if (eb) put_bits(out, pos, T.cl_ext[t], eb), pos += eb;
  }
}

// ---- the segment coder -----------------------------------------------------------------------------------------------------------
// the bytes [t0, t0 + PNG_TILE) of the segment -> LDS, chunk k at word k PNG_CHUNK_WORDS (aligned dwords; src is 16-byte aligned)
__device__ __forceinline__ void load_tile(const uint8_t *src, uint32_t t0, uint32_t seg_len, uint32_t *tile) {
  const uint32_t left = seg_len - t0, nwords = ((left < (uint32_t)PNG_TILE ? left : (uint32_t)PNG_TILE) + 3u) / 4u;
  const uint32_t *srcw = reinterpret_cast<const uint32_t *>(src + t0);
  for (uint32_t d = threadIdx.x; d < nwords; d += PNG_THREADS) tile[(d / (PNG_CHUNK / 4)) * PNG_CHUNK_WORDS + d % (PNG_CHUNK / 4)] = srcw[d];
}

// v over the workgroup: -> the sum of the lanes in front of this one; total: of all
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t *wave_sums, uint32_t &total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint32_t incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(incl, d, 64);
    if (lane >= d) incl += t;
  }
  if (lane == 63) wave_sums[wave] = incl;
  __syncthreads();
  uint32_t base = 0;
  total = 0;
#pragma unroll
  for (int k = 0; k < PNG_THREADS / 64; ++k) {
    if (k < wave) base += wave_sums[k];
    total += wave_sums[k];
  }
  __syncthreads();
  return base + incl - v;
}

__global__ void __launch_bounds__(PNG_THREADS) png_segment_kernel(const uint8_t *__restrict__ filt, PngGeom g, uint8_t *__restrict__ slots,
                                                                  uint32_t *__restrict__ seg_info) {
  __shared__ uint32_t tile[PNG_THREADS * PNG_CHUNK_WORDS];
  __shared__ uint32_t out[PNG_OUT_WORDS];
  __shared__ PngTables T;
  const int tid = threadIdx.x;
  const int64_t seg = blockIdx.x;
  const int32_t s = (int32_t)(seg % g.nseg);
  const int32_t rows = g.h - s * g.rps < g.rps ? g.h - s * g.rps : g.rps;
  const uint32_t seg_len = (uint32_t)(rows * (g.rb + 1));
  const uint8_t *src = filt + (size_t)seg * g.seg_stride;
  uint8_t *slot = slots + (size_t)seg * g.slot_bytes;
  const uint8_t *chunk = reinterpret_cast<const uint8_t *>(tile) + tid * (PNG_CHUNK_WORDS * 4);

  for (int k = tid; k < PNG_SYMS + 2; k += PNG_THREADS) T.hist[k] = 0;
  for (int k = tid; k < PNG_OUT_WORDS; k += PNG_THREADS) out[k] = 0;
  if (tid == 0) T.n_used = 0;
  __syncthreads();

  // pass 1: histogram, Adler sums
  uint64_t s1 = 0, s2 = 0;
  for (uint32_t t0 = 0; t0 < seg_len; t0 += PNG_TILE) {
    load_tile(src, t0, seg_len, tile);
    __syncthreads();
    const uint32_t at = t0 + (uint32_t)tid * PNG_CHUNK;
    const int nb = at >= seg_len ? 0 : seg_len - at < (uint32_t)PNG_CHUNK ? (int)(seg_len - at) : PNG_CHUNK;
    for (int i = 0; i < nb; ++i) {
      const uint32_t b = chunk[i];
      s1 += b;
      s2 += (uint64_t)(seg_len - at - (uint32_t)i) * b;
    }
    tokenize(chunk, nb, [&](uint32_t v) { atomicAdd(&T.hist[v], 1u); },
             [&](uint32_t run) {
               uint32_t eb, ev;
               atomicAdd(&T.hist[length_symbol(run, eb, ev)], 1u);
             });
    __syncthreads();
  }
  s1 = wave_sum_u64(s1), s2 = wave_sum_u64(s2);
  if ((tid & 63) == 0) T.red[0][tid >> 6] = s1, T.red[1][tid >> 6] = s2;
  if (tid == 0) T.hist[PNG_EOB] = 1;
  __syncthreads();

  // the symbols in use, ascending by (count, symbol): every lane ranks its own
  for (int sym = tid; sym < PNG_SYMS; sym += PNG_THREADS) {
    const uint32_t cnt = T.hist[sym];
    if (!cnt) continue;
    int rank = 0;
    for (int j = 0; j < PNG_SYMS; ++j) {
      const uint32_t o = T.hist[j];
      rank += o != 0 && (o < cnt || (o == cnt && j < sym));
    }
    T.sorted[rank] = (uint16_t)sym;
    atomicAdd(&T.n_used, 1u);
  }
  __syncthreads();
  if (tid == 0) {
    uint64_t a = 0, b = 0;
    for (int k = 0; k < PNG_THREADS / 64; ++k) a += T.red[0][k], b += T.red[1][k];
    seg_info[seg * AIVC_PNG_SEG_WORDS + 1] = (uint32_t)(a % ADLER_MOD);
    seg_info[seg * AIVC_PNG_SEG_WORDS + 2] = (uint32_t)(b % ADLER_MOD);
    seg_info[seg * AIVC_PNG_SEG_WORDS + 3] = 0;
    build_block_header(T, out, seg_len);
  }
  __syncthreads();

  if (!T.coded) {  // stored blocks: 00, LEN, ~LEN, the bytes
    const uint32_t nblk = (seg_len + 65534u) / 65535u;
    for (uint32_t k = tid; k < nblk; k += PNG_THREADS) {
      const uint32_t l = seg_len - k * 65535u < 65535u ? seg_len - k * 65535u : 65535u;
      uint8_t *hd = slot + (size_t)k * 65540u;
      hd[0] = 0, hd[1] = (uint8_t)l, hd[2] = (uint8_t)(l >> 8), hd[3] = (uint8_t)~l, hd[4] = (uint8_t)(~l >> 8);
    }
    for (uint32_t i = tid; i < seg_len; i += PNG_THREADS) slot[(size_t)i + 5u * (i / 65535u + 1u)] = src[i];
    if (tid == 0) seg_info[seg * AIVC_PNG_SEG_WORDS] = seg_len + 5u * nblk;
    return;
  }

  // pass 2: the window out[] holds `win` bits; its whole words go to the slot, the partial one stays as word 0
  uint32_t *slotw = reinterpret_cast<uint32_t *>(slot);
  uint32_t win = T.header_bits, flushed = 0;  // (flushed: words in the slot)
  auto flush = [&]() {
    const uint32_t nfull = win >> 5;
    for (uint32_t k = tid; k < nfull; k += PNG_THREADS) slotw[flushed + k] = out[k];
    const uint32_t carry = out[nfull];
    __syncthreads();
    for (uint32_t k = tid; k <= nfull; k += PNG_THREADS) out[k] = k == 0 ? carry : 0u;
    flushed += nfull, win &= 31u;
    __syncthreads();
  };
  flush();
  for (uint32_t t0 = 0; t0 < seg_len; t0 += PNG_TILE) {
    load_tile(src, t0, seg_len, tile);
    __syncthreads();
    const uint32_t at = t0 + (uint32_t)tid * PNG_CHUNK;
    const int nb = at >= seg_len ? 0 : seg_len - at < (uint32_t)PNG_CHUNK ? (int)(seg_len - at) : PNG_CHUNK;
    uint32_t bits = 0;
    tokenize(chunk, nb, [&](uint32_t v) { bits += T.len[v]; },
             [&](uint32_t run) {
               uint32_t eb, ev;
               bits += T.len[length_symbol(run, eb, ev)] + eb + 1u;
             });
    uint32_t total;
    uint32_t pos = win + block_scan(bits, T.scan, total);
    tokenize(chunk, nb, [&](uint32_t v) { put_bits(out, pos, T.code[v], T.len[v]), pos += T.len[v]; },
             [&](uint32_t run) {
               uint32_t eb, ev;
               const uint32_t sym = length_symbol(run, eb, ev), l = T.len[sym];
               put_bits(out, pos, T.code[sym] | (ev << l), l + eb + 1u), pos += l + eb + 1u;  // (the distance code is the bit 0)
             });
    __syncthreads();
    win += total;
    flush();
  }
  if (tid == 0) {  // end of block, then the empty stored block: 3 bits, to the byte, 00 00 FF FF
    put_bits(out, win, T.code[PNG_EOB], T.len[PNG_EOB]);
    uint32_t pos = (win + T.len[PNG_EOB] + 3u + 7u) & ~7u;
    pos += 16u;
    put_bits(out, pos, 0xffffu, 16), pos += 16u;
    T.scan[0] = pos;
  }
  __syncthreads();
  const uint32_t end_bits = T.scan[0];
  for (uint32_t k = tid; k < (end_bits + 31u) >> 5; k += PNG_THREADS) slotw[flushed + k] = out[k];
  if (tid == 0) seg_info[seg * AIVC_PNG_SEG_WORDS] = flushed * 4u + end_bits / 8u;
}

// ---- gather -------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(PNG_THREADS) png_gather_kernel(const uint8_t *__restrict__ slots, const uint32_t *__restrict__ seg_info,
                                                                 const uint64_t *__restrict__ dst, PngGeom g, uint8_t *__restrict__ out) {
  const int64_t seg = blockIdx.x;
  const int32_t s = (int32_t)(seg % g.nseg);
  const uint32_t nbytes = seg_info[seg * AIVC_PNG_SEG_WORDS];
  const uint8_t *src = slots + (size_t)seg * g.slot_bytes;
  uint8_t *d = out + dst[seg];
  for (uint32_t i = threadIdx.x; i < nbytes; i += PNG_THREADS) d[i] = src[i];
  if (s == 0 && threadIdx.x == 0) d[-2] = 0x78, d[-1] = 0x01;
  if (s == g.nseg - 1 && threadIdx.x == 64) {
    uint8_t *e = d + nbytes;
    e[0] = 1, e[1] = 0, e[2] = 0, e[3] = 0xff, e[4] = 0xff;
  }
}

static int png_geometry(int32_t n, int32_t h, int32_t w, int32_t c, int32_t rps, PngGeom &g) {
  if (n < 1 || h < 1 || w < 1 || rps < 1 || (c != 1 && c != 3)) return AIVC_ERR_ARG;
  g.n = n, g.h = h, g.c = c;
  g.rps = rps < h ? rps : h;
  g.rb = (int64_t)w * c;
  g.nseg = (h + g.rps - 1) / g.rps;
  const int64_t len = (int64_t)g.rps * (g.rb + 1);
  if (len >= (int64_t)1 << 31) return AIVC_ERR_UNSUPPORTED;
  g.seg_stride = (len + 15) / 16 * 16;
  g.slot_bytes = (len + 5 * ((len + 65534) / 65535) + 4 + 15) / 16 * 16;
  g.rows = (int64_t)n * h;
  g.segs = (int64_t)n * g.nseg;
  if (g.rows > 0x7fffffff) return AIVC_ERR_UNSUPPORTED;
  return AIVC_OK;
}

}  // namespace aivc

using namespace aivc;

AIVC_EXPORT int aivc_png_deflate(const uint8_t *pix, int32_t n, int32_t h, int32_t w, int32_t c, int32_t filter, int32_t rows_per_segment,
                                 uint8_t *filt, uint8_t *slots, uint32_t *seg_info, aivc_stream_t stream) {
  if (!pix || !filt || !slots || !seg_info || filter < 0 || filter > 5) return AIVC_ERR_ARG;
  PngGeom g;
  if (const int err = png_geometry(n, h, w, c, rows_per_segment, g)) return err;
  hipLaunchKernelGGL(png_filter_kernel, dim3(cdiv((size_t)g.rows, PNG_THREADS / 64)), dim3(PNG_THREADS), 0, to_stream(stream), pix, g, filter, filt);
  if (const int err = check_launch("png_deflate (filter)")) return err;
  hipLaunchKernelGGL(png_segment_kernel, dim3((unsigned)g.segs), dim3(PNG_THREADS), 0, to_stream(stream), filt, g, slots, seg_info);
  return check_launch("png_deflate (segments)");
}

AIVC_EXPORT int aivc_png_gather(const uint8_t *slots, const uint32_t *seg_info, const uint64_t *dst, int32_t n, int32_t h, int32_t w,
                                int32_t c, int32_t rows_per_segment, uint8_t *out, aivc_stream_t stream) {
  if (!slots || !seg_info || !dst || !out) return AIVC_ERR_ARG;
  PngGeom g;
  if (const int err = png_geometry(n, h, w, c, rows_per_segment, g)) return err;
  hipLaunchKernelGGL(png_gather_kernel, dim3((unsigned)g.segs), dim3(PNG_THREADS), 0, to_stream(stream), slots, seg_info, dst, g, out);
  return check_launch("png_gather");
}
