// inflate_core.h -- the zlib inflate of ONE stream (include/aivc_hip_png_read.h: aivc_inflate), in text that hipcc compiles for the
// device and any C++ compiler for the host: plain C++, `__host__ __device__` only under hipcc.  png_read.hip runs it with one
// wavefront per stream and the State in LDS; tools/inflate_host.cpp runs the same text with one lane under the host sanitizers.
//
// The lanes of a stream run ONE control flow: everything that steers it (the bit buffer, positions, decoded symbols) is the same
// value in every lane, made so by Env::uniform where it comes out of the State, so a compiler for the device can keep it on the
// scalar side.  The lanes differ only where they share out bytes or symbols among themselves: the source window, the code
// tables, match copies, the flush.  What an Env supplies:
//     lane(), lanes()          this lane, how many there are (host: 0 of 1)
//     sync()                   every lane's writes to the State are visible to every lane behind it (host: nothing)
//     uniform(v)               v of the first lane (host: v)
//     ballot(p)                bit k = p of lane k (host: p)
//     sum(v)                   v summed over the lanes, uint64 (host: v)
//
// BOUNDS BY CONSTRUCTION.  The source is read in ONE place (load_window: `p < n ? src[p] : 0`), the destination written in ONE
// (flush: index < out <= expect).  Every index into the State is masked to its array's size or bounded by a count that was
// validated before use (build_code refuses an over-subscribed set, so the canonical walk of decode() stays inside sym[]).  No
// value of the stream is trusted: running past the source feeds zeros and is noticed at the next token (overrun).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define AIVC_INFLATE_FN __host__ __device__ inline
#define AIVC_INFLATE_UNROLL _Pragma("unroll")
// the table build and the source window stay out of line on the device: inlined, their registers crowd the symbol loop, and the
// compiler spills scalar registers inside it (experiments/png_read.md)
#define AIVC_INFLATE_COLD __host__ __device__ __attribute__((noinline))
#else
#define AIVC_INFLATE_UNROLL
#define AIVC_INFLATE_COLD inline
#define AIVC_INFLATE_FN inline
#endif

namespace inflate_core {

// the statuses of include/aivc_hip_png_read.h (AIVC_INFLATE_*)
enum : uint32_t {
  ST_OK = 0, ST_SRC_EXHAUSTED = 1, ST_BAD_HEADER = 2, ST_BAD_BLOCK_TYPE = 3, ST_STORED_MISMATCH = 4, ST_BAD_LENGTHS = 5,
  ST_BAD_SYMBOL = 6, ST_BAD_DISTANCE = 7, ST_TOO_LONG = 8, ST_TOO_SHORT = 9, ST_BAD_ADLER = 10, ST_TOO_LARGE = 11
};

constexpr uint32_t RING = 32768, RING_MASK = RING - 1;  // the window of deflate: the last 32 KiB of the output
constexpr uint32_t WIN = 4096;                          // bytes of the source held at a time
constexpr uint32_t FLUSH = 8192;                        // the ring's new bytes go to dst once there are this many (+ one match)
constexpr uint32_t LIT_BITS = 10, DIST_BITS = 8, CL_BITS = 7;  // primary lookup tables: longer codes take the canonical walk
constexpr uint32_t ADLER_MOD = 65521;
constexpr uint32_t INVALID = 0xffffu;
static_assert(FLUSH + 258 < RING, "bytes not yet flushed are never overwritten");

struct Code {
  uint16_t count[16];  // codes per length
  uint16_t sym[288];   // the symbols in canonical order
};

struct State {
  uint8_t ring[RING];
  uint32_t win[WIN / 4];
  uint16_t lit_tab[1u << LIT_BITS];   // (symbol << 4) | length; 0: not a code of at most LIT_BITS bits
  uint16_t dist_tab[1u << DIST_BITS];  // ... also the table of the code-length code
  uint8_t lens[320];                   // HLIT + HDIST <= 316 code lengths
  uint8_t cl_lens[32];
  Code lit, dist;
};

struct Bits {
  uint64_t hold;
  uint32_t cnt;    // valid bits in hold
  uint32_t pos;    // the next source byte to load, a multiple of 4 (may run past n: zeros)
  uint32_t wbase;  // the source position of win[0]; ~0: nothing loaded
};

template <class Env>
AIVC_INFLATE_COLD void load_window(State &S, const uint8_t *src, uint32_t n, uint32_t base) {
  Env::sync();
  for (uint32_t w = Env::lane(); w < WIN / 4; w += Env::lanes()) {
    uint32_t v = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      const uint32_t p = base + 4 * w + k;
      const uint32_t b = p < n ? src[p] : 0u;  // THE source read
      v |= b << (8 * k);
    }
    S.win[w] = v;
  }
  Env::sync();
}

template <class Env>
AIVC_INFLATE_FN void need_window(State &S, Bits &B, const uint8_t *src, uint32_t n, uint32_t pos) {
  const uint32_t base = pos & ~(WIN - 1);
  if (base != B.wbase) {
    load_window<Env>(S, src, n, base);
    B.wbase = base;
  }
}

// at least 33 bits in hold afterwards
template <class Env>
AIVC_INFLATE_FN void refill(State &S, Bits &B, const uint8_t *src, uint32_t n) {
  if (B.cnt <= 32) {
    need_window<Env>(S, B, src, n, B.pos);
    const uint32_t w = Env::uniform(S.win[(B.pos & (WIN - 1)) >> 2]);
    B.hold |= (uint64_t)w << B.cnt;
    B.pos += 4;
    B.cnt += 32;
  }
}

AIVC_INFLATE_FN uint32_t take(Bits &B, uint32_t k) {  // k <= 32 <= B.cnt
  const uint32_t v = (uint32_t)(B.hold & ((1ull << k) - 1ull));
  B.hold >>= k;
  B.cnt -= k;
  return v;
}

AIVC_INFLATE_FN bool overrun(const Bits &B, uint32_t n) { return B.pos > n && (uint64_t)B.pos * 8u - B.cnt > (uint64_t)n * 8u; }
AIVC_INFLATE_FN uint32_t byte_pos(const Bits &B) { return B.pos - (B.cnt >> 3); }  // of the next whole byte

AIVC_INFLATE_FN uint32_t reverse16(uint32_t v) {
  v = ((v & 0x5555u) << 1) | ((v >> 1) & 0x5555u);
  v = ((v & 0x3333u) << 2) | ((v >> 2) & 0x3333u);
  v = ((v & 0x0f0fu) << 4) | ((v >> 4) & 0x0f0fu);
  return ((v & 0x00ffu) << 8) | ((v >> 8) & 0x00ffu);
}

AIVC_INFLATE_FN uint32_t popcount64(uint64_t v) {
  v = v - ((v >> 1) & 0x5555555555555555ull);
  v = (v & 0x3333333333333333ull) + ((v >> 2) & 0x3333333333333333ull);
  v = (v + (v >> 4)) & 0x0f0f0f0f0f0f0f0full;
  return (uint32_t)((v * 0x0101010101010101ull) >> 56);
}

// lens[0 .. nsym) -> C and the primary table tab[1 << bits].  false: an over-subscribed set, or an incomplete one that zlib
// refuses (it takes a set with no code at all, and -- but for the code-length code -- one whose only code has one bit).
template <class Env>
AIVC_INFLATE_COLD bool build_code(State &S, const uint8_t *lens, uint32_t nsym, Code &C, uint16_t *tab, uint32_t bits, bool is_cl) {
  Env::sync();  // lens[] is complete, the table no longer read
  for (uint32_t k = Env::lane(); k < (1u << bits); k += Env::lanes()) tab[k] = 0;
  const uint32_t rounds = (nsym + Env::lanes() - 1) / Env::lanes();
  const uint64_t below = (1ull << Env::lane()) - 1ull;  // the lanes in front of this one
  uint32_t cnt[16];
  AIVC_INFLATE_UNROLL
  for (uint32_t l = 0; l < 16; ++l) cnt[l] = 0;
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t s = r * Env::lanes() + Env::lane();
    const uint32_t mine = s < nsym ? lens[s] : 0u;
    AIVC_INFLATE_UNROLL
    for (uint32_t l = 1; l < 16; ++l) cnt[l] += popcount64(Env::ballot(mine == l));
  }
  int32_t left = 1;
  uint32_t maxlen = 0;
  AIVC_INFLATE_UNROLL
  for (uint32_t l = 1; l < 16; ++l) {
    left = (left << 1) - (int32_t)cnt[l];
    if (left < 0) return false;
    if (cnt[l]) maxlen = l;
  }
  if (left > 0 && maxlen != 0 && (is_cl || maxlen != 1)) return false;
  uint32_t offs[16], code[16];  // where the next symbol of a length goes in C.sym, and its canonical code
  offs[0] = offs[1] = 0, code[0] = code[1] = 0;
  AIVC_INFLATE_UNROLL
  for (uint32_t l = 2; l < 16; ++l) offs[l] = offs[l - 1] + cnt[l - 1], code[l] = (code[l - 1] + cnt[l - 1]) << 1;
  if (Env::lane() == 0) {
    C.count[0] = 0;
    AIVC_INFLATE_UNROLL
    for (uint32_t l = 1; l < 16; ++l) C.count[l] = (uint16_t)cnt[l];
  }
  Env::sync();  // the table is zero
  for (uint32_t r = 0; r < rounds; ++r) {
    const uint32_t s = r * Env::lanes() + Env::lane();
    const uint32_t mine = s < nsym ? lens[s] : 0u;
    AIVC_INFLATE_UNROLL
    for (uint32_t l = 1; l < 16; ++l) {
      const uint64_t mask = Env::ballot(mine == l);
      if (mine == l) {
        const uint32_t rank = popcount64(mask & below);
        C.sym[(offs[l] + rank) % 288u] = (uint16_t)s;
        if (l <= bits) {
          const uint32_t rev = reverse16(code[l] + rank) >> (16 - l);
          for (uint32_t k = rev; k < (1u << bits); k += 1u << l) tab[k] = (uint16_t)((s << 4) | l);
        }
      }
      const uint32_t got = popcount64(mask);
      offs[l] += got, code[l] += got;
    }
  }
  Env::sync();
  return true;
}

// one symbol: the primary table, or -- a longer code, or none -- the canonical walk.  INVALID: no code of the set starts here.
template <class Env>
AIVC_INFLATE_FN uint32_t decode(Bits &B, const uint16_t *tab, uint32_t bits, const Code &C) {
  const uint32_t e = Env::uniform((uint32_t)tab[(uint32_t)B.hold & ((1u << bits) - 1u)]);
  if (e & 15u) {
    B.hold >>= (e & 15u);
    B.cnt -= (e & 15u);
    return e >> 4;
  }
  uint32_t code = 0, first = 0, index = 0;
  uint64_t h = B.hold;
  for (uint32_t l = 1; l < 16; ++l) {
    code |= (uint32_t)h & 1u;
    h >>= 1;
    const uint32_t count = Env::uniform((uint32_t)C.count[l]);
    if (code < first + count) {  // (code >= first always)
      B.hold >>= l;
      B.cnt -= l;
      return Env::uniform((uint32_t)C.sym[(index + (code - first)) % 288u]);
    }
    index += count;
    first = (first + count) << 1;
    code <<= 1;
  }
  return INVALID;
}

// the ring's bytes [flushed, out) -> dst, and into the Adler sums a, b
template <class Env>
AIVC_INFLATE_FN void flush(State &S, uint8_t *dst, uint32_t &flushed, uint32_t out, uint32_t &a, uint32_t &b) {
  Env::sync();
  const uint32_t n = out - flushed;  // <= FLUSH + 258 + WIN
  uint32_t s1 = 0;
  uint64_t s2 = 0;
  for (uint32_t i = Env::lane(); i < n; i += Env::lanes()) {
    const uint32_t v = S.ring[(flushed + i) & RING_MASK];
    dst[flushed + i] = (uint8_t)v;  // THE destination write: flushed + i < out <= expect
    s1 += v;
    s2 += (uint64_t)(n - i) * v;
  }
  const uint64_t t1 = Env::sum(s1), t2 = Env::sum(s2);
  b = (uint32_t)((b + (uint64_t)n * a + t2) % ADLER_MOD);
  a = (uint32_t)((a + t1) % ADLER_MOD);
  flushed = out;
  Env::sync();
}

// One zlib stream src[0 .. n) -> dst[0 .. expect): the status; produced: bytes written to dst; consumed: source bytes up to and
// with the Adler-32 (meaningful where the status is ST_OK).  n, expect < 2^31.
template <class Env>
AIVC_INFLATE_FN uint32_t inflate_stream(State &S, const uint8_t *src, uint32_t n, uint8_t *dst, uint32_t expect, uint32_t &produced,
                                        uint32_t &consumed) {
  Bits B;
  B.hold = 0, B.cnt = 0, B.pos = 0, B.wbase = ~0u;
  uint32_t out = 0, flushed = 0, a = 1, b = 0, status = ST_OK;
  produced = 0, consumed = 0;

  refill<Env>(S, B, src, n);
  const uint32_t cmf = take(B, 8), flg = take(B, 8);
  if (overrun(B, n)) return ST_SRC_EXHAUSTED;
  if ((cmf & 15u) != 8u || (cmf >> 4) > 7u || ((cmf << 8) | flg) % 31u != 0u || (flg & 32u)) return ST_BAD_HEADER;

  for (bool final = false; !final && status == ST_OK;) {
    refill<Env>(S, B, src, n);
    final = take(B, 1) != 0;
    const uint32_t type = take(B, 2);
    if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
    if (type == 3) { status = ST_BAD_BLOCK_TYPE; break; }
    if (type == 0) {  // stored
      take(B, B.cnt & 7u);
      refill<Env>(S, B, src, n);  // (cnt is a multiple of 8: at least 32 bits now)
      const uint32_t len = take(B, 16), nlen = take(B, 16);
      if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
      if ((len ^ nlen) != 0xffffu) { status = ST_STORED_MISMATCH; break; }
      uint32_t q = byte_pos(B);  // <= n
      if (len > n - q) { status = ST_SRC_EXHAUSTED; break; }
      if (len > expect - out) { status = ST_TOO_LONG; break; }
      for (uint32_t left = len; left;) {
        need_window<Env>(S, B, src, n, q);
        const uint32_t at = q & (WIN - 1);
        const uint32_t c = left < WIN - at ? left : WIN - at;
        const uint8_t *wb = reinterpret_cast<const uint8_t *>(S.win);
        for (uint32_t i = Env::lane(); i < c; i += Env::lanes()) S.ring[(out + i) & RING_MASK] = wb[(at + i) & (WIN - 1)];
        out += c, q += c, left -= c;
        if (out - flushed >= FLUSH) flush<Env>(S, dst, flushed, out, a, b);
      }
      B.hold = 0, B.cnt = 0, B.pos = q & ~3u;  // the reader goes on at byte q
      refill<Env>(S, B, src, n);
      take(B, 8u * (q & 3u));
      continue;
    }
    uint32_t nlit, ndist;
    if (type == 1) {  // the fixed codes: 288 and 32 symbols, of which 286, 287 and 30, 31 are never valid
      for (uint32_t s = Env::lane(); s < 320; s += Env::lanes()) S.lens[s] = (uint8_t)(s < 144 ? 8 : s < 256 ? 9 : s < 280 ? 7 : s < 288 ? 8 : 5);
      nlit = 288, ndist = 32;
    } else {
      refill<Env>(S, B, src, n);
      nlit = take(B, 5) + 257, ndist = take(B, 5) + 1;
      const uint32_t ncl = take(B, 4) + 4;
      if (nlit > 286 || ndist > 30) { status = overrun(B, n) ? ST_SRC_EXHAUSTED : ST_BAD_LENGTHS; break; }
      Env::sync();
      const uint8_t order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};
      for (uint32_t k = 0; k < 19; ++k) {
        uint32_t v = 0;
        if (k < ncl) {
          refill<Env>(S, B, src, n);
          v = take(B, 3);
        }
        if (Env::lane() == 0) S.cl_lens[order[k]] = (uint8_t)v;
      }
      if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
      if (!Env::uniform(build_code<Env>(S, S.cl_lens, 19, S.dist, S.dist_tab, CL_BITS, true))) { status = ST_BAD_LENGTHS; break; }
      const uint32_t total = nlit + ndist;
      for (uint32_t i = 0; i < total && status == ST_OK;) {
        refill<Env>(S, B, src, n);
        const uint32_t sym = decode<Env>(B, S.dist_tab, CL_BITS, S.dist);
        if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
        if (sym > 18) { status = ST_BAD_LENGTHS; break; }
        if (sym < 16) {
          if (Env::lane() == 0) S.lens[i % 320u] = (uint8_t)sym;
          ++i;
          continue;
        }
        uint32_t prev = 0, rep;
        if (sym == 16) {
          if (i == 0) { status = ST_BAD_LENGTHS; break; }
          Env::sync();
          prev = Env::uniform((uint32_t)S.lens[(i - 1) % 320u]);
          rep = 3 + take(B, 2);
        } else if (sym == 17) {
          rep = 3 + take(B, 3);
        } else {
          rep = 11 + take(B, 7);
        }
        if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
        if (rep > total - i) { status = ST_BAD_LENGTHS; break; }
        Env::sync();
        for (uint32_t k = Env::lane(); k < rep; k += Env::lanes()) S.lens[(i + k) % 320u] = (uint8_t)prev;
        i += rep;
      }
      if (status != ST_OK) break;
      Env::sync();
      if (Env::uniform((uint32_t)S.lens[256]) == 0) { status = ST_BAD_LENGTHS; break; }  // no end-of-block code
    }
    if (!Env::uniform(build_code<Env>(S, S.lens, nlit, S.lit, S.lit_tab, LIT_BITS, false)) ||
        !Env::uniform(build_code<Env>(S, S.lens + nlit, ndist, S.dist, S.dist_tab, DIST_BITS, false))) { status = ST_BAD_LENGTHS; break; }

    for (;;) {  // the tokens of the block
      refill<Env>(S, B, src, n);
      const uint32_t sym = decode<Env>(B, S.lit_tab, LIT_BITS, S.lit);
      if (sym < 256) {
        if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
        if (out >= expect) { status = ST_TOO_LONG; break; }
        if (Env::lane() == 0) S.ring[out & RING_MASK] = (uint8_t)sym;
        ++out;
      } else if (sym == 256) {
        if (overrun(B, n)) status = ST_SRC_EXHAUSTED;
        break;
      } else {
        if (sym >= 286) { status = overrun(B, n) ? ST_SRC_EXHAUSTED : ST_BAD_SYMBOL; break; }
        const uint32_t k = sym - 257;
        const uint32_t leb = k < 8 || k == 28 ? 0u : (k >> 2) - 1u;
        const uint32_t len = k == 28 ? 258u : k < 8 ? 3u + k : 3u + ((4u + (k & 3u)) << leb) + take(B, leb);
        refill<Env>(S, B, src, n);
        const uint32_t d = decode<Env>(B, S.dist_tab, DIST_BITS, S.dist);
        if (d >= 30) { status = overrun(B, n) ? ST_SRC_EXHAUSTED : ST_BAD_SYMBOL; break; }
        const uint32_t deb = d < 4 ? 0u : (d >> 1) - 1u;
        const uint32_t dist = d < 4 ? 1u + d : 1u + ((2u + (d & 1u)) << deb) + take(B, deb);
        if (overrun(B, n)) { status = ST_SRC_EXHAUSTED; break; }
        if (dist > out) { status = ST_BAD_DISTANCE; break; }
        if (len > expect - out) { status = ST_TOO_LONG; break; }
        // byte i of the match is byte i mod dist of the dist bytes in front of it: every read lies in front of `out`.  Two lanes
        // meet in one byte of the ring only where dist + i - j = RING, i the writer: it comes behind the reader j in lane order.
        const uint32_t from = out - dist;
        for (uint32_t i0 = 0; i0 < len; i0 += Env::lanes()) {
          const uint32_t i = i0 + Env::lane();
          if (i < len) {
            const uint32_t j = dist >= len ? i : i % dist;
            const uint32_t v = S.ring[(from + j) & RING_MASK];
            S.ring[(out + i) & RING_MASK] = (uint8_t)v;
          }
        }
        out += len;
      }
      if (out - flushed >= FLUSH) flush<Env>(S, dst, flushed, out, a, b);
    }
  }
  flush<Env>(S, dst, flushed, out, a, b);  // (a failed stream's bytes so far: inside its own range all the same)
  produced = out;
  if (status != ST_OK) return status;
  if (out != expect) return ST_TOO_SHORT;
  take(B, B.cnt & 7u);
  refill<Env>(S, B, src, n);
  uint32_t sum = 0;
  for (int k = 0; k < 4; ++k) sum = (sum << 8) | take(B, 8);  // (big-endian)
  if (overrun(B, n)) return ST_SRC_EXHAUSTED;
  if (sum != ((b << 16) | a)) return ST_BAD_ADLER;
  consumed = byte_pos(B);
  return ST_OK;
}

}  // namespace inflate_core
