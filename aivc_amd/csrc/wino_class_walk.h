// wino_class_walk.h -- how the transposed Winograd form (conv_wino.hip, MODE 2) reads an entry of its block list.  No HIP
// dependency: the kernel includes it, and tests/wino_class_walk_check.cpp compiles it with the host compiler alone.
//
// The list has gyc = 4 classes x (c_out / 64) channel blocks entries per pixel block, neighbours in the list.  A persistent
// workgroup walks the entries B0 + k W of its XCD's eighth of the list (WinoWalk; W: the workgroups of the XCD).  Read plainly,
// entry % gyc takes only the gyc / gcd(W, gyc) values of one coset along that walk: with W = 32 and gyc = 4 or 8 a single one,
// so a workgroup keeps its class for the whole launch.  The classes issue 16 / 12 / 12 / 9 positions per chunk: the class-0
// workgroups set the launch's length and the others wait for them.
// Hence the entries of pixel block pb are dealt to its gyc (class, channel block) pairs rotated by rot(pb) = pb / q with
// q = W / gcd(W, gyc).  rot is a function of the pixel block alone: a bijection inside every pixel block, whatever the list
// length, the grid and the XCD ranges are.  P = gyc / gcd(W, gyc) blocks of a workgroup are exactly q pixel blocks apart, so rot
// holds each value for P consecutive blocks of every workgroup, in which entry % gyc runs once through its coset, and the next
// value moves on to the next coset: gcd(W, gyc) values of rot in a row give a workgroup the gyc different cb values, once each.
// Over a whole walk its counts of the cb values therefore differ by two at the most (a started group at either end), and by one
// where W is a multiple of gyc (P = 1: cb simply advances by one per block; the 1080p launches, W = 32 and gyc = 4).  The
// entries of a pixel block stay neighbours in the list, walked at the same time by neighbouring workgroups of one XCD, which
// share its raw patch in that L2.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AIVC_WINO_HD __host__ __device__
#else
#define AIVC_WINO_HD
#endif

namespace aivc {

struct WinoClassEntry {
  uint32_t pb;  // pixel block: (image * nby + byi) * nbx + bxi
  uint32_t cb;  // class * gy + channel block
};

// total, nwg: the entries of the list and the workgroups of the launch.  W is that of the XCD whose range holds the pixel
// block's FIRST entry (the XCDs' counts differ where nwg % 8 != 0), so a pixel block that straddles two ranges is rotated alike
// in both.
AIVC_WINO_HD inline WinoClassEntry wino_class_entry(uint32_t entry, uint32_t gyc, uint32_t total, uint32_t nwg) {
  const uint32_t pb = entry / gyc, j = entry - pb * gyc;
  const uint32_t xcd = (pb * gyc) / ((total + 7u) >> 3), w = (nwg + 7u - xcd) >> 3;
  uint32_t q = 1u;
  if (w) {
    uint32_t a = w, b = gyc;  // gcd(w, gyc)
    while (b) {
      const uint32_t t = a % b;
      a = b;
      b = t;
    }
    q = w / a;
  }
  return {pb, (j + pb / q) % gyc};
}

}  // namespace aivc
