// Stand-alone check of aivc_amd/csrc/wino_class_walk.h (tests/test_winograd_class_walk.py compiles and runs it; no GPU, no HIP).
// The block walk of a persistent workgroup (WinoWalk in conv_wino.hip) is restated here, as tests/test_gpu_winograd_5x5_issue.py
// restates it in Python: which entries a workgroup takes is the walk's business, what an entry means is the header's.
//   a. every (pixel block, class * gy + channel block) of the list is computed exactly once, and a pixel block's entries are the
//      gyc neighbours pb * gyc .. pb * gyc + gyc - 1 of the list: total 1 .. 3000 and the flagship totals, gy 1 / 2 / 3,
//      256 / 304 / 64 / total workgroups (capped at the list length, as the launch caps them)
//   b. every workgroup with gyc blocks or more gets each cb value equally often: to within one on the flagship launches
//      (17 x 30 pixel blocks x n = 16 / 64 images, gy 1, 256 workgroups) and wherever the walk's stride is a multiple of gyc
//      (gy 2 on 256 workgroups, gy 1 / 2 on 64), to within two -- the header says why -- where it is not (gy 3: gyc 12 against
//      a stride of 32; 304 workgroups: a stride of 38), on the flagship lists, on one more pixel block (the XCD ranges then cut
//      through pixel blocks) and on a short list
// Prints the first violation and exits 1; prints a summary line and exits 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../aivc_amd/csrc/wino_class_walk.h"

namespace {

// f(entry) for the entries of workgroup wg of nwg, in the order it walks them -> how many
template <class F>
uint32_t owned(uint32_t total, uint32_t nwg, uint32_t wg, F f) {
  const uint32_t xcd = wg & 7u, slot = wg >> 3, per_xcd = (total + 7u) >> 3, wg_per_xcd = (nwg + 7u - xcd) >> 3;
  const uint64_t x_lo = (uint64_t)xcd * per_xcd, x_hi = std::min<uint64_t>(x_lo + per_xcd, total);
  uint32_t n = 0;
  for (uint64_t e = x_lo + slot; e < x_hi; e += wg_per_xcd, ++n) f((uint32_t)e);
  return n;
}

bool exactly_once(uint32_t total, uint32_t gy, uint32_t nwg_asked) {
  const uint32_t gyc = 4u * gy, nwg = std::min(nwg_asked, total);
  static std::vector<uint8_t> seen;
  seen.assign((size_t)(total + gyc - 1u) / gyc * gyc, 0);  // (a real list is whole pixel blocks: once each = all of them)
  uint32_t walked = 0, bad = 0;
  for (uint32_t wg = 0; wg < nwg; ++wg)
    walked += owned(total, nwg, wg, [&](uint32_t e) {
      const aivc::WinoClassEntry d = aivc::wino_class_entry(e, gyc, total, nwg);
      if (d.pb != e / gyc || d.cb >= gyc || seen[d.pb * gyc + d.cb]++) {
        if (!bad++)
          printf("a: total %u gy %u nwg %u: entry %u -> pixel block %u, cb %u (out of range, not the entry's pixel block, or computed twice)\n",
                 total, gy, nwg, e, d.pb, d.cb);
      }
    });
  if (!bad && walked != total) printf("a: total %u gy %u nwg %u: %u entries walked\n", total, gy, nwg, walked);
  return !bad && walked == total;
}

// -> the largest (max - min) of the cb counts of a workgroup with gyc blocks or more; -1: no such workgroup
int worst_spread(uint32_t total, uint32_t gy, uint32_t nwg_asked) {
  const uint32_t gyc = 4u * gy, nwg = std::min(nwg_asked, total);
  int worst = -1;
  for (uint32_t wg = 0; wg < nwg; ++wg) {
    std::vector<int> count(gyc, 0);
    const uint32_t mine = owned(total, nwg, wg, [&](uint32_t e) { ++count[aivc::wino_class_entry(e, gyc, total, nwg).cb]; });
    if (mine < gyc) continue;
    const int spread = *std::max_element(count.begin(), count.end()) - *std::min_element(count.begin(), count.end());
    worst = std::max(worst, spread);
  }
  return worst;
}

}  // namespace

int main() {
  const uint32_t grids[] = {256u, 304u, 64u, 0u};  // 0: one workgroup per entry
  const uint32_t flagship[] = {16u * 17u * 30u, 64u * 17u * 30u};  // pixel blocks
  unsigned lists = 0;
  for (uint32_t gy = 1; gy <= 3; ++gy) {
    for (uint32_t total = 1; total <= 3000; ++total)
      for (uint32_t g : grids) {
        if (!exactly_once(total, gy, g ? g : total)) return 1;
        ++lists;
      }
    for (uint32_t pbs : flagship)
      for (uint32_t g : grids) {
        if (!exactly_once(pbs * 4u * gy, gy, g ? g : pbs * 4u * gy)) return 1;
        ++lists;
      }
  }
  unsigned dealt = 0;
  for (uint32_t pbs : {flagship[0], flagship[1], flagship[0] + 1u, 1001u})
    for (uint32_t gy = 1; gy <= 3; ++gy)
      for (uint32_t g : {256u, 304u, 64u}) {
        const int bound = (g >> 3) % (4u * gy) == 0 ? 1 : 2, s = worst_spread(pbs * 4u * gy, gy, g);
        if (s < 0 || s > bound) {
          printf("b: %u pixel blocks, gy %u, %u workgroups: cb counts of a workgroup %d apart, bound %d\n", pbs, gy, g, s, bound);
          return 1;
        }
        ++dealt;
      }
  printf("ok: %u lists computed exactly once, %u dealt evenly\n", lists, dealt);
  return 0;
}
