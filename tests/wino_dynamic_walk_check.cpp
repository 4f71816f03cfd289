// Stand-alone check of aivc_amd/csrc/wino_dynamic_walk.h (tests/test_winograd_dynamic_walk.py compiles and runs it; no GPU, no
// HIP).  The persistent workgroups of conv_wino.hip claim the entries of their XCD's range from a ticket counter at run time.
// What a workgroup does with the counters is restated here as the kernel does it -- one claim before its first block, one
// more inside every block it computes (the next block: it never holds more than one it has not started), one count on the way
// out behind the claim that found nothing, the last one out zeroes the set -- and run as a simulation in which every
// fetch-and-add is one step and a seeded generator picks whose step comes next:
//   * all workgroups resident from the start, steps interleaved at random;
//   * a bound on the workgroups that run at the same time (1, half the grid, all but one): the others start when one has left,
//     in random order -- workgroups that start after others have finished, down to one at a time;
//   * the same with a random third of the grid held back until every other workgroup has left.
// Lists: total 1 .. 3000 and the 1080p lists (17 x 30 pixel blocks x 16 / 64 images x gy, x 4 classes in the transposed form),
// gy 1 / 2 / 3, 256 / 304 / 64 / total workgroups (capped at the list length, as the launch caps them).  The claims do not
// depend on the form; what an entry means does: MODE 0 / 1 read it plainly (pixel block entry / gy, channel block entry % gy),
// MODE 2 through wino_class_walk.h with 4 gy entries per pixel block.  Checked per run: every entry claimed exactly once and
// none outside [0, total); in each reading every (pixel block, cb) computed exactly once; every workgroup terminates (the
// simulation ends); after the last exit all nine counters are zero, and they were cleaned exactly once.
// Prints the first violation and exits 1; prints a summary line and exits 0.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "../aivc_amd/csrc/wino_class_walk.h"
#include "../aivc_amd/csrc/wino_dynamic_walk.h"

namespace {

using namespace aivc;

struct Workgroup {
  uint32_t xcd = 0, claims = 0, cur = WINO_WALK_END;
  bool out = false;
};

struct Sim {
  uint32_t total, nwg;
  uint32_t slots[WINO_WALK_SLOTS] = {};
  uint32_t cleaned = 0;
  std::vector<uint8_t> claimed;  // per entry: how often a workgroup computed it
  bool stray = false;            // an entry outside [0, total)
  std::vector<Workgroup> wg;

  Sim(uint32_t total_, uint32_t nwg_) : total(total_), nwg(nwg_), claimed(total_, 0), wg(nwg_) {
    for (uint32_t b = 0; b < nwg; ++b) wg[b].xcd = b & (WINO_WALK_XCDS - 1u);
  }
  uint32_t claim(const Workgroup &w) { return wino_ticket_entry(wino_xcd_range(total, w.xcd), slots[w.xcd]++); }
  void compute(uint32_t e) {
    if (e < total) ++claimed[e];
    else stray = true;
  }
  // one step of workgroup b: everything up to and including its next fetch-and-add.  -> false: it has left
  bool step(uint32_t b) {
    Workgroup &w = wg[b];
    if (w.claims == 0) {
      w.cur = claim(w);
    } else {  // a block: the claim of the next one rides in its first chunk
      const uint32_t ahead = claim(w);
      compute(w.cur);
      w.cur = ahead;
    }
    ++w.claims;
    if (w.cur == WINO_WALK_END) {  // out: count, and clean as the last one
      if (wino_last_out(slots[WINO_WALK_EXIT]++, nwg)) {
        for (uint32_t i = 0; i <= WINO_WALK_EXIT; ++i) slots[i] = 0;
        ++cleaned;
      }
      w.out = true;
      return false;
    }
    return true;
  }
};

// resident: workgroups that may run at the same time; held: that many workgroups start only after all the others have left
bool run(uint32_t total, uint32_t nwg, uint32_t resident, uint32_t held, uint32_t seed) {
  Sim s(total, nwg);
  std::mt19937 rng(seed);
  std::vector<uint32_t> waiting(nwg), running, late;
  for (uint32_t b = 0; b < nwg; ++b) waiting[b] = b;
  std::shuffle(waiting.begin(), waiting.end(), rng);
  late.assign(waiting.begin(), waiting.begin() + held);
  waiting.erase(waiting.begin(), waiting.begin() + held);
  uint64_t steps = 0;
  const uint64_t limit = 2ull * total + 4ull * nwg + 16;  // (every step but a workgroup's first one computes a block)
  for (;;) {
    while (running.size() < resident && !waiting.empty()) {
      running.push_back(waiting.back());
      waiting.pop_back();
    }
    if (running.empty()) {
      if (late.empty()) break;
      waiting.swap(late);
      continue;
    }
    const size_t i = rng() % running.size();
    if (!s.step(running[i])) {
      running[i] = running.back();
      running.pop_back();
    }
    if (++steps > limit) {
      printf("total %u nwg %u resident %u held %u seed %u: a workgroup does not terminate\n", total, nwg, resident, held, seed);
      return false;
    }
  }
  const char *what = nullptr;
  if (s.stray) what = "an entry outside the list was computed";
  for (uint32_t e = 0; e < total && !what; ++e)
    if (s.claimed[e] != 1) what = s.claimed[e] ? "an entry was computed twice" : "an entry was never computed";
  for (uint32_t i = 0; i < WINO_WALK_SLOTS && !what; ++i)
    if (s.slots[i]) what = "a counter is not zero after the last exit";
  if (!what && s.cleaned != 1) what = "the counters were not cleaned exactly once";
  for (const Workgroup &w : s.wg)
    if (!what && !w.out) what = "a workgroup never left";
  if (what) printf("total %u nwg %u resident %u held %u seed %u: %s\n", total, nwg, resident, held, seed, what);
  return !what;
}

// the readings of a list whose entries are each claimed once: every (pixel block, cb) exactly once.  mode 0 / 1: plain, mode 2:
// wino_class_entry with 4 gy entries per pixel block
bool readings(uint32_t total, uint32_t gy, uint32_t nwg) {
  static std::vector<uint8_t> seen;
  for (int mode = 0; mode < 3; ++mode) {
    const uint32_t gyc = mode == 2 ? 4u * gy : gy;
    seen.assign((size_t)(total + gyc - 1u) / gyc * gyc, 0);  // (a real list is whole pixel blocks)
    for (uint32_t e = 0; e < total; ++e) {
      WinoClassEntry d = {e / gyc, e % gyc};
      if (mode == 2) d = wino_class_entry(e, gyc, total, nwg);
      if (d.pb != e / gyc || d.cb >= gyc || seen[(size_t)d.pb * gyc + d.cb]++) {
        printf("mode %d total %u gy %u nwg %u: entry %u -> pixel block %u, cb %u (out of range or computed twice)\n", mode, total, gy, nwg, e, d.pb, d.cb);
        return false;
      }
    }
  }
  return true;
}

bool list(uint32_t total, uint32_t nwg_asked, uint32_t seed, unsigned &runs) {
  const uint32_t nwg = std::min(nwg_asked, total);
  const uint32_t bounds[] = {nwg, 1u, std::max(1u, nwg / 2u), std::max(1u, nwg - 1u)};
  // all resident; then one bound of the three per list in turn, without and with a third of the grid held back
  if (!run(total, nwg, nwg, 0u, seed)) return false;
  const uint32_t r = bounds[1u + seed % 3u];
  if (!run(total, nwg, r, 0u, seed + 1u)) return false;
  if (!run(total, nwg, r, nwg / 3u, seed + 2u)) return false;
  if (!run(total, nwg, nwg, nwg / 3u, seed + 3u)) return false;
  runs += 4;
  for (uint32_t gy = 1; gy <= 3; ++gy)
    if (!readings(total, gy, nwg)) return false;
  return true;
}

}  // namespace

int main() {
  const uint32_t grids[] = {256u, 304u, 64u, 0u};  // 0: one workgroup per entry
  unsigned lists = 0, runs = 0;
  uint32_t seed = 20240u;
  for (uint32_t total = 1; total <= 3000; ++total)
    for (uint32_t g : grids) {
      if (!list(total, g ? g : total, seed += 7u, runs)) return 1;
      ++lists;
    }
  for (uint32_t images : {16u, 64u})
    for (uint32_t gy = 1; gy <= 3; ++gy)
      for (uint32_t classes : {1u, 4u})
        for (uint32_t g : {256u, 304u, 64u}) {  // (one workgroup per entry of these lists: the launch never does that)
          if (!list(images * 17u * 30u * gy * classes, g, seed += 7u, runs)) return 1;
          ++lists;
        }
  printf("ok: %u lists, %u interleavings: every entry claimed once, counters zero after the last exit\n", lists, runs);
  return 0;
}
