// wino_dynamic_walk.h -- which entries of the block list a persistent Winograd workgroup takes (conv_wino.hip): the arithmetic of
// the walk.  No HIP dependency: the kernel includes it, and tests/wino_dynamic_walk_check.cpp compiles it with the host compiler.
//
// The dispatcher deals consecutive workgroup ids round-robin to the 8 XCDs (each with a private L2): workgroup b sits on XCD
// b & 7 and walks that XCD's contiguous eighth [lo, hi) of the list.  It does not own a fixed share of it: its next entry is
// lo + (the XCD's ticket counter, fetched and incremented), for as long as that is below hi.  The workgroups of an XCD therefore
// still advance through one region together, in list order (the channel blocks and classes of a pixel block are neighbours in
// the list and share its raw patch in that L2), and a workgroup that starts late -- its CU was held by another kernel's LDS --
// takes what is left, or nothing.  With a fixed share the others finished and the launch then waited for that one workgroup to
// run its whole share.  Nothing crosses XCDs: a late workgroup costs its XCD about one part in its workgroup count.
// A workgroup claims its next entry while it computes the current one and holds no more than that one ahead, so a launch ends
// on at most one block of imbalance, as it did with fixed shares.
//
// The counters of a launch are one slot set: 8 tickets and an exit count, all zero between launches.  Every workgroup counts
// itself out once, after its last claim; the one that finds all the others out zeroes the set.  Launches that may run at the
// same time use different sets (conv_wino.hip: one per stream).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AIVC_WINO_WALK_HD __host__ __device__
#else
#define AIVC_WINO_WALK_HD
#endif

namespace aivc {

constexpr uint32_t WINO_WALK_XCDS = 8u;
constexpr uint32_t WINO_WALK_EXIT = 8u;    // index of the exit count in a slot set
constexpr uint32_t WINO_WALK_SLOTS = 16u;  // uint32 per slot set (64 bytes)
constexpr uint32_t WINO_WALK_END = 0xFFFFFFFFu;  // "no entry": the XCD's range is used up (a list has fewer than 2^31 entries)

struct WinoXcdRange {
  uint32_t lo, hi;  // [lo, hi): empty where the list has fewer than 8 entries per XCD before this one
};

AIVC_WINO_WALK_HD inline WinoXcdRange wino_xcd_range(uint32_t total, uint32_t xcd) {
  const uint32_t per_xcd = (total + 7u) >> 3, lo = xcd * per_xcd;  // (total < 2^31: no overflow)
  const uint32_t hi = lo + per_xcd < total ? lo + per_xcd : total;
  return {lo, hi > lo ? hi : lo};
}

// the entry a ticket stands for: tickets count up from 0 per XCD and launch; those past the range end the walk
AIVC_WINO_WALK_HD inline uint32_t wino_ticket_entry(WinoXcdRange r, uint32_t ticket) {
  return ticket < r.hi - r.lo ? r.lo + ticket : WINO_WALK_END;
}

// exits_before: what the exit count held when this workgroup counted itself out -> it is the last one of nwg and cleans the set
AIVC_WINO_WALK_HD inline bool wino_last_out(uint32_t exits_before, uint32_t nwg) { return exits_before + 1u == nwg; }

}  // namespace aivc
