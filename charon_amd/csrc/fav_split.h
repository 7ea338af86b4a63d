// The slice plan of the keyed FastAggregateVerify's split key sum (hipbls.hip fav_keys_host, kernels.h k_fav_sum_keys):
// a group with more than `slice` keys is cut into consecutive slices of `slice` keys, the last one shorter, each of
// which one workgroup folds to a partial sum; the check kernel then adds the group's partials instead of walking its
// keys.  A group of at most `slice` keys is left whole.  Standard C++ only (no HIP), so the plan is built and tested on
// the host (tests/native/fav_split_main.cpp).
#pragma once
#include <cstdint>
#include <vector>

struct FavSplitPlan {
  std::vector<uint64_t> slices;  // two words per slice: its keys [slices[2 s], slices[2 s + 1]) of the call's key list
  std::vector<uint64_t> poff;    // n_groups + 1: group g owns the slices [poff[g], poff[g + 1]), none when left whole
  uint64_t n_slices() const { return slices.size() / 2; }
};

// Fills `plan` from the call's key offsets (key_offsets[0] == 0, non-decreasing); slice == 0 turns the split off.
// Returns whether any group was cut.  The slices of a cut group tile it exactly, in order, and none is empty.
inline bool fav_split_plan(const uint64_t* key_offsets, uint64_t n_groups, uint64_t slice, FavSplitPlan& plan) {
  plan.slices.clear();
  plan.poff.assign(n_groups + 1, 0);
  for (uint64_t g = 0; g < n_groups; ++g) {
    const uint64_t k0 = key_offsets[g], k1 = key_offsets[g + 1];
    if (slice != 0 && k1 - k0 > slice)
      for (uint64_t lo = k0; lo < k1; lo += slice) {
        plan.slices.push_back(lo);
        plan.slices.push_back(k1 - lo > slice ? lo + slice : k1);
      }
    plan.poff[g + 1] = plan.n_slices();
  }
  return !plan.slices.empty();
}
