// Host program for the keyed FastAggregateVerify's host-side planning (hipbls.hip fav_keys_host), built with
// -fsanitize=address,undefined and run directly (tests/test_fav_keys_static.py):
//   * fav_split.h fav_split_plan: which groups are cut into slices, and that the slices tile each cut group exactly,
//     in order, with none empty and none above the slice size;
//   * hcache_assign.h distinct_messages + hcache_read: the groups' messages folded to the distinct ones and looked up
//     read-only -- hits and misses per distinct message, no insert, no eviction, the bypass.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "fav_split.h"
#include "hcache_assign.h"

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: CHECK(%s)\n", __FILE__, __LINE__, #c); \
      exit(1);                                                    \
    }                                                             \
  } while (0)

static std::vector<uint64_t> offsets(const std::vector<uint64_t>& sizes) {
  std::vector<uint64_t> o(1, 0);
  for (uint64_t s : sizes) o.push_back(o.back() + s);
  return o;
}

// The plan's invariants for group sizes `sizes` at slice size `slice`; returns the number of slices.
static uint64_t check_plan(const std::vector<uint64_t>& sizes, uint64_t slice) {
  const std::vector<uint64_t> koff = offsets(sizes);
  const uint64_t G = sizes.size();
  FavSplitPlan plan;
  plan.slices.assign(7, 99);  // stale content must not survive
  plan.poff.assign(3, 99);
  const bool cut = fav_split_plan(koff.data(), G, slice, plan);
  CHECK(plan.poff.size() == G + 1);
  CHECK(plan.poff[0] == 0);
  CHECK(plan.slices.size() % 2 == 0);
  CHECK(plan.poff[G] == plan.n_slices());
  CHECK(cut == (plan.n_slices() != 0));
  bool any = false;
  for (uint64_t g = 0; g < G; ++g) {
    const uint64_t p0 = plan.poff[g], p1 = plan.poff[g + 1];
    CHECK(p1 >= p0);
    const bool want_cut = slice != 0 && sizes[g] > slice;
    any = any || want_cut;
    if (!want_cut) {
      CHECK(p1 == p0);
      continue;
    }
    CHECK(p1 - p0 == (sizes[g] + slice - 1) / slice);
    CHECK(p1 - p0 >= 2);
    uint64_t at = koff[g];
    for (uint64_t p = p0; p < p1; ++p) {
      const uint64_t lo = plan.slices[2 * p], hi = plan.slices[2 * p + 1];
      CHECK(lo == at);            // in order, no gap, no overlap
      CHECK(hi > lo);             // none empty
      CHECK(hi - lo <= slice);
      if (p + 1 < p1) CHECK(hi - lo == slice);
      at = hi;
    }
    CHECK(at == koff[g + 1]);  // the slices tile the group exactly
  }
  CHECK(cut == any);
  return plan.n_slices();
}

static void test_planner() {
  CHECK(check_plan({}, 64) == 0);                  // no groups, no keys at all
  CHECK(check_plan({0}, 64) == 0);                 // one empty group
  CHECK(check_plan({0, 0, 0}, 1) == 0);
  CHECK(check_plan({0, 1}, 64) == 0);              // groups of 0 and 1 keys
  CHECK(check_plan({1}, 1) == 0);                  // at the threshold: whole
  CHECK(check_plan({2}, 1) == 2);
  CHECK(check_plan({64}, 64) == 0);                // at the threshold: whole
  CHECK(check_plan({65}, 64) == 2);                // 64 + 1
  CHECK(check_plan({128}, 64) == 2);               // an exact multiple of the slice
  CHECK(check_plan({192, 64}, 64) == 3);
  CHECK(check_plan({200}, 64) == 4);               // 64 + 64 + 64 + 8
  CHECK(check_plan({3, 200, 0, 64, 130, 1, 65}, 64) == 4 + 3 + 2);  // mixed above and below
  CHECK(check_plan({40000}, 1024) == 40);
  CHECK(check_plan({40000, 512, 4}, 1024) == 40);
  CHECK(check_plan({200, 4000}, 0) == 0);          // 0 turns the split off
  CHECK(check_plan({5, 6}, UINT64_MAX) == 0);
}

struct Msgs {
  std::vector<uint8_t> blob;
  std::vector<uint64_t> off{0};
  void add(const std::string& m) {
    blob.insert(blob.end(), m.begin(), m.end());
    off.push_back(blob.size());
  }
  uint64_t n() const { return off.size() - 1; }
};

static void test_fold_and_read() {
  const uint32_t C = kHCacheColumn;
  // four groups over three distinct roots (one of them empty): two groups share a root
  Msgs g;
  g.add("root-a");
  g.add("");
  g.add("root-a");
  g.add("root-b");
  std::vector<uint8_t> umsg;
  std::vector<uint64_t> uoff;
  std::vector<uint32_t> mid, src, miss;
  distinct_messages(g.blob.data(), g.off.data(), g.n(), umsg, uoff, mid);
  CHECK(uoff.size() == 4);
  CHECK((mid == std::vector<uint32_t>{0, 1, 0, 2}));

  HCacheState hc;
  // cache off: every distinct message is a miss, nothing is counted
  hcache_reset(hc, 0);
  CHECK(!hcache_read(hc, umsg.data(), uoff.data(), 3, src, miss));
  CHECK((src == std::vector<uint32_t>{0, 1, 2}) && (miss == std::vector<uint32_t>{0, 1, 2}));
  CHECK(hc.hits == 0 && hc.misses == 0);

  // cold: misses counted per distinct message (the shared root once), and nothing inserted
  hcache_reset(hc, 8);
  CHECK(!hcache_read(hc, umsg.data(), uoff.data(), 3, src, miss));
  CHECK((src == std::vector<uint32_t>{0, 1, 2}) && miss.size() == 3);
  CHECK(hc.hits == 0 && hc.misses == 3 && hc.map.empty() && hc.ring == 0);

  // warm: a producer inserts root-a and the empty root; the read finds both, root-b stays a miss of the call's own
  Msgs w;
  w.add("filler");
  w.add("root-a");
  w.add("");
  std::vector<uint32_t> slot, wmiss;
  CHECK(hcache_assign(hc, w.blob.data(), w.off.data(), w.n(), slot, wmiss));
  CHECK(hc.map.size() == 3 && hc.ring == 3);
  const uint64_t hits0 = hc.hits, misses0 = hc.misses;
  CHECK(hcache_read(hc, umsg.data(), uoff.data(), 3, src, miss));
  CHECK((src == std::vector<uint32_t>{C | slot[1], C | slot[2], 2}));
  CHECK((miss == std::vector<uint32_t>{2}));
  CHECK(hc.hits == hits0 + 2 && hc.misses == misses0 + 1);
  CHECK(hc.map.size() == 3 && hc.ring == 3);  // read only: no insert, no eviction, the ring keeps its place
  CHECK(hc.map.count("root-b") == 0);

  // a capacity below the call's distinct messages: bypassed, as hcache_assign bypasses -- no lookup, no count
  hcache_reset(hc, 2);
  Msgs two;
  two.add("root-a");
  two.add("");
  CHECK(hcache_assign(hc, two.blob.data(), two.off.data(), 2, slot, wmiss));
  const uint64_t h1 = hc.hits, m1 = hc.misses;
  CHECK(!hcache_read(hc, umsg.data(), uoff.data(), 3, src, miss));
  CHECK((src == std::vector<uint32_t>{0, 1, 2}) && miss.size() == 3);
  CHECK(hc.hits == h1 && hc.misses == m1 && hc.map.size() == 2);
  // ... while a call that fits reads it
  CHECK(hcache_read(hc, umsg.data(), uoff.data(), 2, src, miss));
  CHECK(miss.empty() && hc.hits == h1 + 2);

  // no messages at all
  CHECK(!hcache_read(hc, nullptr, uoff.data(), 0, src, miss));
  CHECK(src.empty() && miss.empty());
}

int main() {
  test_planner();
  test_fold_and_read();
  puts("ok");
  return 0;
}
