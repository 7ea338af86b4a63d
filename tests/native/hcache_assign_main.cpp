// Stand-alone host check of the H(m) cache's bookkeeping (charon_amd/csrc/hcache_assign.h), built with
// -fsanitize=address,undefined and run as a program by tests/test_verify_keys_lat_static.py.  Exit status 0 and "ok"
// when every case holds; otherwise the failed condition's line and status 1.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <string>
#include <vector>

#include "hcache_assign.h"

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
      exit(1);                                                          \
    }                                                                   \
  } while (0)

namespace {

struct Call {
  std::vector<uint8_t> blob;
  std::vector<uint64_t> offs{0};
  std::vector<std::string> keys;
  explicit Call(const std::vector<std::string>& msgs) : keys(msgs) {
    for (const std::string& m : msgs) {
      blob.insert(blob.end(), m.begin(), m.end());
      offs.push_back(blob.size());
    }
    if (blob.empty()) blob.push_back(0);
  }
  uint64_t n() const { return keys.size(); }
};

HCacheState make(uint64_t cap) {
  HCacheState hc;
  hcache_reset(hc, cap);
  return hc;
}

// The map and key_of describe the same set: every map entry's slot names its key, every non-empty slot is in the map
// under its own index, so no two live keys share a slot.
void consistent(const HCacheState& hc) {
  CHECK(hc.key_of.size() == hc.cap && hc.live.size() == hc.cap);
  CHECK(hc.ring < hc.cap);
  std::set<uint32_t> used;
  for (const auto& kv : hc.map) {
    CHECK(kv.second < hc.cap);
    CHECK(hc.live[kv.second] && hc.key_of[kv.second] == kv.first);
    CHECK(used.insert(kv.second).second);
  }
  uint64_t live = 0;
  for (uint64_t s = 0; s < hc.cap; ++s)
    if (hc.live[s]) {
      auto it = hc.map.find(hc.key_of[s]);
      CHECK(it != hc.map.end() && it->second == s);
      ++live;
    }
  CHECK(live == hc.map.size());
}

// After a call through the cache: each message's slot is where the map has it, and distinct messages got distinct
// slots (no column is written and read for two messages of one call).
void assigned(const HCacheState& hc, const Call& c, const std::vector<uint32_t>& slot) {
  CHECK(slot.size() == c.n());
  std::set<uint32_t> used;
  for (uint64_t m = 0; m < c.n(); ++m) {
    auto it = hc.map.find(c.keys[m]);
    CHECK(it != hc.map.end() && it->second == slot[m]);
    CHECK(used.insert(slot[m]).second);
  }
}

void cold_and_warm() {
  HCacheState hc = make(8);
  Call c({"root-a", "root-b", std::string(200, 'x')});
  std::vector<uint32_t> slot, miss;
  CHECK(hcache_assign(hc, c.blob.data(), c.offs.data(), c.n(), slot, miss));
  CHECK((miss == std::vector<uint32_t>{0, 1, 2}));
  CHECK((slot == std::vector<uint32_t>{0, 1, 2}));
  CHECK(hc.hits == 0 && hc.misses == 3 && hc.map.size() == 3 && hc.ring == 3);
  consistent(hc);
  assigned(hc, c, slot);
  const std::vector<uint32_t> first = slot;
  CHECK(hcache_assign(hc, c.blob.data(), c.offs.data(), c.n(), slot, miss));  // warm: the same columns, nothing to hash
  CHECK(miss.empty() && slot == first);
  CHECK(hc.hits == 3 && hc.misses == 3 && hc.map.size() == 3 && hc.ring == 3);
  consistent(hc);
  Call d({"root-b", "root-c"});  // one hit, one miss
  CHECK(hcache_assign(hc, d.blob.data(), d.offs.data(), d.n(), slot, miss));
  CHECK((miss == std::vector<uint32_t>{1}) && slot[0] == 1 && slot[1] == 3);
  CHECK(hc.hits == 4 && hc.misses == 4);
  consistent(hc);
  assigned(hc, d, slot);
}

void bypass() {
  HCacheState hc = make(2);
  Call c({"a", "b", "c"});
  std::vector<uint32_t> slot{7}, miss{9};
  CHECK(!hcache_assign(hc, c.blob.data(), c.offs.data(), c.n(), slot, miss));  // more messages than slots
  CHECK(hc.map.empty() && hc.hits == 0 && hc.misses == 0 && hc.ring == 0);
  consistent(hc);
  HCacheState off = make(0);
  CHECK(!hcache_assign(off, c.blob.data(), c.offs.data(), 1, slot, miss));  // disabled
  CHECK(off.map.empty() && off.misses == 0);
}

void wrap_and_demotion() {
  HCacheState hc = make(4);
  std::vector<uint32_t> slot, miss;
  Call c1({"a", "b", "c"});
  CHECK(hcache_assign(hc, c1.blob.data(), c1.offs.data(), 3, slot, miss));
  CHECK((slot == std::vector<uint32_t>{0, 1, 2}) && miss.size() == 3 && hc.ring == 3);
  consistent(hc);
  assigned(hc, c1, slot);
  // "a" is cached in slot 0, but the misses d, e take slots 3 and 0: the hit is demoted, and then the three misses
  // take 3, 0, 1 -- "a" moves to slot 3, "b" is evicted, "c" (slot 2) stays
  Call c2({"a", "d", "e"});
  CHECK(hcache_assign(hc, c2.blob.data(), c2.offs.data(), 3, slot, miss));
  CHECK((miss == std::vector<uint32_t>{0, 1, 2}));
  CHECK((slot == std::vector<uint32_t>{3, 0, 1}));
  CHECK(hc.hits == 0 && hc.misses == 6 && hc.ring == 2);
  CHECK(hc.map.size() == 4 && hc.map.count("b") == 0 && hc.map.at("c") == 2);
  consistent(hc);
  assigned(hc, c2, slot);
  // "c" sits in slot 2 = ring: the two misses f, g would take 2 and 3, so "c" is demoted too, and with three misses
  // the range reaches slot 0... which holds "d", not part of this call.  The call ends with c, f, g in 2, 3, 0.
  Call c3({"c", "f", "g"});
  CHECK(hcache_assign(hc, c3.blob.data(), c3.offs.data(), 3, slot, miss));
  CHECK((miss == std::vector<uint32_t>{0, 1, 2}));
  CHECK((slot == std::vector<uint32_t>{2, 3, 0}));
  CHECK(hc.hits == 0 && hc.misses == 9 && hc.ring == 1);
  CHECK(hc.map.size() == 4 && hc.map.at("e") == 1 && hc.map.count("a") == 0 && hc.map.count("d") == 0);
  consistent(hc);
  assigned(hc, c3, slot);
  // a hit outside the misses' range stays a hit: "e" in slot 1 = ring would go, "g" in slot 0 stays
  Call c4({"g", "h"});
  CHECK(hcache_assign(hc, c4.blob.data(), c4.offs.data(), 2, slot, miss));
  CHECK((miss == std::vector<uint32_t>{1}) && slot[0] == 0 && slot[1] == 1);
  CHECK(hc.hits == 1 && hc.misses == 10 && hc.map.count("e") == 0);
  consistent(hc);
  assigned(hc, c4, slot);
}

void error_path_erase() {
  HCacheState hc = make(4);
  std::vector<uint32_t> slot, miss;
  Call c1({"a", "b"});
  CHECK(hcache_assign(hc, c1.blob.data(), c1.offs.data(), 2, slot, miss));
  Call c2({"b", "x", "y"});  // hit b (slot 1), misses x, y in 2, 3 -- then the launch fails
  CHECK(hcache_assign(hc, c2.blob.data(), c2.offs.data(), 3, slot, miss));
  CHECK((miss == std::vector<uint32_t>{1, 2}) && slot[0] == 1);
  hcache_erase_misses(hc, c2.blob.data(), c2.offs.data(), slot, miss);
  CHECK(hc.map.size() == 2 && hc.map.count("x") == 0 && hc.map.count("y") == 0);
  CHECK(hc.map.at("a") == 0 && hc.map.at("b") == 1);  // entries whose columns were written stay
  CHECK(!hc.live[2] && !hc.live[3]);
  consistent(hc);
  // the next call hashes x again instead of reading the unwritten column
  Call c3({"x"});
  CHECK(hcache_assign(hc, c3.blob.data(), c3.offs.data(), 1, slot, miss));
  CHECK((miss == std::vector<uint32_t>{0}));
  consistent(hc);
  assigned(hc, c3, slot);
  // the empty message is a key like any other: evicted when its column is taken (its key "" is no empty slot's mark)
  HCacheState he = make(2);
  Call e1({"", "k"}), e2({"l", "m"}), e3({""});
  CHECK(hcache_assign(he, e1.blob.data(), e1.offs.data(), 2, slot, miss) && miss.size() == 2);
  consistent(he);
  CHECK(hcache_assign(he, e2.blob.data(), e2.offs.data(), 2, slot, miss) && miss.size() == 2);
  CHECK(he.map.count("") == 0 && he.map.size() == 2);
  consistent(he);
  CHECK(hcache_assign(he, e3.blob.data(), e3.offs.data(), 1, slot, miss) && miss.size() == 1);
  consistent(he);
  // a failed call whose misses evicted live entries: those stay gone, nothing points at the unwritten columns
  Call c4({"p", "q", "r", "s"});
  CHECK(hcache_assign(hc, c4.blob.data(), c4.offs.data(), 4, slot, miss));
  CHECK(miss.size() == 4);
  hcache_erase_misses(hc, c4.blob.data(), c4.offs.data(), slot, miss);
  CHECK(hc.map.empty());
  consistent(hc);
}

}  // namespace

int main() {
  cold_and_warm();
  bypass();
  wrap_and_demotion();
  error_path_erase();
  puts("ok");
  return 0;
}
