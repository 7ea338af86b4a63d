// Stand-alone host check of the H(m) prefetch's bookkeeping (charon_amd/csrc/hcache_assign.h: distinct_messages and
// the non-counting form of hcache_assign, as hipbls.hip hcache_prefetch_on uses them), built with
// -fsanitize=address,undefined and run as a program by tests/test_hcache_prefetch_static.py.  Exit status 0 and "ok"
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
  explicit Call(const std::vector<std::string>& msgs) {
    for (const std::string& m : msgs) {
      blob.insert(blob.end(), m.begin(), m.end());
      offs.push_back(blob.size());
    }
    if (blob.empty()) blob.push_back(0);
  }
  uint64_t n() const { return offs.size() - 1; }
};

HCacheState make(uint64_t cap) {
  HCacheState hc;
  hcache_reset(hc, cap);
  return hc;
}

// map, key_of and live describe the same set (hcache_assign_main.cpp's invariant).
void consistent(const HCacheState& hc) {
  CHECK(hc.key_of.size() == hc.cap && hc.live.size() == hc.cap);
  CHECK(hc.cap == 0 || hc.ring < hc.cap);
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

// What hcache_prefetch_on does on the host: fold, assign without counting, report.  `fail` stands for a launch that
// failed after the assignment (the Undo guard's erase).
struct Prefetch {
  bool through = false;
  uint64_t hashed = 0, present = 0;
  std::vector<uint32_t> slot, miss;
  std::vector<std::string> roots;  // the distinct roots, in first-use order
};
Prefetch prefetch(HCacheState& hc, const std::vector<std::string>& msgs, bool fail = false) {
  Call c(msgs);
  std::vector<uint8_t> umsg;
  std::vector<uint64_t> uoff;
  std::vector<uint32_t> mid;
  distinct_messages(c.blob.data(), c.offs.data(), c.n(), umsg, uoff, mid);
  if (umsg.empty()) umsg.push_back(0);
  Prefetch p;
  const uint64_t n = uoff.size() - 1;
  CHECK(mid.size() == c.n());
  for (uint64_t m = 0; m < n; ++m) p.roots.emplace_back((const char*)umsg.data() + uoff[m], uoff[m + 1] - uoff[m]);
  for (uint64_t i = 0; i < c.n(); ++i) CHECK(mid[i] < n && p.roots[mid[i]] == msgs[i]);
  CHECK(std::set<std::string>(p.roots.begin(), p.roots.end()).size() == n);
  const uint64_t hits = hc.hits, misses = hc.misses;
  p.through = hcache_assign(hc, umsg.data(), uoff.data(), n, p.slot, p.miss, false);
  CHECK(hc.hits == hits && hc.misses == misses);  // the counters describe consumers
  if (!p.through) return p;
  if (fail) {
    hcache_erase_misses(hc, umsg.data(), uoff.data(), p.slot, p.miss);
  } else {
    p.hashed = p.miss.size();
    p.present = n - p.miss.size();
    std::set<uint32_t> used;
    for (uint64_t m = 0; m < n; ++m) {
      auto it = hc.map.find(p.roots[m]);
      CHECK(it != hc.map.end() && it->second == p.slot[m]);
      CHECK(used.insert(p.slot[m]).second);
    }
  }
  consistent(hc);
  return p;
}

// A consumer (a keyed Verify) of the same roots: the counting form.
std::vector<uint32_t> consume(HCacheState& hc, const std::vector<std::string>& roots, std::vector<uint32_t>& slot) {
  Call c(roots);
  std::vector<uint32_t> miss;
  CHECK(hcache_assign(hc, c.blob.data(), c.offs.data(), c.n(), slot, miss));
  consistent(hc);
  return miss;
}

void counters_and_duplicates() {
  HCacheState hc = make(8);
  // a duplicate inside the call, the empty message and a long one
  Prefetch p = prefetch(hc, {"root-a", "", "root-a", std::string(200, 'x'), ""});
  CHECK(p.through && p.hashed == 3 && p.present == 0);
  CHECK((p.roots == std::vector<std::string>{"root-a", "", std::string(200, 'x')}));
  CHECK((p.slot == std::vector<uint32_t>{0, 1, 2}) && (p.miss == std::vector<uint32_t>{0, 1, 2}));
  CHECK(hc.hits == 0 && hc.misses == 0 && hc.map.size() == 3 && hc.ring == 3);
  // the Verify that follows shows up as hits, in the prefetch's columns
  std::vector<uint32_t> slot;
  CHECK(consume(hc, {"root-a", ""}, slot).empty());
  CHECK(slot[0] == 0 && slot[1] == 1 && hc.hits == 2 && hc.misses == 0);
  // mixed: two cached, two new, one duplicate of a new one; only the new roots take ring slots
  p = prefetch(hc, {"root-b", "root-a", "root-b", "root-c", ""});
  CHECK(p.through && p.hashed == 2 && p.present == 2);
  CHECK((p.miss == std::vector<uint32_t>{0, 2}));
  CHECK(p.slot[0] == 3 && p.slot[1] == 0 && p.slot[2] == 4 && p.slot[3] == 1 && hc.ring == 5);
  CHECK(hc.hits == 2 && hc.misses == 0 && hc.map.size() == 5);
  // everything present: nothing to hash, nothing moves
  p = prefetch(hc, {"root-c", "root-a"});
  CHECK(p.through && p.hashed == 0 && p.present == 2 && hc.ring == 5 && hc.map.size() == 5);
}

void wrap_and_demotion() {
  HCacheState hc = make(4);
  Prefetch p = prefetch(hc, {"a", "b", "c"});
  CHECK(p.hashed == 3 && (p.slot == std::vector<uint32_t>{0, 1, 2}) && hc.ring == 3);
  // "a" sits in slot 0, which the misses d, e (slots 3, 0) would take: demoted and re-hashed; b is evicted, c stays
  p = prefetch(hc, {"a", "d", "e"});
  CHECK(p.hashed == 3 && p.present == 0);
  CHECK((p.slot == std::vector<uint32_t>{3, 0, 1}) && hc.ring == 2);
  CHECK(hc.map.size() == 4 && hc.map.count("b") == 0 && hc.map.at("c") == 2);
  // an evicted root is a miss for its consumer, a surviving one a hit
  std::vector<uint32_t> slot;
  CHECK((consume(hc, {"c"}, slot) == std::vector<uint32_t>{}) && slot[0] == 2);
  CHECK((consume(hc, {"b"}, slot) == std::vector<uint32_t>{0}) && slot[0] == 2);  // takes ring slot 2: c goes
  CHECK(hc.hits == 1 && hc.misses == 1 && hc.map.count("c") == 0 && hc.ring == 3);
  // a hit outside the misses' range stays present: "e" in slot 1, the miss f takes slot 3 (a goes)
  p = prefetch(hc, {"e", "f"});
  CHECK(p.hashed == 1 && p.present == 1 && p.slot[0] == 1 && p.slot[1] == 3 && hc.ring == 0);
  CHECK(hc.map.count("a") == 0 && hc.hits == 1 && hc.misses == 1);
  // exactly the capacity: every root is new, the whole ring turns over
  p = prefetch(hc, {"w", "x", "y", "z"});
  CHECK(p.hashed == 4 && p.present == 0 && (p.slot == std::vector<uint32_t>{0, 1, 2, 3}) && hc.ring == 0);
  CHECK(hc.map.size() == 4 && hc.map.count("e") == 0);
}

void bypass() {
  HCacheState hc = make(4);
  Prefetch p = prefetch(hc, {"a", "b", "c", "d", "e"});  // five distinct roots into four columns
  CHECK(!p.through && p.hashed == 0 && p.present == 0 && hc.map.empty() && hc.ring == 0);
  consistent(hc);
  p = prefetch(hc, {"a", "b", "a", "c", "b", "d"});  // six items, four distinct: goes through
  CHECK(p.through && p.hashed == 4);
  HCacheState off = make(0);
  p = prefetch(off, {"a"});
  CHECK(!p.through && p.hashed == 0 && p.present == 0 && off.map.empty());
  consistent(off);
}

void failed_prefetch() {
  HCacheState hc = make(4);
  CHECK(prefetch(hc, {"a", "b"}).hashed == 2);
  // b present (slot 1), x and y assigned 2 and 3 -- then the launch fails
  Prefetch p = prefetch(hc, {"b", "x", "y", "x"}, true);
  CHECK(p.through && (p.miss == std::vector<uint32_t>{1, 2}));
  CHECK(hc.map.size() == 2 && hc.map.at("a") == 0 && hc.map.at("b") == 1);
  CHECK(!hc.live[2] && !hc.live[3] && hc.hits == 0 && hc.misses == 0);
  // the consumer hashes x itself instead of reading the unwritten column
  std::vector<uint32_t> slot;
  CHECK((consume(hc, {"x"}, slot) == std::vector<uint32_t>{0}) && hc.misses == 1);
  // a failed prefetch whose misses evicted live entries: those stay gone, nothing points at the unwritten columns
  p = prefetch(hc, {"p", "q", "r", "s"}, true);
  CHECK(p.through && p.miss.size() == 4 && hc.map.empty());
}

}  // namespace

int main() {
  counters_and_duplicates();
  wrap_and_demotion();
  bypass();
  failed_prefetch();
  puts("ok");
  return 0;
}
