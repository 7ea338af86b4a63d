// The H(m) cache's host-side bookkeeping (hipbls.hip HCache): which signing root sits in which column of the resident
// table, FIFO replacement over a ring of columns.  Standard C++ only (no HIP), so the hit-demotion fixed point and the
// error-path erase are built and tested on the host (tests/native/hcache_assign_main.cpp).
#pragma once
#include <cstdint>
#include <string>
#include <unordered_map>
#include <vector>

struct HCacheState {
  uint64_t cap = 0;  // 0 = disabled
  uint64_t ring = 0;
  std::unordered_map<std::string, uint32_t> map;
  std::vector<std::string> key_of;  // slot -> key
  std::vector<uint8_t> live;        // slot holds a key (the empty message's key is "", so key_of alone cannot tell)
  uint64_t hits = 0, misses = 0;
};

// An empty cache of `cap` columns (0 = disabled), counters zero.
inline void hcache_reset(HCacheState& hc, uint64_t cap) {
  hc.map.clear();
  hc.key_of.assign(cap, std::string());
  hc.live.assign(cap, 0);
  hc.ring = 0;
  hc.hits = hc.misses = 0;
  hc.cap = cap;
}

// The distinct messages of n items in first-use order (umsg / uoff) and each item's index among them: the message
// table that hcache_assign takes (the keyed Verify latency route, the queue's keyed batches, the prefetch).
inline void distinct_messages(const uint8_t* msgs, const uint64_t* offs, uint64_t n, std::vector<uint8_t>& umsg,
                              std::vector<uint64_t>& uoff, std::vector<uint32_t>& mid) {
  std::unordered_map<std::string, uint32_t> pos;
  mid.resize(n);
  umsg.clear();
  uoff.assign(1, 0);
  for (uint64_t i = 0; i < n; ++i) {
    std::string key((const char*)msgs + offs[i], offs[i + 1] - offs[i]);
    auto it = pos.find(key);
    if (it == pos.end()) {
      it = pos.emplace(std::move(key), (uint32_t)(uoff.size() - 1)).first;
      umsg.insert(umsg.end(), msgs + offs[i], msgs + offs[i + 1]);
      uoff.push_back(umsg.size());
    }
    mid[i] = it->second;
  }
}

// Assigns cache columns for the n_msgs distinct messages of one call: fills slot[m] and the list of messages that
// must be hashed (misses).  Returns false (cache bypassed) when disabled or the call has more messages than slots.
// count = false is the prefetch's form (hipbls_hcache_prefetch): the same slots, ring and map, but the hits / misses
// counters stay put, since they describe the calls that consume H(m).
inline bool hcache_assign(HCacheState& hc, const uint8_t* msgs, const uint64_t* offs, uint64_t n_msgs,
                          std::vector<uint32_t>& slot, std::vector<uint32_t>& miss, bool count = true) {
  if (hc.cap == 0 || n_msgs > hc.cap) return false;
  slot.assign(n_msgs, 0);
  miss.clear();
  std::vector<std::string> keys(n_msgs);
  std::vector<char> hit(n_msgs, 0);
  for (uint64_t m = 0; m < n_msgs; ++m) {
    keys[m].assign((const char*)msgs + offs[m], offs[m + 1] - offs[m]);
    auto it = hc.map.find(keys[m]);
    if (it != hc.map.end()) {
      slot[m] = (uint32_t)it->second;
      hit[m] = 1;
    }
  }
  // The misses take slots [ring, ring + k); a hit inside that range would be overwritten by this very call, so it
  // is demoted to a miss (which grows k): iterate to the fixed point.
  for (;;) {
    uint64_t k = 0;
    for (uint64_t m = 0; m < n_msgs; ++m) k += hit[m] ? 0 : 1;
    bool changed = false;
    for (uint64_t m = 0; m < n_msgs; ++m)
      if (hit[m] && (slot[m] + hc.cap - hc.ring) % hc.cap < k) {
        hit[m] = 0;
        changed = true;
      }
    if (!changed) break;
  }
  for (uint64_t m = 0; m < n_msgs; ++m) {
    if (hit[m]) {
      if (count) hc.hits += 1;
      continue;
    }
    // messages are distinct within a call (the caller's message table), so each miss takes its own slot
    const uint32_t s = (uint32_t)hc.ring;
    hc.ring = (hc.ring + 1) % hc.cap;
    // a demoted hit still sits in the map under its old slot: that slot's key_of must not keep naming it
    auto old = hc.map.find(keys[m]);
    if (old != hc.map.end() && old->second != s && hc.live[old->second] && hc.key_of[old->second] == keys[m])
      hc.live[old->second] = 0;
    if (hc.live[s]) hc.map.erase(hc.key_of[s]);
    hc.key_of[s] = keys[m];
    hc.live[s] = 1;
    hc.map[keys[m]] = s;
    slot[m] = s;
    miss.push_back((uint32_t)m);
    if (count) hc.misses += 1;
  }
  return true;
}

// The read-only lookup of a call that consumes a root last (the keyed FastAggregateVerify, hipbls.hip fav_keys_host):
// src[m] = kHCacheColumn | column for a message the cache holds, else m itself, the message's column in a table of the
// call's own, and `miss` lists those messages (the ones the call hashes).  Hits and misses count per distinct message;
// nothing is inserted or evicted and the ring keeps its place, so there is nothing to undo when the call fails.
// Bypassed exactly where hcache_assign bypasses (disabled, or more messages than columns): every message is the call's
// own and nothing counts.  Returns whether any message was found.
constexpr uint32_t kHCacheColumn = 0x80000000u;
inline bool hcache_read(HCacheState& hc, const uint8_t* msgs, const uint64_t* offs, uint64_t n_msgs,
                        std::vector<uint32_t>& src, std::vector<uint32_t>& miss) {
  const bool lookup = hc.cap != 0 && n_msgs <= hc.cap;
  src.assign(n_msgs, 0);
  miss.clear();
  bool any = false;
  for (uint64_t m = 0; m < n_msgs; ++m) {
    auto it = lookup ? hc.map.find(std::string((const char*)msgs + offs[m], offs[m + 1] - offs[m])) : hc.map.end();
    if (it != hc.map.end()) {
      src[m] = kHCacheColumn | (uint32_t)it->second;
      hc.hits += 1;
      any = true;
    } else {
      src[m] = (uint32_t)m;
      miss.push_back((uint32_t)m);
      if (lookup) hc.misses += 1;
    }
  }
  return any;
}

// The error path of a call whose launch failed after hcache_assign: its misses' columns were never written, so their
// entries leave the map (a later call hashes those roots again instead of reading an unwritten column as H(m)).  The
// entries the misses evicted stay gone; the ring keeps its place.
inline void hcache_erase_misses(HCacheState& hc, const uint8_t* msgs, const uint64_t* offs,
                                const std::vector<uint32_t>& slot, const std::vector<uint32_t>& miss) {
  for (uint32_t m : miss) {
    const std::string key((const char*)msgs + offs[m], offs[m + 1] - offs[m]);
    auto it = hc.map.find(key);
    if (it == hc.map.end() || it->second != slot[m]) continue;
    hc.map.erase(it);
    if (slot[m] < hc.cap && hc.key_of[slot[m]] == key) hc.live[slot[m]] = 0;
  }
}
