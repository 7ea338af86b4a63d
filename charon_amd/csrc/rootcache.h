// Device-resident cache from a 32-byte signing root to H(m), its hash to G2 in affine form: the
// wire-format fused Verify (kernels.h k_root_lookup, k_verify_fused) looks a root up before it hashes it, and publishes
// what it hashed.  Only messages of exactly 32 bytes are eligible, and only Verify fills the cache, so every stored
// point is a DST_POP hash.
//
// The key cache's three invariants (keycache.h) hold unchanged, and its mixing, claim and compare-and-swap helpers are
// reused:
//   1. only truths are stored: a lane inserts only the H it just computed for the bytes it tagged, never an infinity;
//   2. slots are write-once within a generation: claim[slot] goes 0 -> fingerprint by one compare-and-swap and the
//      winner alone writes the entry.  Roots age, unlike keys, so the host empties a half-full table (a new
//      generation, hipbls.hip rootcache_roll_if_due) -- with the device idle, never beside a kernel that could read a slot;
//   3. entries check themselves: a reader compares all 32 tag bytes with the item's message and then a 64-bit check
//      value over the tag and H, over its private copy.  Any mismatch is a miss, and a miss hashes as before.
//
// The pack/check part is plain C++ (tests/test_rootcache_host.py compiles it with g++); the probe and the insert are
// device code (serial stand-ins on a host build).
#pragma once
#include "keycache.h"

namespace bls {

// Entry: 64 words, 256-byte aligned.
//   [0,8)   tag: the 32 message bytes, little-endian words
//   [8,56)  H(m), affine, as jac_to_aff returns it (x.c0, x.c1, y.c0, y.c1: canonical Montgomery form)
//   [56,58) check value over tag and H, both halves non-zero
//   [58,64) unused, zero
constexpr int RC_WORDS = 64;
constexpr int RC_TAG = 0, RC_H = 8, RC_CHK = 56, RC_USED = 60;  // RC_USED: what a reader loads (a multiple of 4)
constexpr uint32_t RC_MSG_BYTES = 32;
constexpr uint32_t RC_NONE = 0xffffffffu;  // "no slot recorded" in k_root_lookup's pslot

// Passed to the kernels by value.  entries == nullptr: the cache is off.
struct rootcache {
  uint32_t* entries;        // slots x RC_WORDS
  uint32_t* claim;          // slots: 0 = empty, else the owner's fingerprint
  unsigned long long* ctr;  // hits, misses, inserts
  uint32_t mask;            // slots - 1
  uint32_t pad_;
};

KC_HD void rc_tag_from_msg(uint32_t tag[8], const uint8_t* m32) {
  for (int k = 0; k < 8; ++k)
    tag[k] = (uint32_t)m32[4 * k] | ((uint32_t)m32[4 * k + 1] << 8) | ((uint32_t)m32[4 * k + 2] << 16) |
             ((uint32_t)m32[4 * k + 3] << 24);
}
KC_HD uint64_t rc_tag_hash(const uint32_t tag[8]) { return kc_fold(0x452821E638D01377ull, tag, 8); }
KC_HD uint64_t rc_check(uint64_t tag_hash, const uint32_t h[48]) {
  return kc_check_final(kc_fold(tag_hash ^ 0xBE5466CF34E90C6Cull, h, 48));
}

KC_HD void rc_pack(uint32_t e[RC_WORDS], const uint32_t tag[8], const uint32_t h[48]) {
  for (int k = 0; k < 8; ++k) e[RC_TAG + k] = tag[k];
  for (int k = 0; k < 48; ++k) e[RC_H + k] = h[k];
  const uint64_t c = rc_check(rc_tag_hash(tag), h);
  e[RC_CHK] = (uint32_t)c;
  e[RC_CHK + 1] = (uint32_t)(c >> 32);
  for (int k = RC_CHK + 2; k < RC_WORDS; ++k) e[k] = 0;
}

// Does this copy of an entry hold `tag`'s root?  e is the reader's private copy of words [0, RC_USED).  An all-zero
// slot never matches, the all-zero message included: a stored check value has both halves non-zero.  h (when given)
// receives the packed H(m) on true.
KC_HD bool rc_entry_get(const uint32_t* e, const uint32_t tag[8], uint32_t* h /* 48 or null */) {
  uint32_t diff = 0;
  for (int k = 0; k < 8; ++k) diff |= e[RC_TAG + k] ^ tag[k];
  if (diff) return false;
  const uint64_t c = rc_check(rc_tag_hash(tag), e + RC_H);
  if (e[RC_CHK] != (uint32_t)c || e[RC_CHK + 1] != (uint32_t)(c >> 32)) return false;
  if (h)
    for (int k = 0; k < 48; ++k) h[k] = e[RC_H + k];
  return true;
}

// The probe sequence: RC_PROBES windows of KC_WINDOW consecutive slots, the first at the key cache's home slot, the
// others at rehashed homes.  One window is not enough here: a call of the fused kernel is as slow as its slowest
// wave, so a handful of roots whose only window was full (measured: 3 to 9 of 65,536 at a quarter load) made a warm
// call as slow as a cold one.  With four independent windows that takes four full ones.
constexpr int RC_PROBES = 4;
constexpr int RC_SEQ = RC_PROBES * KC_WINDOW;
KC_HD uint32_t rc_seq_slot(uint64_t tag_hash, int j, uint32_t mask) {  // j in [0, RC_SEQ)
  const int p = j / KC_WINDOW;
  const uint32_t home = p ? (uint32_t)(kc_mix(tag_hash, (uint32_t)p) >> 20) : kc_home(tag_hash, mask);
  return (home + (uint32_t)(j % KC_WINDOW)) & mask;
}

// Probe the sequence for `tag` and return the slot whose entry verifies, or RC_NONE.  A plain load of claim decides
// per slot: zero ends the probe (an insert would have taken that slot), this root's fingerprint reads the entry and
// verifies it.
KC_HD uint32_t rc_find(const rootcache& rc, const uint32_t tag[8]) {
  const uint64_t th = rc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, rc.mask);
    const uint32_t c = kc_load_claim(rc.claim + s);
    if (!c) return RC_NONE;
    if (c != fpr) continue;
    uint32_t e[RC_WORDS];
    kc_load_words(e, rc.entries + (uint64_t)s * RC_WORDS, 0, RC_USED);
    if (rc_entry_get(e, tag, nullptr)) return s;
  }
  return RC_NONE;
}

// A recorded slot's entry, loaded and verified over this reader's own copy (slot <= mask: k_root_lookup recorded it
// under the same struct; the mask is applied again so that no value of `slot` reads outside the table).
KC_HD bool rc_get_slot(const rootcache& rc, uint32_t slot, const uint32_t tag[8], uint32_t h[48]) {
  uint32_t e[RC_WORDS];
  kc_load_words(e, rc.entries + (uint64_t)(slot & rc.mask) * RC_WORDS, 0, RC_USED);
  return rc_entry_get(e, tag, h);
}

// Publish the H(m) a lane just computed for `tag`'s bytes (keycache.h kc_insert's rules: first empty slot of the
// sequence by compare-and-swap, the winner writes, a lane that meets its own fingerprint stops, a full sequence
// publishes nothing).  Returns whether this lane wrote an entry.
KC_HD bool rc_insert(const rootcache& rc, const uint32_t tag[8], const uint32_t h[48]) {
  const uint64_t th = rc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, rc.mask);
    uint32_t c = kc_load_claim(rc.claim + s);
    if (!c) c = kc_cas_claim(rc.claim + s, fpr);
    if (c == fpr) return false;
    if (c) continue;
    uint32_t e[RC_WORDS];
    rc_pack(e, tag, h);
    kc_store_entry(rc.entries + (uint64_t)s * RC_WORDS, e);
    return true;
  }
  return false;
}

// One counter (0 hits, 1 misses, 2 inserts) raised by the number of active lanes with `flag`, once per wave.
#if defined(__HIP_DEVICE_COMPILE__)
KC_HD void rc_count(const rootcache& rc, int which, bool flag) {
  const uint64_t act = __ballot(1), m = __ballot(flag);
  if (!m) return;
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane != (uint32_t)(__ffsll((unsigned long long)act) - 1)) return;
  __hip_atomic_fetch_add((kc_gu64*)rc.ctr + which, (unsigned long long)__popcll(m), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}
#else
KC_HD void rc_count(const rootcache& rc, int which, bool flag) {
  if (flag) rc.ctr[which] += 1;
}
#endif

}  // namespace bls
