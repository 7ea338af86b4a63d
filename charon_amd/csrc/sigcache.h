// Device-resident cache from a signature's 96 wire bytes to its decoded affine point: a partial
// signature reaches the engine twice, first in a Verify (parsigex, validatorapi) and then, with its duty's other
// partials, in sigagg.  The Verify kernels publish what they decoded; sigagg's scaling lanes look a partial up before
// they decompress and subgroup-test it.  Verify only inserts, sigagg only looks up.
//
// The key cache's three invariants (keycache.h) hold, stated for signatures, and its mixing, claim and
// compare-and-swap helpers and the root cache's probe sequence are reused:
//   1. only truths are stored: an entry is written only for wire bytes that decoded DEC_OK to a point proven to lie
//      in G2.  A bad encoding, x >= p, an off-curve x, a point outside G2, the infinity signature and a wrong flag
//      combination are never entries;
//   2. slots are write-once within a generation: claim[slot] goes 0 -> fingerprint by one compare-and-swap and the
//      winner alone writes the entry.  Signatures are a stream, so the host empties a half-full table (a new
//      generation, hipbls.hip sigcache_roll_if_due) with the device idle;
//   3. entries check themselves: a reader compares all 96 tag bytes and then a 64-bit check value over tag and y, on
//      its private copy.  Any mismatch is a miss, and a miss decodes as before.
// No fences, no cache control: ordering moves the hit rate, never a result.
//
// The pack/check part is plain C++ (tests/test_sigcache_host.py compiles it with g++); the probe and the insert are
// device code (serial stand-ins on a host build).
#pragma once
#include "rootcache.h"

namespace bls {

// Entry: 64 words, 256-byte aligned.
//   [0,24)  tag: the 96 wire bytes as received (flags included: S and -S share x and differ here), little-endian words
//   [24,48) y (c0, c1), canonical Montgomery form, as g2_decompress returns it (x is recomputed from the wire bytes)
//   [48,50) check value over tag and y, both halves non-zero
//   [50,64) zero
constexpr int SC_WORDS = 64;
constexpr int SC_TAG = 0, SC_Y = 24, SC_CHK = 48, SC_USED = 52;  // SC_USED: what a reader loads (a multiple of 4)
constexpr uint64_t SC_MAX_SLOTS = 1ull << 22;

// Passed to the kernels by value.  entries == nullptr: the cache is off.
struct sigcache {
  uint32_t* entries;        // slots x SC_WORDS
  uint32_t* claim;          // slots: 0 = empty, else the owner's fingerprint
  unsigned long long* ctr;  // hits, misses, inserts
  uint32_t mask;            // slots - 1
  uint32_t pad_;
};

KC_HD void sc_tag_from_wire(uint32_t tag[24], const uint8_t* b96) {
  for (int k = 0; k < 24; ++k)
    tag[k] = (uint32_t)b96[4 * k] | ((uint32_t)b96[4 * k + 1] << 8) | ((uint32_t)b96[4 * k + 2] << 16) |
             ((uint32_t)b96[4 * k + 3] << 24);
}
KC_HD uint64_t sc_tag_hash(const uint32_t tag[24]) { return kc_fold(0x082EFA98EC4E6C89ull, tag, 24); }
KC_HD uint64_t sc_check(uint64_t tag_hash, const uint32_t y[24]) {
  return kc_check_final(kc_fold(tag_hash ^ 0x3F84D5B5B5470917ull, y, 24));
}

KC_HD void sc_pack(uint32_t e[SC_WORDS], const uint32_t tag[24], const uint32_t y[24]) {
  for (int k = 0; k < 24; ++k) e[SC_TAG + k] = tag[k];
  for (int k = 0; k < 24; ++k) e[SC_Y + k] = y[k];
  const uint64_t c = sc_check(sc_tag_hash(tag), y);
  e[SC_CHK] = (uint32_t)c;
  e[SC_CHK + 1] = (uint32_t)(c >> 32);
  for (int k = SC_CHK + 2; k < SC_WORDS; ++k) e[k] = 0;
}

// Does this copy of an entry hold `tag`'s signature?  e is the reader's private copy of words [0, SC_USED).  An
// all-zero slot never matches, the all-zero tag included: a stored check value has both halves non-zero.
KC_HD bool sc_entry_get(const uint32_t* e, const uint32_t tag[24], uint32_t y[24]) {
  uint32_t diff = 0;
  for (int k = 0; k < 24; ++k) diff |= e[SC_TAG + k] ^ tag[k];
  if (diff) return false;
  const uint64_t c = sc_check(sc_tag_hash(tag), e + SC_Y);
  if (e[SC_CHK] != (uint32_t)c || e[SC_CHK + 1] != (uint32_t)(c >> 32)) return false;
  for (int k = 0; k < 24; ++k) y[k] = e[SC_Y + k];
  return true;
}

// Probe the root cache's sequence (RC_PROBES windows of KC_WINDOW slots; a single window that fills would silently
// lose hits in a stream) for `tag`.  A plain load of claim decides per slot: zero ends the probe as a miss, this
// signature's fingerprint reads the entry and verifies it.  A stale zero only costs a hit.
KC_HD bool sc_lookup(const sigcache& sc, const uint32_t tag[24], uint32_t y[24]) {
  const uint64_t th = sc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, sc.mask);
    const uint32_t c = kc_load_claim(sc.claim + s);
    if (!c) return false;
    if (c != fpr) continue;
    uint32_t e[SC_WORDS];
    kc_load_words(e, sc.entries + (uint64_t)s * SC_WORDS, 0, SC_USED);
    if (sc_entry_get(e, tag, y)) return true;
  }
  return false;
}

// Publish a signature that decoded DEC_OK and is proven to lie in G2 (keycache.h kc_insert's rules: the first empty
// slot of the sequence by compare-and-swap, the winner writes, a lane that meets its own fingerprint stops, a full
// sequence publishes nothing).  Returns whether this lane wrote an entry.
KC_HD bool sc_insert(const sigcache& sc, const uint32_t tag[24], const uint32_t y[24]) {
  const uint64_t th = sc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, sc.mask);
    uint32_t c = kc_load_claim(sc.claim + s);
    if (!c) c = kc_cas_claim(sc.claim + s, fpr);  // a stale zero is settled here: the swap returns the truth
    if (c == fpr) return false;
    if (c) continue;
    uint32_t e[SC_WORDS];
    sc_pack(e, tag, y);
    kc_store_entry(sc.entries + (uint64_t)s * SC_WORDS, e);
    return true;
  }
  return false;
}

// One counter (0 hits, 1 misses, 2 inserts) raised by the number of active lanes with `flag`, once per wave
// (rootcache.h rc_count on this cache's counters).
KC_HD void sc_count(const sigcache& sc, int which, bool flag) {
  rootcache r{};
  r.ctr = sc.ctr;
  rc_count(r, which, flag);
}

// Whether a generation is due to end (host side): the inserts since it began have reached half the slots.
KC_HD bool sc_generation_due(uint64_t inserts, uint64_t gen_base, uint64_t slots) {
  return slots != 0 && inserts - gen_base >= slots / 2;
}

}  // namespace bls
