// Device-resident cache from a public key's 48 wire bytes to its decoded form: the wire-format
// Verify and RLC kernels look a key up before they decompress and subgroup-test it, and publish what they decoded.
//
// Correctness never depends on memory ordering between workgroups or XCDs:
//   1. only truths are stored: an entry is written only for a key that decoded DEC_OK with the subgroup test passed;
//   2. slots are write-once: claim[slot] goes 0 -> fingerprint by one compare-and-swap, the winner alone writes the
//      entry, nothing is evicted or overwritten, and only hipbls_keycache_config zeroes the buffers again;
//   3. entries check themselves: a reader compares all 48 tag bytes and then a 64-bit check value over every word it
//      goes on to use.  A slot starts zeroed and each word is written once, so a torn or stale read can only show
//      zeros in place of final words, which the check value rejects.  Any mismatch is a miss, and a miss does what the
//      kernels did before the cache existed.
// So ordering and cache flavours move the hit rate, never a result.
//
// The pack/check part below is plain C++ (tests/test_keycache_host.py compiles it with g++); the probe and the insert
// are device code (serial stand-ins on a host build, where lanes run one by one).
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define KC_HD __host__ __device__ static __forceinline__
#else
#define KC_HD static inline
#endif

namespace bls {

// Entry: 64 words, 256-byte aligned (two cache lines that no other entry shares).
//   [0,12)  tag: the wire bytes as received (flags included: P and -P share x and differ here), little-endian words
//   [12,24) y, canonical Montgomery form (x is recomputed from the wire bytes)
//   [24,60) [x] pk, Jacobian, as g1_decompress_keep_x returns it
//   [60,62) check value over tag and y       (all a Verify reader uses)
//   [62,64) check value over tag and [x] pk  (the RLC readers verify both)
constexpr int KC_WORDS = 64;
constexpr int KC_TAG = 0, KC_Y = 12, KC_XPK = 24, KC_CHK_Y = 60, KC_CHK_X = 62;
constexpr int KC_WINDOW = 8;          // probe window: consecutive slots from the home slot
constexpr uint64_t KC_MIN_SLOTS = 8;  // so a window never visits a slot twice

// Passed to the kernels by value.  entries == nullptr: the cache is off.
struct keycache {
  uint32_t* entries;        // slots x KC_WORDS
  uint32_t* claim;          // slots: 0 = empty, else the owner's fingerprint
  unsigned long long* ctr;  // hits, misses, inserts
  uint32_t mask;            // slots - 1
  uint32_t pad_;
};

// One step of the check: for a fixed word the map h -> h' is a bijection (xor, odd multiplier, xor-shift), so zeroing
// ONE non-zero word always changes the final value; zeroing several changes it unless a 64-bit collision occurs.
KC_HD uint64_t kc_mix(uint64_t h, uint32_t w) {
  h = (h ^ w) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
KC_HD uint64_t kc_fold(uint64_t h, const uint32_t* w, int n) {
  for (int i = 0; i < n; ++i) h = kc_mix(h, w[i]);
  return h;
}
KC_HD void kc_tag_from_wire(uint32_t tag[12], const uint8_t* b48) {
  for (int k = 0; k < 12; ++k)
    tag[k] = (uint32_t)b48[4 * k] | ((uint32_t)b48[4 * k + 1] << 8) | ((uint32_t)b48[4 * k + 2] << 16) |
             ((uint32_t)b48[4 * k + 3] << 24);
}
KC_HD uint64_t kc_tag_hash(const uint32_t tag[12]) { return kc_fold(0x243F6A8885A308D3ull, tag, 12); }
KC_HD uint32_t kc_home(uint64_t tag_hash, uint32_t mask) { return (uint32_t)tag_hash & mask; }
KC_HD uint32_t kc_fingerprint(uint64_t tag_hash) {  // never 0: 0 is the empty claim
  const uint32_t f = (uint32_t)(tag_hash >> 32);
  return f ? f : 1u;
}
// A stored check value has both halves non-zero, so a check word read as zero never matches either.
KC_HD uint64_t kc_check_final(uint64_t h) {
  if (!(uint32_t)h) h |= 1ull;
  if (!(uint32_t)(h >> 32)) h |= 1ull << 32;
  return h;
}
KC_HD uint64_t kc_check_y(uint64_t tag_hash, const uint32_t y[12]) {
  return kc_check_final(kc_fold(tag_hash ^ 0x13198A2E03707344ull, y, 12));
}
KC_HD uint64_t kc_check_x(uint64_t tag_hash, const uint32_t xpk[36]) {
  return kc_check_final(kc_fold(tag_hash ^ 0xA4093822299F31D0ull, xpk, 36));
}

KC_HD void kc_pack(uint32_t e[KC_WORDS], const uint32_t tag[12], const uint32_t y[12], const uint32_t xpk[36]) {
  const uint64_t th = kc_tag_hash(tag);
  for (int k = 0; k < 12; ++k) e[KC_TAG + k] = tag[k];
  for (int k = 0; k < 12; ++k) e[KC_Y + k] = y[k];
  for (int k = 0; k < 36; ++k) e[KC_XPK + k] = xpk[k];
  const uint64_t cy = kc_check_y(th, y), cx = kc_check_x(th, xpk);
  e[KC_CHK_Y] = (uint32_t)cy;
  e[KC_CHK_Y + 1] = (uint32_t)(cy >> 32);
  e[KC_CHK_X] = (uint32_t)cx;
  e[KC_CHK_X + 1] = (uint32_t)(cx >> 32);
}

// Does this copy of an entry hold `tag`'s key?  On true y (and xpk, when asked for) are the packed values.  e is the
// reader's private copy of the words it uses: tag, y, the y check, and with xpk also [x] pk and its check.
KC_HD bool kc_entry_get(const uint32_t* e, const uint32_t tag[12], uint32_t y[12], uint32_t* xpk /* 36 or null */) {
  uint32_t diff = 0;
  for (int k = 0; k < 12; ++k) diff |= e[KC_TAG + k] ^ tag[k];
  if (diff) return false;  // an all-zero slot ends here: the compression flag makes tag word 0 non-zero
  const uint64_t th = kc_tag_hash(tag);
  const uint64_t cy = kc_check_y(th, e + KC_Y);
  if (e[KC_CHK_Y] != (uint32_t)cy || e[KC_CHK_Y + 1] != (uint32_t)(cy >> 32)) return false;
  if (xpk) {
    const uint64_t cx = kc_check_x(th, e + KC_XPK);
    if (e[KC_CHK_X] != (uint32_t)cx || e[KC_CHK_X + 1] != (uint32_t)(cx >> 32)) return false;
    for (int k = 0; k < 36; ++k) xpk[k] = e[KC_XPK + k];
  }
  for (int k = 0; k < 12; ++k) y[k] = e[KC_Y + k];
  return true;
}

// ---------------------------------------------------------------- probe and insert
#if defined(__HIP_DEVICE_COMPILE__)
// global address space: the loads, stores and the compare-and-swap are global_ forms, not flat_
typedef __attribute__((address_space(1))) uint32_t kc_gu32;
typedef __attribute__((address_space(1))) unsigned long long kc_gu64;
typedef __attribute__((address_space(1))) uint4 kc_gu128;
KC_HD uint32_t kc_cas_claim(uint32_t* p, uint32_t want) {  // returns the old value (0: this lane owns the slot)
  uint32_t old = 0;
  __hip_atomic_compare_exchange_strong((kc_gu32*)p, &old, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_AGENT);
  return old;
}
KC_HD uint32_t kc_load_claim(const uint32_t* p) { return *(const kc_gu32*)p; }
KC_HD void kc_load_words(uint32_t* dst, const uint32_t* src, int w0, int w1) {  // [w0, w1), multiples of 4
  const kc_gu128* s = (const kc_gu128*)__builtin_assume_aligned(src, 16);
  for (int k = w0 / 4; k < w1 / 4; ++k) {
    const uint4 v = s[k];
    dst[4 * k] = v.x, dst[4 * k + 1] = v.y, dst[4 * k + 2] = v.z, dst[4 * k + 3] = v.w;
  }
}
KC_HD void kc_store_entry(uint32_t* dst, const uint32_t* e) {
  kc_gu128* d = (kc_gu128*)__builtin_assume_aligned(dst, 16);
  for (int k = 0; k < KC_WORDS / 4; ++k) d[k] = make_uint4(e[4 * k], e[4 * k + 1], e[4 * k + 2], e[4 * k + 3]);
}
// hits / misses / inserts, once per wave: a ballot and a popcount per counter, one atomic from the first active lane
KC_HD void kc_count(const keycache& kc, bool hit, bool inserted) {
  const uint64_t act = __ballot(1), mh = __ballot(hit), mi = __ballot(inserted);
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane != (uint32_t)(__ffsll((unsigned long long)act) - 1)) return;
  kc_gu64* c = (kc_gu64*)kc.ctr;
  const unsigned long long nh = __popcll(mh), nm = __popcll(act & ~mh), ni = __popcll(mi);
  if (nh) __hip_atomic_fetch_add(c + 0, nh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (nm) __hip_atomic_fetch_add(c + 1, nm, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (ni) __hip_atomic_fetch_add(c + 2, ni, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
#else
KC_HD uint32_t kc_cas_claim(uint32_t* p, uint32_t want) {
  const uint32_t old = *p;
  if (!old) *p = want;
  return old;
}
KC_HD uint32_t kc_load_claim(const uint32_t* p) { return *p; }
KC_HD void kc_load_words(uint32_t* dst, const uint32_t* src, int w0, int w1) {
  for (int k = w0; k < w1; ++k) dst[k] = src[k];
}
KC_HD void kc_store_entry(uint32_t* dst, const uint32_t* e) {
  for (int k = 0; k < KC_WORDS; ++k) dst[k] = e[k];
}
KC_HD void kc_count(const keycache& kc, bool hit, bool inserted) {
  kc.ctr[hit ? 0 : 1] += 1;
  if (inserted) kc.ctr[2] += 1;
}
#endif

// Probe the window for `tag`: a plain load of claim decides per slot -- zero ends the probe as a miss, this key's
// fingerprint reads the entry and verifies it.  A stale zero only costs a hit.
KC_HD bool kc_lookup(const keycache& kc, const uint32_t tag[12], uint32_t y[12], uint32_t* xpk /* 36 or null */) {
  const uint64_t th = kc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th), home = kc_home(th, kc.mask);
  for (int k = 0; k < KC_WINDOW; ++k) {
    const uint32_t s = (home + (uint32_t)k) & kc.mask;
    const uint32_t c = kc_load_claim(kc.claim + s);
    if (!c) return false;
    if (c != fpr) continue;
    uint32_t e[KC_WORDS];
    const uint32_t* src = kc.entries + (uint64_t)s * KC_WORDS;
    kc_load_words(e, src, 0, 24);
    kc_load_words(e, src, 60, 64);
    if (xpk) kc_load_words(e, src, 24, 60);
    if (kc_entry_get(e, tag, y, xpk)) return true;
  }
  return false;
}

// Publish a key that just decoded DEC_OK.  The first empty slot of the window is claimed by compare-and-swap and the
// winner writes the entry with ordinary stores.  A lane that meets its own fingerprint stops: the key is there (or on
// its way), so the copies of one key in a cold batch do not fill the window with duplicates.  A full window: no
// caching.  Returns whether this lane wrote an entry.
KC_HD bool kc_insert(const keycache& kc, const uint32_t tag[12], const uint32_t y[12], const uint32_t xpk[36]) {
  const uint64_t th = kc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th), home = kc_home(th, kc.mask);
  for (int k = 0; k < KC_WINDOW; ++k) {
    const uint32_t s = (home + (uint32_t)k) & kc.mask;
    uint32_t c = kc_load_claim(kc.claim + s);
    if (!c) c = kc_cas_claim(kc.claim + s, fpr);  // a stale zero is settled here: the swap returns the truth
    if (c == fpr) return false;
    if (c) continue;
    uint32_t e[KC_WORDS];
    kc_pack(e, tag, y, xpk);
    kc_store_entry(kc.entries + (uint64_t)s * KC_WORDS, e);
    return true;
  }
  return false;
}

}  // namespace bls
