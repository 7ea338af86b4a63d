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
//   [58]    the root's line block (below): 0 = none, else its index in the line pool + 1.  Not under the check value:
//           packed as 0, written once per generation by the lane that filled the block, after the block
//   [59,64) unused, zero
constexpr int RC_WORDS = 64;
constexpr int RC_TAG = 0, RC_H = 8, RC_CHK = 56, RC_LINES = 58, RC_USED = 60;  // RC_USED: what a reader loads (a multiple of 4)
constexpr uint32_t RC_MSG_BYTES = 32;
constexpr uint32_t RC_NONE = 0xffffffffu;  // "no slot recorded" in k_root_lookup's pslot

// Passed to the kernels by value.  entries == nullptr: the cache is off.
struct rootcache {
  uint32_t* entries;        // slots x RC_WORDS
  uint32_t* claim;          // slots: 0 = empty, else the owner's fingerprint
  unsigned long long* ctr;  // hits, misses, inserts
  uint32_t mask;            // slots - 1
  uint32_t blocks;          // line pool: blocks of RL_BLOCK_WORDS words at `lines` (0: lines off)
  uint32_t* lines;
  unsigned long long* lctr;  // RL_CTR_*: blocks handed out, line hits, blocks published, pool full, check failures
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
// verifies it.  e_lines (when given) receives the found entry's RC_LINES word.
KC_HD uint32_t rc_find(const rootcache& rc, const uint32_t tag[8], uint32_t* e_lines = nullptr) {
  const uint64_t th = rc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, rc.mask);
    const uint32_t c = kc_load_claim(rc.claim + s);
    if (!c) return RC_NONE;
    if (c != fpr) continue;
    uint32_t e[RC_WORDS];
    kc_load_words(e, rc.entries + (uint64_t)s * RC_WORDS, 0, RC_USED);
    if (rc_entry_get(e, tag, nullptr)) {
      if (e_lines) *e_lines = e[RC_LINES];
      return s;
    }
  }
  return RC_NONE;
}

// A recorded slot's entry, loaded and verified over this reader's own copy (slot <= mask: k_root_lookup recorded it
// under the same struct; the mask is applied again so that no value of `slot` reads outside the table).
// e_lines (when given) receives the entry's RC_LINES word from the same copy.
KC_HD bool rc_get_slot(const rootcache& rc, uint32_t slot, const uint32_t tag[8], uint32_t h[48],
                       uint32_t* e_lines = nullptr) {
  uint32_t e[RC_WORDS];
  kc_load_words(e, rc.entries + (uint64_t)(slot & rc.mask) * RC_WORDS, 0, RC_USED);
  if (e_lines) *e_lines = e[RC_LINES];
  return rc_entry_get(e, tag, h);
}

// Publish the H(m) a lane just computed for `tag`'s bytes (keycache.h kc_insert's rules: first empty slot of the
// sequence by compare-and-swap, the winner writes, a lane that meets its own fingerprint stops, a full sequence
// publishes nothing).  Returns the slot this lane wrote, or RC_NONE.
KC_HD uint32_t rc_insert_slot(const rootcache& rc, const uint32_t tag[8], const uint32_t h[48]) {
  const uint64_t th = rc_tag_hash(tag);
  const uint32_t fpr = kc_fingerprint(th);
  for (int j = 0; j < RC_SEQ; ++j) {
    const uint32_t s = rc_seq_slot(th, j, rc.mask);
    uint32_t c = kc_load_claim(rc.claim + s);
    if (!c) c = kc_cas_claim(rc.claim + s, fpr);
    if (c == fpr) return RC_NONE;
    if (c) continue;
    uint32_t e[RC_WORDS];
    rc_pack(e, tag, h);
    kc_store_entry(rc.entries + (uint64_t)s * RC_WORDS, e);
    return s;
  }
  return RC_NONE;
}

KC_HD bool rc_insert(const rootcache& rc, const uint32_t tag[8], const uint32_t h[48]) {
  return rc_insert_slot(rc, tag, h) != RC_NONE;
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

// ---------------------------------------------------------------- line blocks
// In Verify's pair e(pk, H(m)) the G2 point the Miller loop walks starts at H(m), so its 63 doublings and 5 additions,
// and each line's three Fp2 coefficients before they are scaled by pk's coordinates, depend on the root alone.  A
// block holds those 68 lines in loop order -- the first doubling, the bit-62 addition, then bits 61..0 with the
// additions at bits 60, 57, 48 and 16 -- each as three Fp2 values of 24 words, exactly the canonical Montgomery words
// pairing.h's steps hold before their fp2_mul_fp:
//   doubling: g0 = 3b'Z^2 - Y^2, J3 = 3X^2, H = 2YZ        addition: g0 = theta x2 - lambda y2, theta, lambda
// and ends with a 64-bit check value over its words, seeded with the root's tag hash, both halves non-zero.  Blocks
// live in a pool beside the entry table, handed out by a device counter; the entry's word RC_LINES names the block.
// The three invariants hold here too: a lane records only the lines of the H(m) it holds for the bytes it tagged; a
// block is handed to one lane and an entry's RC_LINES is written once per generation, by that lane, after the block;
// a reader folds the check over the very words it feeds to the products and discards the loop's result on a mismatch.
// The pool is not zeroed when a generation ends: a block left from an earlier generation passes the check only under
// the seed of the root it was recorded for, and then it holds that root's true lines.
constexpr int RL_LINES = 68;
constexpr int RL_LINE_WORDS = 72;
constexpr int RL_CHK = RL_LINES * RL_LINE_WORDS;  // 4896: the check value's two words (at a multiple of 4)
constexpr int RL_BLOCK_WORDS = 4928;              // 77 x 256 bytes
static_assert(RL_CHK % 4 == 0 && RL_CHK + 4 <= RL_BLOCK_WORDS && RL_BLOCK_WORDS % 64 == 0, "line block layout");
enum { RL_CTR_NEXT = 0, RL_CTR_HITS, RL_CTR_PUBLISHED, RL_CTR_FULL, RL_CTR_BAD, RL_CTRS };

// What a Verify lane does about lines: replay a block, fill one, or neither (both null: today's loop).
struct rl_plan {
  const uint32_t* replay;
  uint32_t* record;
  uint32_t* entry_word;  // the entry's RC_LINES word, for the block being filled
  uint32_t index1;       // that block's index + 1
  uint64_t seed;         // the check's start value, bound to the root
  unsigned long long* lctr;  // the pool's counters, for the lane that replays or fills
};

KC_HD uint64_t rl_seed(uint64_t tag_hash) { return tag_hash ^ 0xC0AC29B7C97C50DDull; }
// The check's step takes two words at a time (kc_mix's map with a 64-bit input: still a bijection of h for a fixed
// pair, so one changed word always changes the value): half the multiplications of a word-by-word fold, which at one
// wave per SIMD is a chain of dependent instructions nothing else hides.
KC_HD uint64_t rl_mix2(uint64_t h, uint32_t lo, uint32_t hi) {
  h = (h ^ (((uint64_t)hi << 32) | lo)) * 0x9E3779B97F4A7C15ull;
  return h ^ (h >> 29);
}
KC_HD uint64_t rl_fold(uint64_t h, const uint32_t* w, int n) {  // n even
  for (int i = 0; i < n; i += 2) h = rl_mix2(h, w[i], w[i + 1]);
  return h;
}
// The check folds a line in the order the steps produce it: the second and third value, then g0.
KC_HD uint64_t rl_fold_line(uint64_t h, const uint32_t w[RL_LINE_WORDS]) {
  return rl_fold(rl_fold(h, w + 24, 48), w, 24);
}
KC_HD bool rl_check_ok(uint64_t h, uint32_t c0, uint32_t c1) {
  const uint64_t c = kc_check_final(h);
  return c0 == (uint32_t)c && c1 == (uint32_t)(c >> 32);
}
// A whole block in the reader's hands (host tests; the kernel folds line by line as it replays).
KC_HD bool rl_block_ok(const uint32_t* b, uint64_t seed) {
  uint64_t h = seed;
  for (int l = 0; l < RL_LINES; ++l) h = rl_fold_line(h, b + l * RL_LINE_WORDS);
  return rl_check_ok(h, b[RL_CHK], b[RL_CHK + 1]);
}

#if defined(__HIP_DEVICE_COMPILE__)
KC_HD void rl_load_line(uint32_t w[RL_LINE_WORDS], const uint32_t* src) { kc_load_words(w, src, 0, RL_LINE_WORDS); }
KC_HD void rl_load_check(uint32_t c[4], const uint32_t* blk) { kc_load_words(c, blk + RL_CHK, 0, 4); }
KC_HD void rl_store_words(uint32_t* dst, const uint32_t* v, int n) {  // n a multiple of 4, dst 16-byte aligned
  kc_gu128* d = (kc_gu128*)__builtin_assume_aligned(dst, 16);
  for (int k = 0; k < n / 4; ++k) d[k] = make_uint4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
}
KC_HD void rl_store_word(uint32_t* dst, uint32_t v) { *(kc_gu32*)dst = v; }
KC_HD unsigned long long rl_take_block(const rootcache& rc) {
  return __hip_atomic_fetch_add((kc_gu64*)rc.lctr + RL_CTR_NEXT, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
KC_HD void rl_count(unsigned long long* lctr, int which, bool flag) {
  const uint64_t act = __ballot(1), m = __ballot(flag);
  if (!m) return;
  const uint32_t lane = __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u));
  if (lane != (uint32_t)(__ffsll((unsigned long long)act) - 1)) return;
  __hip_atomic_fetch_add((kc_gu64*)lctr + which, (unsigned long long)__popcll(m), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_AGENT);
}
#else
KC_HD void rl_load_line(uint32_t w[RL_LINE_WORDS], const uint32_t* src) {
  for (int k = 0; k < RL_LINE_WORDS; ++k) w[k] = src[k];
}
KC_HD void rl_load_check(uint32_t c[4], const uint32_t* blk) {
  for (int k = 0; k < 4; ++k) c[k] = blk[RL_CHK + k];
}
KC_HD void rl_store_words(uint32_t* dst, const uint32_t* v, int n) {
  for (int k = 0; k < n; ++k) dst[k] = v[k];
}
KC_HD void rl_store_word(uint32_t* dst, uint32_t v) { *dst = v; }
KC_HD unsigned long long rl_take_block(const rootcache& rc) { return rc.lctr[RL_CTR_NEXT]++; }
KC_HD void rl_count(unsigned long long* lctr, int which, bool flag) {
  if (flag) lctr[which] += 1;
}
#endif

// Which loop a wave runs is decided for the wave: a wave that ran the replaying loop for some lanes and a full loop
// for others would run both one after the other (measured: a call of 65,536 items with 90 % of its roots warm took
// 42 ms that way against 30 ms with the lines off).  So a wave replays only if every lane of it that reaches the
// pairing has a block, and runs the recording loop -- with nothing to record on the other lanes -- if any lane fills one.
#if defined(__HIP_DEVICE_COMPILE__)
KC_HD bool rl_wave_all(bool flag) { return __ballot(flag) == __ballot(1); }
KC_HD bool rl_wave_any(bool flag) { return __ballot(flag) != 0; }
#else
KC_HD bool rl_wave_all(bool flag) { return flag; }
KC_HD bool rl_wave_any(bool flag) { return flag; }
#endif

// A hit's plan: e_lines is the entry's RC_LINES word from the reader's verified copy.  An index outside the pool is
// compared away here, before any load.
KC_HD void rl_plan_hit(rl_plan& plan, const rootcache& rc, uint32_t e_lines, uint64_t tag_hash) {
  if (!rc.lines || e_lines == 0 || e_lines - 1 >= rc.blocks) return;
  plan.replay = rc.lines + (uint64_t)(e_lines - 1) * RL_BLOCK_WORDS;
  plan.seed = rl_seed(tag_hash);
  plan.lctr = rc.lctr;
}
// The plan of the lane that just wrote `slot`'s entry: take the pool's next block, if one is left.
KC_HD void rl_plan_insert(rl_plan& plan, const rootcache& rc, uint32_t slot, uint64_t tag_hash) {
  if (!rc.lines) return;
  const unsigned long long b = rl_take_block(rc);
  if (b >= rc.blocks) return;
  plan.record = rc.lines + b * RL_BLOCK_WORDS;
  plan.entry_word = rc.entries + (uint64_t)(slot & rc.mask) * RC_WORDS + RC_LINES;
  plan.index1 = (uint32_t)b + 1;
  plan.seed = rl_seed(tag_hash);
  plan.lctr = rc.lctr;
}
// The recording lane's last step, after the loop: the check value, then the entry's word.
KC_HD void rl_publish(const rl_plan& plan, uint64_t h) {
  const uint64_t c = kc_check_final(h);
  const uint32_t tail[4] = {(uint32_t)c, (uint32_t)(c >> 32), 0, 0};
  rl_store_words(plan.record + RL_CHK, tail, 4);
  rl_store_word(plan.entry_word, plan.index1);
}

}  // namespace bls
