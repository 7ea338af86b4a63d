// Host program for the root cache's entry format (tests/test_rootcache_host.py): charon_amd/csrc/rootcache.h's pack
// and check functions, and its probe/insert on a host-side table (lanes one by one) through the wrapper the fused
// Verify kernel calls (rlc.h verify_hm_rc), with H(m) from the host build of the kernels' arithmetic.
// Exit status 0 = all passed.  Test-only; also built with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../charon_amd/csrc/ops.h"
#include "../../charon_amd/csrc/rlc.h"

using namespace bls;

#define CHECK(c)                                                  \
  do {                                                            \
    if (!(c)) {                                                   \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                   \
    }                                                             \
  } while (0)

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

static void hash_root(g2a& hm, const uint8_t* m32) {
  g2j hj;
  hash_to_g2(hj, m32, 32, DST_POP, 43);
  jac_to_aff(hm, hj);
}

static int entry_checks(const uint8_t* m32) {
  g2a hm;
  hash_root(hm, m32);
  const uint32_t* h = &hm.x.c0.v[0];
  uint32_t tag[8], e[RC_WORDS], got[48];
  rc_tag_from_msg(tag, m32);
  rc_pack(e, tag, h);
  CHECK(e[RC_CHK] != 0 && e[RC_CHK + 1] != 0);
  for (int w = RC_CHK + 2; w < RC_WORDS; ++w) CHECK(e[w] == 0);

  // pack and get round-trip
  memset(got, 0, sizeof(got));
  CHECK(rc_entry_get(e, tag, got));
  CHECK(!memcmp(got, h, sizeof(got)));
  CHECK(rc_entry_get(e, tag, nullptr));

  // an all-zero slot matches no message, the all-zero message included
  uint32_t zero[RC_WORDS] = {}, ztag[8] = {};
  CHECK(!rc_entry_get(zero, tag, got));
  CHECK(!rc_entry_get(zero, ztag, got));
  CHECK(!rc_entry_get(zero, ztag, nullptr));

  // a tag differing in one bit, every bit in turn
  for (int bit = 0; bit < 256; ++bit) {
    uint8_t m[32];
    memcpy(m, m32, 32);
    m[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    uint32_t t2[8];
    rc_tag_from_msg(t2, m);
    CHECK(!rc_entry_get(e, t2, got));
  }

  // every non-zero word zeroed in turn
  int nonzero = 0;
  for (int w = 0; w < RC_WORDS; ++w) {
    if (!e[w]) continue;
    ++nonzero;
    uint32_t t[RC_WORDS];
    memcpy(t, e, sizeof(t));
    t[w] = 0;
    CHECK(!rc_entry_get(t, tag, got));
  }
  CHECK(nonzero >= 50);

  // a seeded sample of subsets of the non-zero words zeroed (what a torn or stale read can show)
  for (int trial = 0; trial < 20000; ++trial) {
    uint32_t t[RC_WORDS];
    memcpy(t, e, sizeof(t));
    const uint64_t m = trial % 3 == 0 ? rnd() & rnd() & rnd() : (trial % 3 == 1 ? rnd() : rnd() | rnd());
    bool any = false;
    for (int w = 0; w < RC_WORDS; ++w)
      if (((m >> w) & 1) && e[w]) {
        t[w] = 0;
        any = true;
      }
    if (!any) continue;
    CHECK(!rc_entry_get(t, tag, got));
  }
  // whole cache lines missing: the first or the second 128 bytes still zero
  for (int half = 0; half < 2; ++half) {
    uint32_t t[RC_WORDS];
    memcpy(t, e, sizeof(t));
    memset(t + 32 * half, 0, 32 * sizeof(uint32_t));
    CHECK(!rc_entry_get(t, tag, got));
  }
  return 0;
}

static int table_checks(const std::vector<std::vector<uint8_t>>& roots) {
  const uint32_t slots = 8;  // one probe window: the table is the window
  std::vector<uint32_t> entries(slots * RC_WORDS, 0), claim(slots, 0);
  unsigned long long ctr[3] = {0, 0, 0};
  rootcache rc{};
  rc.entries = entries.data();
  rc.claim = claim.data();
  rc.ctr = ctr;
  rc.mask = slots - 1;
  const uint8_t* r0 = roots[0].data();
  uint32_t tag0[8];
  rc_tag_from_msg(tag0, r0);
  g2a want, a;
  hash_root(want, r0);

  // cold: nothing found, hashed and published once
  CHECK(rc_find(rc, tag0) == RC_NONE);
  verify_hm_rc(a, r0, 32, rc, RC_NONE);
  CHECK(ctr[2] == 1 && !memcmp(&a, &want, sizeof(a)));
  const uint32_t s0 = rc_find(rc, tag0);
  CHECK(s0 != RC_NONE && s0 < slots);
  // warm, through the recorded slot: H from the entry, nothing published
  memset(&a, 0, sizeof(a));
  verify_hm_rc(a, r0, 32, rc, s0);
  CHECK(ctr[2] == 1 && !memcmp(&a, &want, sizeof(a)));
  // the same root hashed again without a recorded slot (a racing lane): its own fingerprint stops the insert
  verify_hm_rc(a, r0, 32, rc, RC_NONE);
  CHECK(ctr[2] == 1 && !memcmp(&a, &want, sizeof(a)));

  // a recorded slot that holds another root (a stale slot) is a miss: the message is hashed
  g2a w1, b;
  hash_root(w1, roots[1].data());
  verify_hm_rc(b, roots[1].data(), 32, rc, s0);
  CHECK(!memcmp(&b, &w1, sizeof(b)) && memcmp(&b, &want, sizeof(b)) && ctr[2] == 2);
  // a slot index beyond the table reads inside it (masked) and misses
  verify_hm_rc(b, roots[1].data(), 32, rc, 0x7fffffffu);
  CHECK(!memcmp(&b, &w1, sizeof(b)) && ctr[2] == 2);

  // other lengths bypass the cache: hashed, never published, never served
  uint8_t longer[33];
  memcpy(longer, r0, 32);
  longer[32] = 0;
  g2a l0, l1;
  {
    g2j hj;
    hash_to_g2(hj, longer, 33, DST_POP, 43);
    jac_to_aff(l0, hj);
  }
  verify_hm_rc(l1, longer, 33, rc, s0);
  CHECK(!memcmp(&l0, &l1, sizeof(l0)) && ctr[2] == 2);
  verify_hm_rc(l1, longer, 31, rc, s0);
  CHECK(ctr[2] == 2);

  // more roots than slots: the window fills, then nothing is published and nothing is overwritten
  for (int rep = 0; rep < 2; ++rep)
    for (const auto& r : roots) {
      g2a p, q;
      hash_root(p, r.data());
      uint32_t t[8];
      rc_tag_from_msg(t, r.data());
      verify_hm_rc(q, r.data(), 32, rc, rc_find(rc, t));
      CHECK(!memcmp(&p, &q, sizeof(p)));
    }
  CHECK(ctr[2] == slots);
  int claimed = 0;
  for (uint32_t s = 0; s < slots; ++s) claimed += claim[s] != 0;
  CHECK(claimed == (int)slots);
  const std::vector<uint32_t> full = entries;
  {
    uint8_t fresh[32];
    memset(fresh, 0xA5, 32);
    uint32_t t[8];
    rc_tag_from_msg(t, fresh);
    CHECK(rc_find(rc, t) == RC_NONE);
    g2a q;
    verify_hm_rc(q, fresh, 32, rc, RC_NONE);
    CHECK(ctr[2] == slots && entries == full);  // a full window publishes nothing
  }
  CHECK(rc_find(rc, tag0) == s0);  // the first entry is still there

  // the cache off: the plain hash
  rootcache off{};
  verify_hm_rc(a, r0, 32, off, RC_NONE);
  CHECK(!memcmp(&a, &want, sizeof(a)));
  return 0;
}

int main() {
  std::vector<std::vector<uint8_t>> roots;
  for (int i = 0; i < 12; ++i) {
    std::vector<uint8_t> r(32);
    for (auto& b : r) b = (uint8_t)rnd();
    roots.push_back(r);
  }
  roots.push_back(std::vector<uint8_t>(32, 0));  // the all-zero root is a root like any other
  for (size_t i = 0; i < 3; ++i)
    if (entry_checks(roots[i].data())) return 1;
  if (entry_checks(roots.back().data())) return 1;
  if (table_checks(roots)) return 1;
  printf("rootcache_host ok: %zu roots\n", roots.size());
  return 0;
}
