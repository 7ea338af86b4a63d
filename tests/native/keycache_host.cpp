// Host program for the key cache's entry format (tests/test_keycache_host.py): charon_amd/csrc/keycache.h's pack and
// check functions, and its probe/insert on a host-side table (lanes one by one), with a real key decoded by the host
// build of the kernels' arithmetic.  argv: one or more valid 48-byte public keys in hex.  Exit status 0 = all passed.
// Test-only; also built with -fsanitize=address,undefined.
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

static bool unhex48(uint8_t* out, const char* s) {
  if (strlen(s) != 96) return false;
  for (int i = 0; i < 48; ++i) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

// which words each reader uses
static bool in_y_part(int w) { return w < KC_XPK || (w >= KC_CHK_Y && w < KC_CHK_X); }

static int entry_checks(const uint8_t* pk48) {
  g1a pk;
  g1j xpk;
  CHECK(g1_decompress_keep_x(pk, xpk, pk48) == DEC_OK);
  uint32_t tag[12], e[KC_WORDS];
  kc_tag_from_wire(tag, pk48);
  CHECK(tag[0] != 0);  // the compression flag
  kc_pack(e, tag, pk.y.v, &xpk.x.v[0]);
  for (int h = KC_CHK_Y; h < KC_WORDS; ++h) CHECK(e[h] != 0);

  // the untouched entry passes, for both readers, and hands back what was packed
  uint32_t y[12], x36[36];
  CHECK(kc_entry_get(e, tag, y, nullptr));
  CHECK(!memcmp(y, pk.y.v, sizeof(y)));
  memset(y, 0, sizeof(y));
  CHECK(kc_entry_get(e, tag, y, x36));
  CHECK(!memcmp(y, pk.y.v, sizeof(y)) && !memcmp(x36, &xpk.x.v[0], sizeof(x36)));

  // an all-zero slot matches no key
  uint32_t zero[KC_WORDS] = {};
  CHECK(!kc_entry_get(zero, tag, y, nullptr));
  CHECK(!kc_entry_get(zero, tag, y, x36));

  // the same x with the other sign flag is another key
  uint8_t neg[48];
  memcpy(neg, pk48, 48);
  neg[0] ^= 0x20;
  uint32_t ntag[12];
  kc_tag_from_wire(ntag, neg);
  CHECK(!kc_entry_get(e, ntag, y, nullptr));

  // every non-zero word zeroed in turn: the reader that uses the word rejects the entry; a reader that does not use
  // it still returns the packed values
  int nonzero = 0;
  for (int w = 0; w < KC_WORDS; ++w) {
    if (!e[w]) continue;
    ++nonzero;
    uint32_t t[KC_WORDS];
    memcpy(t, e, sizeof(t));
    t[w] = 0;
    CHECK(!kc_entry_get(t, tag, y, x36));
    if (in_y_part(w)) {
      CHECK(!kc_entry_get(t, tag, y, nullptr));
    } else {
      CHECK(kc_entry_get(t, tag, y, nullptr));
      CHECK(!memcmp(y, pk.y.v, sizeof(y)));
    }
  }
  CHECK(nonzero >= 60);

  // random subsets of the non-zero words zeroed (what a torn or stale read can show)
  for (int trial = 0; trial < 20000; ++trial) {
    uint32_t t[KC_WORDS];
    memcpy(t, e, sizeof(t));
    const uint64_t m = trial % 3 == 0 ? rnd() & rnd() & rnd() : (trial % 3 == 1 ? rnd() : rnd() | rnd());
    bool any = false, any_y = false;
    for (int w = 0; w < KC_WORDS; ++w)
      if (((m >> w) & 1) && e[w]) {
        t[w] = 0;
        any = true;
        any_y = any_y || in_y_part(w);
      }
    if (!any) continue;
    CHECK(!kc_entry_get(t, tag, y, x36));
    if (any_y) CHECK(!kc_entry_get(t, tag, y, nullptr));
  }
  // whole cache lines missing: the first or the second 128 bytes still zero
  for (int half = 0; half < 2; ++half) {
    uint32_t t[KC_WORDS];
    memcpy(t, e, sizeof(t));
    memset(t + 32 * half, 0, 32 * sizeof(uint32_t));
    CHECK(!kc_entry_get(t, tag, y, x36));
    CHECK(!kc_entry_get(t, tag, y, nullptr));
  }
  return 0;
}

// probe and insert on a host table, through the same decode wrapper the kernels call
static int table_checks(const std::vector<std::vector<uint8_t>>& keys) {
  const uint32_t slots = 8;
  std::vector<uint32_t> entries(slots * KC_WORDS, 0), claim(slots, 0);
  unsigned long long ctr[3] = {0, 0, 0};
  keycache kc{};
  kc.entries = entries.data();
  kc.claim = claim.data();
  kc.ctr = ctr;
  kc.mask = slots - 1;
  const uint8_t* k0 = keys[0].data();
  g1a a, b;
  g1j xa, xb;
  CHECK(g1_decompress_keep_x(a, xa, k0) == DEC_OK);
  CHECK(g1_decode_kc_x(b, xb, k0, kc) == DEC_OK);  // cold: decoded and published
  CHECK(ctr[0] == 0 && ctr[1] == 1 && ctr[2] == 1);
  CHECK(!memcmp(&a, &b, sizeof(a)) && !memcmp(&xa, &xb, sizeof(xa)));
  memset(&b, 0, sizeof(b));
  memset(&xb, 0, sizeof(xb));
  CHECK(g1_decode_kc_x(b, xb, k0, kc) == DEC_OK);  // warm: x from the wire bytes, y and [x] pk from the entry
  CHECK(ctr[0] == 1 && ctr[1] == 1 && ctr[2] == 1);
  CHECK(!memcmp(&a, &b, sizeof(a)) && !memcmp(&xa, &xb, sizeof(xa)));
  memset(&b, 0, sizeof(b));
  CHECK(g1_decode_kc_pk(b, k0, kc) == DEC_OK);  // the Verify reader
  CHECK(ctr[0] == 2 && !memcmp(&a, &b, sizeof(a)));

  // -P: the same x, another key, another entry
  uint8_t neg[48];
  memcpy(neg, k0, 48);
  neg[0] ^= 0x20;
  g1a n;
  CHECK(g1_decode_kc_pk(n, neg, kc) == DEC_OK);
  CHECK(ctr[2] == 2);
  CHECK(!memcmp(&n.x, &a.x, sizeof(a.x)) && memcmp(&n.y, &a.y, sizeof(a.y)));
  CHECK(g1_decode_kc_pk(b, neg, kc) == DEC_OK && !memcmp(&n, &b, sizeof(n)));
  CHECK(ctr[2] == 2 && ctr[0] == 3);

  // invalid keys are never entries: infinity, missing compression flag, x >= p (all ones under the flag mask)
  uint8_t inf[48] = {0xc0}, noflag[48], big[48];
  memcpy(noflag, k0, 48);
  noflag[0] &= 0x7f;
  memset(big, 0xff, 48);
  big[0] = 0x9f;
  const unsigned long long ins = ctr[2];
  for (int rep = 0; rep < 2; ++rep) {
    CHECK(g1_decode_kc_pk(b, inf, kc) == DEC_INF);
    CHECK(g1_decode_kc_pk(b, noflag, kc) == DEC_BAD);
    CHECK(g1_decode_kc_pk(b, big, kc) == DEC_BAD);
  }
  CHECK(ctr[2] == ins);

  // more keys than slots: at most `slots` inserts, results as without the cache, nothing overwritten
  for (int rep = 0; rep < 2; ++rep)
    for (const auto& k : keys) {
      g1a p, q;
      g1j xp, xq;
      CHECK(g1_decompress_keep_x(p, xp, k.data()) == DEC_OK);
      CHECK(g1_decode_kc_x(q, xq, k.data(), kc) == DEC_OK);
      CHECK(!memcmp(&p, &q, sizeof(p)) && !memcmp(&xp, &xq, sizeof(xp)));
    }
  CHECK(ctr[2] <= slots);
  int claimed = 0;
  for (uint32_t s = 0; s < slots; ++s) claimed += claim[s] != 0;
  CHECK((unsigned long long)claimed == ctr[2]);
  CHECK(g1_decode_kc_pk(b, k0, kc) == DEC_OK && !memcmp(&a, &b, sizeof(a)));  // the first entry is still there

  // the cache off: the plain decode
  keycache off{};
  CHECK(g1_decode_kc_pk(b, k0, off) == DEC_OK && !memcmp(&a, &b, sizeof(a)));
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    fprintf(stderr, "usage: keycache_host <pk hex> [<pk hex> ...]\n");
    return 2;
  }
  std::vector<std::vector<uint8_t>> keys;
  for (int i = 1; i < argc; ++i) {
    std::vector<uint8_t> k(48);
    if (!unhex48(k.data(), argv[i])) {
      fprintf(stderr, "bad key hex: %s\n", argv[i]);
      return 2;
    }
    keys.push_back(k);
  }
  for (const auto& k : keys)
    if (entry_checks(k.data())) return 1;
  if (table_checks(keys)) return 1;
  printf("keycache_host ok: %zu keys\n", keys.size());
  return 0;
}
