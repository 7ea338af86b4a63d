// Host program for the signature cache (tests/test_sigcache_host.py): charon_amd/csrc/sigcache.h's pack and check
// functions, its probe / insert rules on a host-side table (lanes one by one), the generation threshold, the RLC
// producer's rule, and sigagg's scaling lane (rlc.h tagg_scale_partial_sc) on its hit path against its miss path, on
// partials signed by the oracle.  Argument: a text file of groups,
//     G <t>            then t lines   P <id> <96-byte signature, hex>   then   A <96-byte aggregate, hex>
// Prints the host work counter's Fp products and squarings per partial on both paths.
// Exit status 0 = all passed.  Test-only; also built with -fsanitize=address,undefined.
#define BLS_COUNT_OPS 1
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../charon_amd/csrc/ops.h"
#include "../../charon_amd/csrc/rlc.h"

namespace bls {
thread_local uint64_t g_fp_mul_count = 0;
thread_local uint64_t g_fp_sqr_count = 0;
}  // namespace bls
using namespace bls;

#define CHECK(c)                                                      \
  do {                                                                \
    if (!(c)) {                                                       \
      fprintf(stderr, "%s:%d: failed: %s\n", __FILE__, __LINE__, #c); \
      return 1;                                                       \
    }                                                                 \
  } while (0)

struct Group {
  std::vector<int64_t> ids;
  std::vector<uint8_t> sigs;  // 96 t
  uint8_t agg[96];
};

static bool unhex(uint8_t* out, const char* s, size_t n) {
  if (strlen(s) != 2 * n) return false;
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    if (sscanf(s + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

static bool read_groups(const char* path, std::vector<Group>& gs) {
  FILE* f = fopen(path, "r");
  if (!f) return false;
  char kind[4], hex[256];
  long long a;
  bool ok = true;
  while (ok && fscanf(f, "%3s", kind) == 1) {
    if (kind[0] == 'G') {
      ok = fscanf(f, "%lld", &a) == 1;
      gs.emplace_back();
    } else if (kind[0] == 'P' && !gs.empty()) {
      uint8_t s[96];
      ok = fscanf(f, "%lld %255s", &a, hex) == 2 && unhex(s, hex, 96);
      gs.back().ids.push_back((int64_t)a);
      gs.back().sigs.insert(gs.back().sigs.end(), s, s + 96);
    } else if (kind[0] == 'A' && !gs.empty()) {
      ok = fscanf(f, "%255s", hex) == 1 && unhex(gs.back().agg, hex, 96);
    } else {
      ok = false;
    }
  }
  fclose(f);
  return ok && !gs.empty();
}

struct Table {
  std::vector<uint32_t> entries, claim;
  unsigned long long ctr[3] = {0, 0, 0};
  sigcache sc{};
  explicit Table(uint32_t slots) : entries((size_t)slots * SC_WORDS, 0), claim(slots, 0) {
    sc.entries = entries.data();
    sc.claim = claim.data();
    sc.ctr = ctr;
    sc.mask = slots - 1;
  }
};

static int entry_checks(const uint8_t* sig96) {
  g2a s;
  CHECK(g2_decompress(s, sig96, true) == DEC_OK);
  const uint32_t* y = &s.y.c0.v[0];
  uint32_t tag[24], e[SC_WORDS], got[24];
  sc_tag_from_wire(tag, sig96);
  sc_pack(e, tag, y);
  CHECK(e[SC_CHK] != 0 && e[SC_CHK + 1] != 0);
  for (int w = SC_CHK + 2; w < SC_WORDS; ++w) CHECK(e[w] == 0);
  static_assert(SC_USED % 4 == 0 && SC_USED >= SC_CHK + 2 && SC_USED <= SC_WORDS, "what a reader loads");

  // pack and get round-trip; x comes back from the wire bytes
  memset(got, 0, sizeof(got));
  CHECK(sc_entry_get(e, tag, got));
  CHECK(!memcmp(got, y, sizeof(got)));
  fp2 x;
  g2_x_from_wire(x, sig96);
  CHECK(fp2_eq(x, s.x));

  // an all-zero slot matches no tag, the all-zero tag included
  uint32_t zero[SC_WORDS] = {}, ztag[24] = {};
  CHECK(!sc_entry_get(zero, tag, got));
  CHECK(!sc_entry_get(zero, ztag, got));

  // a tag differing in one bit, every bit in turn
  for (int bit = 0; bit < 768; ++bit) {
    uint8_t m[96];
    memcpy(m, sig96, 96);
    m[bit / 8] ^= (uint8_t)(1u << (bit % 8));
    uint32_t t2[24];
    sc_tag_from_wire(t2, m);
    CHECK(!sc_entry_get(e, t2, got));
  }

  // every single word of the entry zeroed in turn
  int nonzero = 0;
  for (int w = 0; w < SC_WORDS; ++w) {
    if (!e[w]) continue;
    ++nonzero;
    uint32_t t[SC_WORDS];
    memcpy(t, e, sizeof(t));
    t[w] = 0;
    CHECK(!sc_entry_get(t, tag, got));
  }
  CHECK(nonzero >= 44);
  // whole cache lines missing: the first or the second 128 bytes still zero
  for (int half = 0; half < 2; ++half) {
    uint32_t t[SC_WORDS];
    memcpy(t, e, sizeof(t));
    memset(t + 32 * half, 0, 32 * sizeof(uint32_t));
    CHECK(!sc_entry_get(t, tag, got));
  }
  return 0;
}

static int table_checks(const std::vector<const uint8_t*>& sigs) {
  const uint8_t* s0 = sigs[0];
  g2a a0;
  CHECK(g2_decompress(a0, s0, true) == DEC_OK);
  uint32_t tag0[24], y[24];
  sc_tag_from_wire(tag0, s0);
  const uint64_t th0 = sc_tag_hash(tag0);

  {  // first empty slot of the sequence; own fingerprint stops; the sign twin is an entry of its own
    Table T(64);
    CHECK(!sc_lookup(T.sc, tag0, y));
    const int taken = 11;  // the sequence's first 11 slots belong to others: past the first window
    uint32_t other = kc_fingerprint(th0) + 1;  // another signature's fingerprint
    if (!other) other = 2;
    for (int j = 0; j < taken; ++j) T.claim[rc_seq_slot(th0, j, T.sc.mask)] = other;
    uint32_t expect = 0;
    for (int j = 0; j < RC_SEQ; ++j) {
      expect = rc_seq_slot(th0, j, T.sc.mask);
      if (!T.claim[expect]) break;
    }
    sig_publish(T.sc, s0, a0);
    CHECK(T.ctr[2] == 1 && T.claim[expect] == kc_fingerprint(th0));
    CHECK(sc_lookup(T.sc, tag0, y) && !memcmp(y, &a0.y.c0.v[0], sizeof(y)));
    const std::vector<uint32_t> before = T.entries;
    sig_publish(T.sc, s0, a0);  // the same signature again: its own fingerprint stops the insert
    CHECK(T.ctr[2] == 1 && T.entries == before);

    // same x, the other sign flag: -S, another 96 bytes, another entry
    uint8_t twin[96];
    memcpy(twin, s0, 96);
    twin[0] ^= 0x20;
    g2a at;
    CHECK(g2_decompress(at, twin, true) == DEC_OK);
    CHECK(fp2_eq(at.x, a0.x) && !fp2_eq(at.y, a0.y));
    uint32_t ttag[24], ty[24];
    sc_tag_from_wire(ttag, twin);
    CHECK(!sc_lookup(T.sc, ttag, ty));
    sig_publish(T.sc, twin, at);
    CHECK(T.ctr[2] == 2);
    CHECK(sc_lookup(T.sc, ttag, ty) && !memcmp(ty, &at.y.c0.v[0], sizeof(ty)));
    CHECK(sc_lookup(T.sc, tag0, y) && !memcmp(y, &a0.y.c0.v[0], sizeof(y)));
  }
  {  // a full sequence: not cached, nothing overwritten
    Table T(8);
    for (auto& c : T.claim) c = 0x12345u;
    const std::vector<uint32_t> before = T.entries;
    sig_publish(T.sc, s0, a0);
    CHECK(T.ctr[2] == 0 && T.entries == before && !sc_lookup(T.sc, tag0, y));
  }
  {  // more signatures than slots: at most `slots` inserts, every stored one still found and true
    Table T(8);
    for (int rep = 0; rep < 2; ++rep)
      for (const uint8_t* s : sigs) {
        g2a a;
        CHECK(g2_decompress(a, s, true) == DEC_OK);
        sig_publish(T.sc, s, a);
      }
    CHECK(T.ctr[2] <= 8 && T.ctr[2] >= 1);
    unsigned found = 0;
    for (const uint8_t* s : sigs) {
      g2a a;
      CHECK(g2_decompress(a, s, true) == DEC_OK);
      uint32_t t[24], yy[24];
      sc_tag_from_wire(t, s);
      if (sc_lookup(T.sc, t, yy)) {
        ++found;
        CHECK(!memcmp(yy, &a.y.c0.v[0], sizeof(yy)));
      }
    }
    CHECK(found == T.ctr[2]);
  }
  // the generation threshold: half the slots, counted from the generation's start; an empty table is never due
  CHECK(!sc_generation_due(3, 0, 8) && sc_generation_due(4, 0, 8) && sc_generation_due(9, 0, 8));
  CHECK(!sc_generation_due(103, 100, 8) && sc_generation_due(104, 100, 8));
  CHECK(!sc_generation_due(1000, 0, 0));
  CHECK(!sc_generation_due(131071, 0, 262144) && sc_generation_due(131072, 0, 262144));
  return 0;
}

// The RLC item stage's rule (rlc.h rlc_item_decoded_sc): a signature that decodes DEC_OK with the subgroup test is
// published, anything else never.
static int producer_checks(const uint8_t* sig96) {
  Table T(64);
  g1a pk;
  pk.x = G1_GEN_X;
  pk.y = G1_GEN_Y;
  g1j xpk;
  jac_from_aff(xpk, pk);
  rlc_seed seed{};
  uint32_t rp[36], rs[72];
  uint8_t bad[96];
  memcpy(bad, sig96, 96);
  bad[95] ^= 1;  // a flipped bit: off the curve or outside G2
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, bad, seed, 0, rp, rs, T.sc) == HIPBLS_ERR_SIGNATURE && T.ctr[2] == 0);
  uint8_t inf[96] = {0xc0};
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, inf, seed, 0, rp, rs, T.sc) == HIPBLS_ERR_VERIFY && T.ctr[2] == 0);
  memcpy(bad, sig96, 96);
  bad[0] &= 0x7f;  // the compression flag cleared
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, bad, seed, 0, rp, rs, T.sc) == HIPBLS_ERR_SIGNATURE && T.ctr[2] == 0);
  memcpy(bad, sig96, 96);
  bad[0] |= 0x40;  // the infinity flag with an x
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, bad, seed, 0, rp, rs, T.sc) == HIPBLS_ERR_SIGNATURE && T.ctr[2] == 0);
  memset(bad, 0xff, 96);
  bad[0] = 0x9f;  // x >= p
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, bad, seed, 0, rp, rs, T.sc) == HIPBLS_ERR_SIGNATURE && T.ctr[2] == 0);
  for (const auto c : T.claim) CHECK(c == 0);
  uint32_t rs0[72];
  CHECK(rlc_item_decoded_sc(DEC_OK, pk, xpk, sig96, seed, 0, rp, rs, T.sc) == RLC_PENDING && T.ctr[2] == 1);
  CHECK(rlc_item_decoded(DEC_OK, pk, xpk, sig96, seed, 0, rp, rs0) == RLC_PENDING && !memcmp(rs, rs0, sizeof(rs)));
  return 0;
}

struct Ops {
  uint64_t mul = 0, sqr = 0, parts = 0;
};

// Hit path against miss path of the scaling lane for one group, and both sums against the oracle's aggregate.
static int group_checks(const Group& g, Ops& miss_ops, Ops& hit_ops, bool expect_small) {
  const int t = (int)g.ids.size();
  Table T(256);
  sigcache off{};
  int64_t c;
  uint64_t L;
  CHECK(lagrange_small(g.ids.data(), t, 0, c, L) == expect_small);
  g2j sum_miss, sum_hit;
  jac_set_inf(sum_miss);
  jac_set_inf(sum_hit);
  bool negative = false;
  for (int k = 0; k < t; ++k) {
    const uint8_t* s = g.sigs.data() + 96 * k;
    if (expect_small && lagrange_small(g.ids.data(), t, k, c, L) && c < 0) negative = true;
    g2j am, ah, ac;
    uint64_t m0 = g_fp_mul_count, q0 = g_fp_sqr_count;
    CHECK(tagg_scale_partial_sc(am, s, g.ids.data(), t, k, HIPBLS_OK, off) == DEC_OK);
    miss_ops.mul += g_fp_mul_count - m0, miss_ops.sqr += g_fp_sqr_count - q0, miss_ops.parts += 1;
    // cold, cache on: a miss, the same words as with the cache off, and sigagg never fills the cache
    CHECK(tagg_scale_partial_sc(ac, s, g.ids.data(), t, k, HIPBLS_OK, T.sc) == DEC_OK);
    CHECK(!memcmp(&ac, &am, sizeof(ac)) && T.ctr[2] == (unsigned long long)k && T.ctr[1] == (unsigned long long)k + 1);
    g2a a;
    CHECK(g2_decompress(a, s, true) == DEC_OK);
    sig_publish(T.sc, s, a);
    m0 = g_fp_mul_count, q0 = g_fp_sqr_count;
    CHECK(tagg_scale_partial_sc(ah, s, g.ids.data(), t, k, HIPBLS_OK, T.sc) == DEC_OK);
    hit_ops.mul += g_fp_mul_count - m0, hit_ops.sqr += g_fp_sqr_count - q0, hit_ops.parts += 1;
    CHECK(T.ctr[0] == 2ull * k + 1);  // one hit here and one in the ERR_COMBINE call below, per partial
    // the same group element, whatever the Jacobian words
    CHECK(jac_eq(am, ah));
    uint8_t bm[96], bh[96];
    g2_compress(bm, am);
    g2_compress(bh, ah);
    CHECK(!memcmp(bm, bh, 96));
    g2a fm, fh;
    jac_to_aff(fm, am);
    jac_to_aff(fh, ah);
    CHECK(fp2_eq(fm.x, fh.x) && fp2_eq(fm.y, fh.y));
    g2j x = sum_miss;
    jac_add(sum_miss, x, am);
    x = sum_hit;
    jac_add(sum_hit, x, ah);
    // an id check that failed (ERR_COMBINE) scales nothing on either path
    CHECK(tagg_scale_partial_sc(ah, s, g.ids.data(), t, k, HIPBLS_ERR_COMBINE, T.sc) == DEC_OK && jac_is_inf(ah));
    CHECK(tagg_scale_partial_sc(am, s, g.ids.data(), t, k, HIPBLS_ERR_COMBINE, off) == DEC_OK && jac_is_inf(am));
  }
  if (expect_small && t >= 4) CHECK(negative);
  tagg_unscale(sum_miss, g.ids.data(), t);
  tagg_unscale(sum_hit, g.ids.data(), t);
  uint8_t om[96], oh[96], ref[96];
  g2_compress(om, sum_miss);
  g2_compress(oh, sum_hit);
  CHECK(!memcmp(om, g.agg, 96) && !memcmp(oh, g.agg, 96));
  CHECK(op_threshold_aggregate(ref, g.sigs.data(), g.ids.data(), t) == HIPBLS_OK && !memcmp(ref, g.agg, 96));
  return 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: sigcache_host <groups file>\n");
    return 2;
  }
  std::vector<Group> gs;
  if (!read_groups(argv[1], gs)) {
    fprintf(stderr, "bad groups file\n");
    return 2;
  }
  std::vector<const uint8_t*> sigs;
  for (const Group& g : gs)
    for (size_t k = 0; k < g.ids.size(); ++k) sigs.push_back(g.sigs.data() + 96 * k);
  CHECK(sigs.size() >= 12);
  for (int i = 0; i < 2; ++i)
    if (entry_checks(sigs[i])) return 1;
  if (table_checks(sigs)) return 1;
  if (producer_checks(sigs[0])) return 1;
  Ops ms, hs, mf, hf;
  size_t small_groups = 0, field_groups = 0;
  for (const Group& g : gs) {
    bool small = true;
    for (int64_t id : g.ids) small = small && id <= (1 << 20) && id >= -(1 << 20);
    if (group_checks(g, small ? ms : mf, small ? hs : hf, small)) return 1;
    (small ? small_groups : field_groups) += 1;
  }
  CHECK(small_groups >= 2 && field_groups >= 1);
  printf("ops small miss: %.1f mul %.1f sqr per partial\n", (double)ms.mul / ms.parts, (double)ms.sqr / ms.parts);
  printf("ops small hit: %.1f mul %.1f sqr per partial\n", (double)hs.mul / hs.parts, (double)hs.sqr / hs.parts);
  printf("ops field miss: %.1f mul %.1f sqr per partial\n", (double)mf.mul / mf.parts, (double)mf.sqr / mf.parts);
  printf("ops field hit: %.1f mul %.1f sqr per partial\n", (double)hf.mul / hf.parts, (double)hf.sqr / hf.parts);
  printf("sigcache_host ok: %zu groups, %zu partials\n", gs.size(), sigs.size());
  return 0;
}
