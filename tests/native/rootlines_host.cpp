// Host program for the root cache's line blocks (tests/test_rootlines_host.py): charon_amd/csrc/rootcache.h's block
// format and check, the recording and the replaying Miller loops of pairing_lds.h against pairing.h's miller_loop_2,
// and the plan / publish rules on a host-side table (lanes one by one) through the chain k_verify_fused runs
// (rlc.h op_verify_l_kernel_rc).  Exit status 0 = all passed.  Test-only; also built with -fsanitize=address,undefined.
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

static uint64_t g_rng = 0xD1B54A32D192ED03ull;
static uint64_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return g_rng;
}

struct Item {
  uint8_t sk[32], pk48[48], root[32], sig96[96];
  g1a pk;
  g2a hm, sig;
};

static u32x4 g_f12[36];  // one lane's Fp12 accumulator (S = 1)
static const f12l<1> F{g_f12};

static int make_item(Item& it) {
  for (auto& b : it.sk) b = (uint8_t)rnd();
  it.sk[0] &= 0x3f;  // below r
  for (auto& b : it.root) b = (uint8_t)rnd();
  CHECK(op_sk_to_pk(it.pk48, it.sk) == HIPBLS_OK);
  CHECK(op_sign(it.sig96, it.sk, it.root, 32) == HIPBLS_OK);
  CHECK(g1_decompress(it.pk, it.pk48, true) == DEC_OK);
  CHECK(g2_decompress(it.sig, it.sig96, false) == DEC_OK);
  g2j hj;
  hash_to_g2(hj, it.root, 32, DST_POP, 43);
  jac_to_aff(it.hm, hj);
  return 0;
}

static uint64_t seed_of(const uint8_t* root) {
  uint32_t tag[8];
  rc_tag_from_msg(tag, root);
  return rl_seed(rc_tag_hash(tag));
}

// Record hm's lines into blk while the full loop runs; f and T1 as the loop leaves them.
static void record(fp12& f, g2j& T1, uint32_t* blk, const g1a& pk, const g2a& hm, const g2a& sig, uint64_t seed) {
  g1a P1;
  P1.x = G1_GEN_X;
  P1.y = G1_NEG_GEN_Y;
  rl_recorder rec{blk, seed};
  miller_loop_2_l_body<1, true>(f, F, pk, hm, P1, sig, &T1, rec);
  rl_plan plan{};
  uint32_t word = 0;
  plan.record = blk;
  plan.entry_word = &word;
  plan.index1 = 1;
  rl_publish(plan, rec.h);
}

static int loops_agree(const Item& it, const g1a& pk, const g2a& sig, std::vector<uint32_t>& blk) {
  g1a P1;
  P1.x = G1_GEN_X;
  P1.y = G1_NEG_GEN_Y;
  fp12 want, f;
  g2j wantT, T1;
  miller_loop_2(want, pk, it.hm, P1, sig, &wantT);
  const uint64_t seed = seed_of(it.root);
  blk.assign(RL_BLOCK_WORDS, 0xA5A5A5A5u);  // a pool is never zeroed
  record(f, T1, blk.data(), pk, it.hm, sig, seed);
  CHECK(!memcmp(&f, &want, sizeof(f)) && !memcmp(&T1, &wantT, sizeof(T1)));
  CHECK(rl_block_ok(blk.data(), seed));
  memset(&f, 0, sizeof(f));
  memset(&T1, 0, sizeof(T1));
  CHECK(miller_loop_2_l_replay<1>(f, F, pk, sig, &T1, blk.data(), seed));
  CHECK(!memcmp(&f, &want, sizeof(f)) && !memcmp(&T1, &wantT, sizeof(T1)));
  // a recording loop with the flag off is the plain loop
  rl_recorder off{nullptr, 0};
  miller_loop_2_l_body<1, true>(f, F, pk, it.hm, P1, sig, &T1, off);
  CHECK(!memcmp(&f, &want, sizeof(f)) && !memcmp(&T1, &wantT, sizeof(T1)) && off.h == 0);
  return 0;
}

// The status of one pairing check three ways: recording, replaying, replaying a corrupt block (then the fallback).
static int statuses_agree(const g1a& pk, const g2a& hm, const g2a& sig, const uint8_t* root, int* st_out) {
  const int want = pairing_check_verify_sig(pk, hm, sig);
  const uint64_t seed = seed_of(root);
  std::vector<uint32_t> blk(RL_BLOCK_WORDS, 0);
  uint32_t word = 0;
  unsigned long long c[RL_CTRS] = {};
  rl_plan none{};
  CHECK((pairing_check_verify_sig_l_body<1, true, true>(pk, hm, sig, F, &none)) == want);
  rl_plan rec{};
  rec.record = blk.data();
  rec.entry_word = &word;
  rec.index1 = 7;
  rec.seed = seed;
  rec.lctr = c;
  CHECK((pairing_check_verify_sig_l_body<1, true, true>(pk, hm, sig, F, &rec)) == want);
  CHECK(word == 7 && rl_block_ok(blk.data(), seed));
  CHECK(c[RL_CTR_PUBLISHED] == 1 && c[RL_CTR_HITS] == 0 && c[RL_CTR_BAD] == 0);
  rl_plan rep{};
  rep.replay = blk.data();
  rep.seed = seed;
  rep.lctr = c;
  CHECK((pairing_check_verify_sig_l_body<1, true, true>(pk, hm, sig, F, &rep)) == want);
  CHECK(c[RL_CTR_HITS] == 1 && c[RL_CTR_BAD] == 0);
  blk[(size_t)(rnd() % RL_CHK)] ^= 1u << (rnd() % 32);
  CHECK((pairing_check_verify_sig_l_body<1, true, true>(pk, hm, sig, F, &rep)) == want);
  CHECK(c[RL_CTR_HITS] == 1 && c[RL_CTR_BAD] == 1 && c[RL_CTR_PUBLISHED] == 1);
  *st_out = want;
  return 0;
}

static int block_checks(const std::vector<uint32_t>& good, uint64_t seed, uint64_t other_seed) {
  CHECK(rl_block_ok(good.data(), seed));
  CHECK(good[RL_CHK] != 0 && good[RL_CHK + 1] != 0);
  CHECK(!rl_block_ok(good.data(), other_seed));  // root A's block presented for root B
  std::vector<uint32_t> t(RL_BLOCK_WORDS, 0);
  CHECK(!rl_block_ok(t.data(), seed));  // an all-zero block
  CHECK(!rl_block_ok(t.data(), 0));
  // every word under the check, and the check's own two: zeroed, and one bit flipped
  int nonzero = 0;
  for (int w = 0; w < RL_CHK + 2; ++w) {
    t = good;
    if (good[w]) {
      ++nonzero;
      t[w] = 0;
      CHECK(!rl_block_ok(t.data(), seed));
    }
    t[w] = good[w] ^ (1u << (w % 32));
    CHECK(!rl_block_ok(t.data(), seed));
  }
  CHECK(nonzero > RL_CHK - 16);
  // a seeded sample of subsets zeroed: scattered words, whole lines, everything from some word on
  for (int trial = 0; trial < 600; ++trial) {
    t = good;
    if (trial % 3 == 0) {
      const int k = 1 + (int)(rnd() % 64);
      for (int j = 0; j < k; ++j) t[rnd() % (RL_CHK + 2)] = 0;
    } else if (trial % 3 == 1) {
      const int l = (int)(rnd() % RL_LINES);
      memset(&t[(size_t)l * RL_LINE_WORDS], 0, RL_LINE_WORDS * 4);
    } else {
      const size_t from = rnd() % (RL_CHK + 2);
      memset(&t[from], 0, (RL_CHK + 2 - from) * 4);
    }
    if (t == good) continue;
    CHECK(!rl_block_ok(t.data(), seed));
  }
  return 0;
}

// The plan and publish rules on a serial table: two blocks for three roots.
static int pool_checks(const std::vector<Item>& items) {
  const uint32_t slots = 8, blocks = 2;
  std::vector<uint32_t> entries(slots * RC_WORDS, 0), claim(slots, 0), pool((size_t)blocks * RL_BLOCK_WORDS, 0x5A5A5A5Au);
  const std::vector<uint32_t> guard = pool;
  unsigned long long ctr[3] = {0, 0, 0}, lctr[RL_CTRS] = {};
  rootcache rc{};
  rc.entries = entries.data();
  rc.claim = claim.data();
  rc.ctr = ctr;
  rc.mask = slots - 1;
  rc.lines = pool.data();
  rc.blocks = blocks;
  rc.lctr = lctr;
  const keycache kc{};
  auto slot_of = [&](const Item& it) {
    uint32_t tag[8];
    rc_tag_from_msg(tag, it.root);
    return rc_find(rc, tag);
  };
  auto verify = [&](const Item& it) {
    return op_verify_l_kernel_rc<1>(it.pk48, it.root, 32, it.sig96, F, kc, rc, slot_of(it));
  };
  auto lines_word = [&](const Item& it) { return entries[(size_t)slot_of(it) * RC_WORDS + RC_LINES]; };

  // cold: roots 0 and 1 take the two blocks, root 2 meets a full pool and publishes H alone
  for (int i = 0; i < 3; ++i) CHECK(verify(items[i]) == HIPBLS_OK);
  CHECK(ctr[2] == 3 && lctr[RL_CTR_PUBLISHED] == 2 && lctr[RL_CTR_FULL] == 1 && lctr[RL_CTR_HITS] == 0);
  CHECK(lines_word(items[0]) == 1 && lines_word(items[1]) == 2 && lines_word(items[2]) == 0);
  CHECK(rl_block_ok(pool.data(), seed_of(items[0].root)));
  CHECK(rl_block_ok(pool.data() + RL_BLOCK_WORDS, seed_of(items[1].root)));
  // warm: two replay, the third runs the full loop on its cached H and claims nothing; the index is written once
  const std::vector<uint32_t> filled = pool, e0 = entries;
  for (int i = 0; i < 3; ++i) CHECK(verify(items[i]) == HIPBLS_OK);
  CHECK(ctr[2] == 3 && lctr[RL_CTR_HITS] == 2 && lctr[RL_CTR_PUBLISHED] == 2 && lctr[RL_CTR_BAD] == 0);
  CHECK(pool == filled && entries == e0);
  // a failing item replays to the same status
  {
    Item x = items[0];
    memcpy(x.sig96, items[1].sig96, 96);
    CHECK(verify(x) == HIPBLS_ERR_VERIFY && lctr[RL_CTR_HITS] == 3);
  }
  // an index outside the pool is never followed: the full loop, no hit, no failure
  {
    const uint32_t s = slot_of(items[0]);
    entries[(size_t)s * RC_WORDS + RC_LINES] = blocks + 1;
    CHECK(verify(items[0]) == HIPBLS_OK && lctr[RL_CTR_HITS] == 3 && lctr[RL_CTR_BAD] == 0);
    entries[(size_t)s * RC_WORDS + RC_LINES] = 0xffffffffu;
    CHECK(verify(items[0]) == HIPBLS_OK && lctr[RL_CTR_HITS] == 3 && lctr[RL_CTR_BAD] == 0);
    // and an index that names another root's block fails that block's check and falls back
    entries[(size_t)s * RC_WORDS + RC_LINES] = 2;
    CHECK(verify(items[0]) == HIPBLS_OK && lctr[RL_CTR_HITS] == 3 && lctr[RL_CTR_BAD] == 1);
  }
  // a rollover: the table is emptied and the counter starts over, the pool keeps its words
  std::fill(entries.begin(), entries.end(), 0);
  std::fill(claim.begin(), claim.end(), 0);
  lctr[RL_CTR_NEXT] = 0;
  CHECK(!rl_block_ok(pool.data(), seed_of(items[2].root)));  // block 0 still holds root 0's lines: not root 2's
  CHECK(verify(items[2]) == HIPBLS_OK);
  CHECK(lines_word(items[2]) == 1 && lctr[RL_CTR_PUBLISHED] == 3 && rl_block_ok(pool.data(), seed_of(items[2].root)));
  CHECK(verify(items[2]) == HIPBLS_OK && lctr[RL_CTR_HITS] == 4);
  // the stale block of an earlier generation that does pass is that root's own: root 1 again, served from block 1 if
  // the entry ever named it
  CHECK(rl_block_ok(pool.data() + RL_BLOCK_WORDS, seed_of(items[1].root)));

  // lines off: the plan stays empty and the pool is not touched
  rootcache off = rc;
  off.lines = nullptr;
  off.blocks = 0;
  off.lctr = nullptr;
  const std::vector<uint32_t> before = pool;
  uint32_t tag[8];
  rc_tag_from_msg(tag, items[3].root);
  CHECK(op_verify_l_kernel_rc<1>(items[3].pk48, items[3].root, 32, items[3].sig96, F, kc, off, RC_NONE) == HIPBLS_OK);
  CHECK(pool == before && rc_find(off, tag) != RC_NONE);
  // k_verify_fused's own chain (no plan at all) serves the same entries: a hit on root 3, a swapped share on root 2
  CHECK((op_verify_l_kernel_rc<1, false>(items[3].pk48, items[3].root, 32, items[3].sig96, F, kc, rc, rc_find(rc, tag))) ==
        HIPBLS_OK);
  CHECK((op_verify_l_kernel_rc<1, false>(items[2].pk48, items[2].root, 32, items[3].sig96, F, kc, rc, slot_of(items[2]))) ==
        HIPBLS_ERR_VERIFY);
  CHECK(pool == before);
  (void)guard;
  return 0;
}

int main() {
  std::vector<Item> items(12);
  for (auto& it : items)
    if (make_item(it)) return 1;

  // record, then replay: f and T1 word for word as miller_loop_2's, valid pairs and failing ones alike
  std::vector<uint32_t> blk, blk0;
  for (size_t i = 0; i < items.size(); ++i) {
    const Item& it = items[i];
    const g1a& pk = i % 4 == 3 ? items[(i + 1) % items.size()].pk : it.pk;
    if (loops_agree(it, pk, it.sig, blk)) return 1;
    if (i == 0) blk0 = blk;
  }
  if (block_checks(blk0, seed_of(items[0].root), seed_of(items[1].root))) return 1;

  // statuses against pairing_check_verify_sig
  const Item& a = items[0];
  const Item& b = items[1];
  int st = -1;
  if (statuses_agree(a.pk, a.hm, a.sig, a.root, &st)) return 1;
  CHECK(st == HIPBLS_OK);
  if (statuses_agree(a.pk, b.hm, a.sig, b.root, &st)) return 1;  // a wrong root
  CHECK(st == HIPBLS_ERR_VERIFY);
  if (statuses_agree(b.pk, a.hm, a.sig, a.root, &st)) return 1;  // a swapped key
  CHECK(st == HIPBLS_ERR_VERIFY);
  {
    // a flipped signature bit that still decodes, and a random point on the curve: both outside G2
    g2a s;
    bool found = false;
    for (int bit = 8; bit < 768 && !found; ++bit) {
      uint8_t w[96];
      memcpy(w, a.sig96, 96);
      w[bit / 8] ^= (uint8_t)(1u << (bit % 8));
      found = g2_decompress(s, w, false) == DEC_OK;
    }
    CHECK(found);
    if (statuses_agree(a.pk, a.hm, s, a.root, &st)) return 1;
    CHECK(st == HIPBLS_ERR_SIGNATURE);
    found = false;
    for (int t = 0; t < 64 && !found; ++t) {
      uint8_t w[96];
      for (auto& x : w) x = (uint8_t)rnd();
      w[0] = (uint8_t)(0x80 | (w[0] & 0x1f));
      found = g2_decompress(s, w, false) == DEC_OK;
    }
    CHECK(found);
    if (statuses_agree(a.pk, a.hm, s, a.root, &st)) return 1;
    CHECK(st == HIPBLS_ERR_SIGNATURE);
  }
  if (pool_checks(items)) return 1;
  printf("rootlines_host ok: %zu items\n", items.size());
  return 0;
}
