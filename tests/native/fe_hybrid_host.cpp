// Host program for the fused Verify's final exponentiation (tests/test_fe_hybrid_host.py): pairing_lds.h's hybrid
// a^|x| (compressed squarings to bit 57, Granger-Scott squarings above it) against pairing.h's fp12_cyc_exp_xabs_gs
// word for word, and final_exp_is_one_l (compare with conj(m^3), no last product) against
// fp12_is_one(final_exponentiation(f)).  Exit status 0 = all passed.  Test-only; also built with
// -fsanitize=address,undefined.
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

static u32x4 g_f12[36];  // one lane's Fp12 accumulator (S = 1)
static const f12l<1> F{g_f12};

// Any twelve limbs below p are an element (in Montgomery form): the top limb is kept below p's.
static void fp_random(fp& r) {
  for (int i = 0; i < 11; ++i) r.v[i] = (uint32_t)rnd();
  r.v[11] = (uint32_t)(rnd() % 0x1a0111eaull);
}
static void fp12_random(fp12& r) {
  fp* c = &r.c0.c0.c0;
  for (int i = 0; i < 12; ++i) fp_random(c[i]);
}
static void fp12_set_zero_all(fp12& r) { memset(&r, 0, sizeof(r)); }
static bool same(const fp12& a, const fp12& b) { return !memcmp(&a, &b, sizeof(fp12)); }

// f^((p^6-1)(p^2+1)): the final exponentiation's easy part, which lands in the cyclotomic subgroup
static void easy_part(fp12& m, const fp12& f) {
  fp12 t, fi;
  fp12_conj(t, f);
  fp12_inv(fi, f);
  fp12_mul(m, t, fi);
  fp12_frobenius(t, m, 2);
  fp12_mul(m, t, m);
}

static void states_of(cyc_c* st, const fp12& a) {
  cyc_c c;
  c.z2 = a.c1.c0;
  c.z3 = a.c0.c2;
  c.z4 = a.c0.c1;
  c.z5 = a.c1.c2;
  static const int runs[6] = {16, 32, 9, 3, 2, 1};
  for (int s = 0; s < KAR_STATES; ++s) {
    cyc_sqr_run(c, runs[s]);
    st[s] = c;
  }
}

// The power against Granger-Scott's, and the flag the caller's fallback hangs on.
static int power_agrees(const fp12& a, bool want_fallback) {
  fp12 want, got, guard;
  fp12_cyc_exp_xabs_gs(want, a);
  memset(&guard, 0xA5, sizeof(guard));
  got = guard;
  const bool fallback = fp12_cyc_exp_xabs_karabina_l(got, a, F);
  CHECK(fallback == want_fallback);
  if (fallback)
    CHECK(same(got, guard));  // r untouched: the caller computes it
  else
    CHECK(same(got, want));
  got = guard;
  fp12_cyc_exp_xabs_l(got, a, F);
  CHECK(same(got, want));
  return 0;
}

static int powers() {
  // the hybrid power saves a^(2^16), a^(2^48) and a^(2^57); built with -DBLS_FE_HYBRID=0, all six
  static_assert(KAR_STATES == (BLS_FE_HYBRID ? 3 : 6), "saved compressed states");
  fp12 one;
  fp12_set_one(one);
  int non_trivial = 0;
  for (int i = 0; i < 200; ++i) {
    fp12 f, m;
    fp12_random(f);
    easy_part(m, f);
    non_trivial += !fp12_is_one(m);
    if (power_agrees(m, false)) return 1;
  }
  CHECK(non_trivial == 200);
  if (power_agrees(one, true)) return 1;

  // A vanishing denominator.  den is 4 z2, or z3 where z2 == 0, so it vanishes only with z2 == z3 == 0.  In the
  // cyclotomic subgroup the relations behind cyc_z1_parts then give z4 z5 == 0 and xi z5^2 + 3 z4^2 == 0, so z4 == z5
  // == 0 too: the element lies in Fp4, and the subgroup (of order p^4 - p^2 + 1, prime to p^4 - 1) meets Fp4 in the
  // identity alone.  Squaring is a bijection there (odd order), so no power of another element vanishes either.  An
  // input with a vanishing denominator other than the identity is therefore outside the subgroup: an Fp4 element
  // (z2..z5 == 0 at every state) goes through the whole function, and the test at each single state is made on the
  // states themselves (those of a real element with z2, z3 zeroed at one of them), since an input that reaches such a
  // state at bit 16, 48 or 57 alone would take inverting the squaring map to build.
  {
    fp12 a;
    fp12_set_zero_all(a);
    fp_random(a.c0.c0.c0);
    fp_random(a.c0.c0.c1);
    fp_random(a.c1.c1.c0);
    fp_random(a.c1.c1.c1);
    if (power_agrees(a, true)) return 1;
    fp12_set_zero_all(a);  // and 0 itself
    if (power_agrees(a, true)) return 1;
  }
  {
    fp12 f, m, want, got, guard;
    fp12_random(f);
    easy_part(m, f);
    fp12_cyc_exp_xabs_gs(want, m);
    cyc_c st[KAR_STATES];
    states_of(st, m);
    memset(&guard, 0x5A, sizeof(guard));
    got = guard;
    CHECK(!cyc_exp_xabs_from_states_l(got, st, F) && same(got, want));
    for (int s = 0; s < KAR_STATES; ++s) {
      cyc_c t[KAR_STATES];
      memcpy(t, st, sizeof(t));
      fp2_set_zero(t[s].z2);
      fp2_set_zero(t[s].z3);
      got = guard;
      CHECK(cyc_exp_xabs_from_states_l(got, t, F) && same(got, guard));
      // z2 == 0 alone is no degenerate state: the other formula's denominator z3 stands in
      memcpy(t, st, sizeof(t));
      fp2_set_zero(t[s].z2);
      got = guard;
      CHECK(!cyc_exp_xabs_from_states_l(got, t, F) && !same(got, guard));
    }
  }
  return 0;
}

struct Item {
  uint8_t sk[32], pk48[48], root[32], sig96[96];
  g1a pk;
  g2a hm, sig;
};

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

// final_exp_is_one_l on f against fp12_is_one(final_exponentiation(f)), and the value form against the value.
static int is_one_agrees(const fp12& f, bool want_one) {
  fp12 e, el;
  final_exponentiation(e, f);
  CHECK(fp12_is_one(e) == want_one);
  final_exponentiation_l(el, f, F);
  CHECK(same(e, el));
  CHECK(final_exp_is_one_l(f, F) == want_one);
  fp12 g = f;  // whichever form the build's BLS_FE_CMP gives Verify's check
  CHECK(final_exp_l_is_one(g, F) == want_one);
  return 0;
}

static int triple(const g1a& pk, const g2a& hm, const g2a& sig, int want_status) {
  g1a P1;
  P1.x = G1_GEN_X;
  P1.y = G1_NEG_GEN_Y;
  fp12 f;
  g2j T1;
  miller_loop_2(f, pk, hm, P1, sig, &T1);
  // a signature outside G2 is refused by its own check whatever the pairing gives; the comparison still has to agree
  fp12 e;
  final_exponentiation(e, f);
  if (is_one_agrees(f, fp12_is_one(e))) return 1;
  if (want_status != HIPBLS_ERR_SIGNATURE) CHECK(fp12_is_one(e) == (want_status == HIPBLS_OK));
  CHECK(pairing_check_verify_sig(pk, hm, sig) == want_status);
  CHECK((pairing_check_verify_sig_l_body<1, true>(pk, hm, sig, F)) == want_status);
  CHECK((pairing_check_verify_sig_l<1>(pk, hm, sig, F)) == want_status);
  return 0;
}

static int finals() {
  std::vector<Item> items(4);
  for (auto& it : items)
    if (make_item(it)) return 1;
  for (const Item& it : items)
    if (triple(it.pk, it.hm, it.sig, HIPBLS_OK)) return 1;
  const Item& a = items[0];
  const Item& b = items[1];
  if (triple(a.pk, b.hm, a.sig, HIPBLS_ERR_VERIFY)) return 1;  // a wrong root
  if (triple(b.pk, a.hm, a.sig, HIPBLS_ERR_VERIFY)) return 1;  // a swapped key
  if (triple(a.pk, a.hm, b.sig, HIPBLS_ERR_VERIFY)) return 1;  // another item's signature
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
    if (triple(a.pk, a.hm, s, HIPBLS_ERR_SIGNATURE)) return 1;
    found = false;
    for (int t = 0; t < 64 && !found; ++t) {
      uint8_t w[96];
      for (auto& x : w) x = (uint8_t)rnd();
      w[0] = (uint8_t)(0x80 | (w[0] & 0x1f));
      found = g2_decompress(s, w, false) == DEC_OK;
    }
    CHECK(found);
    if (triple(a.pk, a.hm, s, HIPBLS_ERR_SIGNATURE)) return 1;
  }
  // f = 0: fp12_inv(0) is 0, every later value is 0, and 0 is not one -- in the value form and in the comparison
  fp12 z, e;
  fp12_set_zero_all(z);
  final_exponentiation(e, z);
  CHECK(fp12_is_zero(e) && !fp12_is_one(e));
  if (is_one_agrees(z, false)) return 1;
  // f = 1 and an Fp2 element: the easy part gives the identity; random elements: not one
  fp12 f;
  fp12_set_one(f);
  if (is_one_agrees(f, true)) return 1;
  fp12_set_zero_all(f);
  fp_random(f.c0.c0.c0);
  fp_random(f.c0.c0.c1);
  if (is_one_agrees(f, true)) return 1;
  for (int i = 0; i < 8; ++i) {
    fp12_random(f);
    if (is_one_agrees(f, false)) return 1;
  }
  return 0;
}

int main() {
  if (powers()) return 1;
  if (finals()) return 1;
  printf("fe_hybrid_host ok: 200 powers\n");
  return 0;
}
