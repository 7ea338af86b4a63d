// A joint-Feldman dealing round in batches (kryptology dkg/frost rounds 1 and 2): the per-lane
// functions of k_commit_ct, k_share_check_ct and k_share_sum_ct (dkg_ct.hip), written once for the device and the host
// tests.
//
// The rule is deal_ct.h's: a secret (a polynomial coefficient, a share received from a dealer, a node's final share)
// reaches data only.  What is PUBLIC here and may steer control flow and addresses: the lane's position (validator v,
// coefficient j, dealer d), threshold, n_dealers, the commitments with their decode status, the include mask, and the
// VERDICT of a share check (a complaint is broadcast).  Every function that handles a secret carries the suffix _ct
// and is force-inlined into its kernel; beyond deal_ct.h's callees they call nothing.
#pragma once
#include "deal_ct.h"

namespace bls {

// ---- commitments: [a_j] g1 for coefficient j of a validator's polynomial --------------------------------------------
// The mask "the secret and every tail coefficient are below r", over the public threshold (what split_eval_ct returns,
// without the evaluation).
BLS_HD BLS_INLINE uint32_t commit_valid_ct(const uint8_t* secret32, const uint8_t* tail, uint32_t threshold) {
  fr coef;
  uint32_t ok = ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t j = threshold - 1u; j != 0u; --j) ok &= fr_load_mask_ct(coef, tail + 32 * (size_t)(j - 1u));
  ok &= fr_load_mask_ct(coef, secret32);
  return ok;
}

// Lane (v, j): out48 = [a_j] g1 compressed, a_0 the secret and a_j = tail[j-1]; the infinity encoding with status OK for
// a zero coefficient; zero bytes and ERR_SECRET for every coefficient of a validator that has one >= r.  j is public.
// At every comb step the accumulator is [a mod 16^w] g1 with a < r, so g1_madd_ne_ct meets no exceptional pair.
BLS_HD BLS_INLINE int op_commit_ct(uint8_t* out48, comb_ptr T, const uint8_t* secret32, const uint8_t* tail,
                                   uint32_t threshold, uint32_t j) {
  const uint32_t ok = commit_valid_ct(secret32, tail, threshold);
  const uint8_t* const src = j == 0u ? secret32 : tail + 32 * (size_t)(j - 1u);  // a select on the public j
  fr a;
  (void)fr_load_zero_ct(a, src);
  for (int i = 0; i < 8; ++i) a.v[i] &= ok;
  g1j p;
  uint32_t inf;
  g1_mul_comb_ct(p, inf, T, a.v);
  g1_compress48_ct(out48, p, inf, ok);
  return (int)gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
}

// ---- the receiver's check of one share against its dealer's commitments ---------------------------------------------
// Lane (v, d): [share] g1 compressed (the infinity encoding for a zero share; a share >= r enters as 0) against the 48
// expected bytes, the dealer's polynomial commitment evaluated at the receiver's id, by an OR of XORs over all 48
// bytes.  decode_status is the public status of that evaluation (not OK: a commitment did not decode).  The verdict,
// in this order: ERR_PUBKEY, ERR_SECRET (share >= r), ERR_VERIFY (mismatch), OK.
BLS_HD BLS_INLINE int op_share_check_ct(comb_ptr T, const uint8_t* share32, const uint8_t* expected48,
                                        int decode_status) {
  fr s;
  const uint32_t below = fr_load_zero_ct(s, share32);
  g1j p;
  uint32_t inf;
  g1_mul_comb_ct(p, inf, T, s.v);
  uint8_t got[48];
  g1_compress48_ct(got, p, inf, ~0u);
  uint32_t diff = 0;
#pragma unroll
  for (int b = 0; b < 48; ++b) diff |= (uint32_t)(got[b] ^ expected48[b]);
  const uint32_t same = ~mask_nz_ct(diff);
  const uint32_t pub_ok = gcd30::mask_eq((uint32_t)decode_status, (uint32_t)HIPBLS_OK);
  uint32_t st = gcd30::bfi(same, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_VERIFY);
  st = gcd30::bfi(below, st, (uint32_t)HIPBLS_ERR_SECRET);
  return (int)gcd30::bfi(pub_ok, st, (uint32_t)HIPBLS_ERR_PUBKEY);
}

// ---- a node's final share: the sum of the shares of the qualified dealers -------------------------------------------
// One term: acc += share for the bytes at share32 when `active` (the public include mask of the dealer) is all ones;
// an excluded dealer adds 0 and leaves ok alone (recover_term_ct's pattern).  Plain limbs below r throughout.
BLS_HD BLS_INLINE void share_sum_term_ct(fr& acc, uint32_t& ok, const uint8_t* share32, uint32_t active) {
  fr s;
  const uint32_t below = fr_load_zero_ct(s, share32);
  for (int i = 0; i < 8; ++i) s.v[i] &= active;
  ok &= below | ~active;
  fr_add_ct(acc, acc, s);
}
// The end of it: the sum's bytes and the status from the public mask any_included and the mask ok; the scalar for the
// pubshare is left in sum_plain (zero unless the status is OK), keep_out says whether it is.
BLS_HD BLS_INLINE int share_sum_finish_ct(uint8_t* out32, fr& sum_plain, uint32_t& keep_out, const fr& acc,
                                          uint32_t any_included, uint32_t ok) {
  const uint32_t keep = any_included & ok;
  for (int i = 0; i < 8; ++i) sum_plain.v[i] = acc.v[i] & keep;
  fr_store_be32_ct(out32, sum_plain, keep);
  keep_out = keep;
  const uint32_t st = gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
  return (int)gcd30::bfi(any_included, st, (uint32_t)HIPBLS_ERR_COMBINE);
}

// A whole validator on one lane, for the host (the kernel runs the same pieces).  include: n_dealers bytes or null.
BLS_HD BLS_INLINE int op_share_sum_ct(uint8_t* out32, uint8_t* pub48, int* pub_status, comb_ptr T, bool with_pub,
                                      const uint8_t* shares, const uint8_t* include, uint32_t n_dealers) {
  fr acc;
  for (int i = 0; i < 8; ++i) acc.v[i] = 0;
  uint32_t ok = ~0u, any = 0u;
  for (uint32_t d = 0; d < n_dealers; ++d) {
    const uint32_t act = include == nullptr || include[d] != 0 ? ~0u : 0u;  // public
    any |= act;
    share_sum_term_ct(acc, ok, shares + 32 * (size_t)d, act);
  }
  fr sum;
  uint32_t keep;
  const int st = share_sum_finish_ct(out32, sum, keep, acc, any, ok);
  if (with_pub) *pub_status = g1_pub_ct(pub48, T, sum, keep);
  return st;
}

}  // namespace bls
