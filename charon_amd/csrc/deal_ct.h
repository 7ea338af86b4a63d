// Secret-independent ThresholdSplit and RecoverSecret in batches (tbls/herumi.go ThresholdSplit, RecoverSecret, and
// the SecretToPublicKey calls that follow them in dkg/keycast.go and cmd/combine): the per-lane functions of k_deal_ct
// and k_recover_ct (deal_ct.hip), written once for the device and the host tests.
//
// The rule is sign_ct.h's: a secret (the root secret, a polynomial coefficient, a share, the recovered secret)
// reaches data only.  What is PUBLIC here and may steer control flow and addresses: the lane's position (validator
// v, share index k, group g), total, threshold, the share ids and the group sizes.  Every function that handles a
// secret carries the suffix _ct and is force-inlined into its kernel.  Beyond sign_ct.h's callees they call nothing
// out of line; the kernels call lagrange_at_zero and recover_ids_status on the public ids.
#pragma once
#include "sign_ct.h"

namespace bls {

#if defined(BLS_CT_TRACE) && !defined(__HIP_DEVICE_COMPILE__)
enum : uint8_t { CT_FR_ADD = 32, CT_FR_SUB, CT_FR_MUL };  // operation codes after field.h's
#endif

// ---- Fr with selects by mask ------------------------------------------------------------------------------------
// fr.h's fr_add / fr_sub / fr_mul with the final choice as a mask from the borrow and gcd30::bfi instead of `?:`.
// Operands below r (a coefficient or share >= r enters as 0: fr_load_zero_ct), so every intermediate is in range.
BLS_HD BLS_INLINE void fr_add_ct(fr& r, const fr& a, const fr& b) {
  BLS_CT_OP(CT_FR_ADD);
  uint32_t s[8], d[8];
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)a.v[i] + b.v[i];
    s[i] = (uint32_t)c;
    c >>= 32;
  }
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    br += (int64_t)s[i] - FR_LIMBS[i];
    d[i] = (uint32_t)br;
    br >>= 32;
  }
  const uint32_t keep_s = (uint32_t)br & ~(0u - (uint32_t)c);  // s < r and no carry out
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = gcd30::bfi(keep_s, s[i], d[i]);
}

BLS_HD BLS_INLINE void fr_sub_ct(fr& r, const fr& a, const fr& b) {
  BLS_CT_OP(CT_FR_SUB);
  uint32_t d[8], e[8];
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    br += (int64_t)a.v[i] - b.v[i];
    d[i] = (uint32_t)br;
    br >>= 32;
  }
  const uint32_t neg = (uint32_t)br;  // a < b: add r back
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    c += (uint64_t)d[i] + FR_LIMBS[i];
    e[i] = (uint32_t)c;
    c >>= 32;
  }
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = gcd30::bfi(neg, e[i], d[i]);
}

// CIOS Montgomery product, as fr_mul
BLS_HD BLS_INLINE void fr_mul_ct(fr& r, const fr& a, const fr& b) {
  BLS_CT_OP(CT_FR_MUL);
  uint32_t t[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const uint32_t bi = b.v[i];
    uint64_t A = (uint64_t)a.v[0] * bi + t[0];
    t[0] = (uint32_t)A;
    const uint32_t m = t[0] * FR_INV32;
    uint64_t C = (uint64_t)m * FR_LIMBS[0] + t[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) {
      A = (uint64_t)a.v[j] * bi + t[j] + (A >> 32);
      t[j] = (uint32_t)A;
      C = (uint64_t)m * FR_LIMBS[j] + t[j] + (C >> 32);
      t[j - 1] = (uint32_t)C;
    }
    t[7] = (uint32_t)(C >> 32) + (uint32_t)(A >> 32);
  }
  uint32_t d[8];
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    br += (int64_t)t[i] - FR_LIMBS[i];
    d[i] = (uint32_t)br;
    br >>= 32;
  }
  const uint32_t keep_t = (uint32_t)br;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.v[i] = gcd30::bfi(keep_t, t[i], d[i]);
}
BLS_HD BLS_INLINE void fr_to_mont_ct(fr& r, const fr& a) {
  fr r2;
  for (int i = 0; i < 8; ++i) r2.v[i] = FR_R2[i];
  fr_mul_ct(r, a, r2);
}
BLS_HD BLS_INLINE void fr_from_mont_ct(fr& r, const fr& a) {
  fr one;
  for (int i = 0; i < 8; ++i) one.v[i] = i == 0 ? 1u : 0u;
  fr_mul_ct(r, a, one);
}
// 32 big-endian bytes -> limbs below r: the value, or 0 when it is >= r.  Returns the mask "value < r", which drives
// the status and the zero-fill only.
BLS_HD BLS_INLINE uint32_t fr_load_zero_ct(fr& r, const uint8_t* b) {
  const uint32_t ok = fr_load_mask_ct(r, b);
  for (int i = 0; i < 8; ++i) r.v[i] &= ok;
  return ok;
}
BLS_HD BLS_INLINE void fr_store_be32_ct(uint8_t* out, const fr& a, uint32_t keep) {
#pragma unroll
  for (int w = 0; w < 8; ++w)
#pragma unroll
    for (int b = 0; b < 4; ++b) out[31 - 4 * w - b] = (uint8_t)((a.v[w] & keep) >> (8 * b));
}

// ---- the split: f(k) = secret + a_1 k + ... + a_{t-1} k^{t-1} by Horner -------------------------------------------
// k and threshold are public; every lane of a launch runs threshold steps.  k = 0 gives the secret itself.  Returns
// the mask "the secret and every coefficient are below r"; share_plain is f(k) with bad coefficients taken as 0.
BLS_HD BLS_INLINE uint32_t split_eval_ct(fr& share_plain, const uint8_t* secret32, const uint8_t* tail,
                                         uint32_t threshold, uint32_t k) {
  fr x, acc, coef;
  for (int i = 0; i < 8; ++i) {
    x.v[i] = i == 0 ? k : 0u;
    acc.v[i] = 0;
  }
  fr_to_mont_ct(x, x);
  uint32_t ok = ~0u;
  // the tail from the top coefficient down, then the secret: the trip count is the public threshold - 1
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (uint32_t j = threshold - 1u; j != 0u; --j) {
    ok &= fr_load_zero_ct(coef, tail + 32 * (size_t)(j - 1u));
    fr_to_mont_ct(coef, coef);
    fr_mul_ct(acc, acc, x);
    fr_add_ct(acc, acc, coef);
  }
  ok &= fr_load_zero_ct(coef, secret32);
  fr_to_mont_ct(coef, coef);
  fr_mul_ct(acc, acc, x);
  fr_add_ct(acc, acc, coef);
  fr_from_mont_ct(share_plain, acc);
  return ok;
}

// ---- [s] g1 over a fixed-base comb: 64 mixed additions, no doubling ------------------------------------------------
// T[w][j-1] = [j 16^w] g1 for w = 0..63, j = 1..15: affine, Montgomery, x then y (24 words per entry; k_g1_comb_build).
constexpr int COMB_WINDOWS = 64;
constexpr int COMB_ROW_WORDS = 15 * 24;
constexpr int COMB_WORDS = COMB_WINDOWS * COMB_ROW_WORDS;  // 92,160 bytes

// The table is read through a uniform pointer into read-only memory: on the device the constant address space, whose
// uniform loads are scalar loads (the address is the wave's, it cannot be a lane's).
#if defined(__HIP_DEVICE_COMPILE__)
typedef const __attribute__((address_space(4))) uint32_t* comb_ptr;
#define BLS_COMB_PTR(p) ((::bls::comb_ptr)(p))
#else
typedef const uint32_t* comb_ptr;
#define BLS_COMB_PTR(p) (p)
#endif

// [j 16^w] g1 as a scalar, for the builder and the tests (public)
BLS_HD BLS_INLINE void comb_entry_scalar(uint32_t* k8, int w, int j) {
  for (int i = 0; i < 8; ++i) k8[i] = 0;
  k8[w >> 3] = (uint32_t)j << (4 * (w & 7));
}
// The builder's lane (w, j): variable-time arithmetic on public values
BLS_HD BLS_INLINE void comb_build_entry(uint32_t* out24, int w, int j) {
  uint32_t k[8];
  comb_entry_scalar(k, w, j);
  g1j g, p;
  g.x = G1_GEN_X;
  g.y = G1_GEN_Y;
  fp_set_one(g.z);
  jac_mul_limbs(p, g, k, 8);
  g1a a;
  jac_to_aff(a, p);
  for (int i = 0; i < 12; ++i) {
    out24[i] = a.x.v[i];
    out24[12 + i] = a.y.v[i];
  }
}

// madd-2007-bl without its exceptional cases: r = p + (qx, qy) for p != infinity, p != +-q.  For any other operands
// the result is some field elements; the caller discards it by mask.
BLS_HD BLS_INLINE void g1_madd_ne_ct(g1j& r, const g1j& p, const fp& qx, const fp& qy) {
  fp z1z1, u2, s2, h, hh, i, j, rr, v, t, x3, y3, z3;
  f_sqr(z1z1, p.z);
  f_mul(u2, qx, z1z1);
  f_mul(s2, qy, p.z);
  f_mul(s2, s2, z1z1);
  f_sub(h, u2, p.x);
  f_sqr(hh, h);
  f_add(i, hh, hh);
  f_add(i, i, i);
  f_mul(j, h, i);
  f_sub(rr, s2, p.y);
  f_add(rr, rr, rr);
  f_mul(v, p.x, i);
  f_sqr(x3, rr);
  f_sub(x3, x3, j);
  f_sub(x3, x3, v);
  f_sub(x3, x3, v);
  f_sub(t, v, x3);
  f_mul(y3, rr, t);
  f_mul(t, p.y, j);
  f_add(t, t, t);
  f_sub(y3, y3, t);
  f_add(z3, p.z, h);
  f_sqr(z3, z3);
  f_sub(z3, z3, z1z1);
  f_sub(z3, z3, hh);
  r.x = x3;
  r.y = y3;
  r.z = z3;
}

// The digits leave k at the bottom, lowest window first.  At step w the accumulator is [k mod 16^w] g1 and the entry
// [d 16^w] g1, d the window: never equal, never opposite for k < r.  Every step reads all 15 entries
// of T[w] at addresses that only w decides and keeps one by the masks d == j.
BLS_HD BLS_INLINE void g1_mul_comb_ct(g1j& r, uint32_t& inf_out, comb_ptr T, const uint32_t* k_plain) {
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = k_plain[i];
  g1j acc;
  jac_set_inf(acc);
  fp one;
  fp_set_one(one);
  uint32_t inf = ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int w = 0; w < COMB_WINDOWS; ++w) {
    const uint32_t d = k[0] & 15u;
#pragma unroll
    for (int i = 0; i < 7; ++i) k[i] = (k[i] >> 4) | (k[i + 1] << 28);
    k[7] >>= 4;
    comb_ptr row = T + (size_t)w * COMB_ROW_WORDS;
    uint32_t e[24];
#pragma unroll
    for (int i = 0; i < 24; ++i) e[i] = row[i];  // entry 1; the others replace it under their masks
#pragma unroll
    for (int j = 2; j < 16; ++j) {
      const uint32_t m = gcd30::mask_eq(d, (uint32_t)j);
      uint32_t t[24];
#pragma unroll
      for (int i = 0; i < 24; ++i) t[i] = row[(j - 1) * 24 + i];
#pragma unroll
      for (int i = 0; i < 24; ++i) e[i] = gcd30::bfi(m, t[i], e[i]);
    }
    g1j ent, sum;
#pragma unroll
    for (int i = 0; i < 12; ++i) {
      ent.x.v[i] = e[i];
      ent.y.v[i] = e[12 + i];
    }
    ent.z = one;
    g1_madd_ne_ct(sum, acc, ent.x, ent.y);
    const uint32_t d0 = gcd30::mask_eq(d, 0u);
    jac_sel_ct(sum, inf, ent, sum);
    jac_sel_ct(acc, d0, acc, sum);
    inf &= d0;
  }
  r = acc;
  inf_out = inf;
}

// g1_compress_ct's bytes, formed a word at a time at compile-time positions (its byte loops, left rolled, index the
// output by the loop counter)
BLS_HD BLS_INLINE void g1_compress48_ct(uint8_t* b, const g1j& p, uint32_t inf, uint32_t keep) {
  g1a a;
  jac_to_aff(a, p);
  fp x;
  fp_from_mont(x, a.x);
  const uint32_t flags = (0x80u | (fp_lex_mask_ct(a.y) & 0x20u)) << 24;
#pragma unroll
  for (int t = 0; t < 12; ++t) {
    uint32_t w = x.v[11 - t];
    if (t == 0) w = gcd30::bfi(inf, 0xc0000000u, w | flags);
    else w &= ~inf;
    w &= keep;
    b[4 * t] = (uint8_t)(w >> 24);
    b[4 * t + 1] = (uint8_t)(w >> 16);
    b[4 * t + 2] = (uint8_t)(w >> 8);
    b[4 * t + 3] = (uint8_t)w;
  }
}

// [s] g1 compressed for a scalar below r, with hipbls_secret_to_public_key_batch_ct's bytes and status: the key, or
// zero bytes and HIPBLS_ERR_SECRET for s = 0 or a clear `ok` (the scalar's validator or group failed).
BLS_HD BLS_INLINE int g1_pub_ct(uint8_t* out48, comb_ptr T, const fr& s_plain, uint32_t ok) {
  uint32_t any = 0;
  for (int i = 0; i < 8; ++i) any |= s_plain.v[i];
  ok &= mask_nz_ct(any);
  g1j pk;
  uint32_t inf;
  g1_mul_comb_ct(pk, inf, T, s_plain.v);
  g1_compress48_ct(out48, pk, inf, ok);
  return (int)gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
}

// ---- the per-lane operations ----------------------------------------------------------------------------------------
// Lane (v, k) of the deal: share32 = f_v(k) (zero bytes when the validator is bad) and the validator's status; the
// scalar for the public key is left in share_plain (zero for a bad validator) with its mask in ok_out.
BLS_HD BLS_INLINE int op_deal_ct(uint8_t* share32, fr& share_plain, uint32_t& ok_out, const uint8_t* secret32,
                                 const uint8_t* tail, uint32_t threshold, uint32_t k) {
  const uint32_t ok = split_eval_ct(share_plain, secret32, tail, threshold, k);
  for (int i = 0; i < 8; ++i) share_plain.v[i] &= ok;
  fr_store_be32_ct(share32, share_plain, ok);
  ok_out = ok;
  return (int)gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
}

// HIPBLS_OK, or HIPBLS_ERR_COMBINE for an empty group, an id 0 or a duplicate id: public, variable-time
BLS_HD BLS_CALL int recover_ids_status(const int64_t* ids, uint32_t m) {
  int st = m > 0 ? HIPBLS_OK : HIPBLS_ERR_COMBINE;
  for (uint32_t a = 0; a < m; ++a) {
    if (ids[a] == 0) st = HIPBLS_ERR_COMBINE;
    for (uint32_t b = a + 1; b < m; ++b)
      if (ids[a] == ids[b]) st = HIPBLS_ERR_COMBINE;
  }
  return st;
}

// One term of the recovery: acc += lambda s, for the share bytes at share32 when `active` (the public k < m of the
// lane's group) is all ones; an inactive lane adds 0 and leaves ok alone.  lambda is public (plain).
BLS_HD BLS_INLINE void recover_term_ct(fr& acc, uint32_t& ok, const fr& lam_plain, const uint8_t* share32,
                                       uint32_t active) {
  fr s, lam;
  const uint32_t below = fr_load_zero_ct(s, share32);
  for (int i = 0; i < 8; ++i) s.v[i] &= active;
  ok &= below | ~active;
  fr_to_mont_ct(lam, lam_plain);
  fr_to_mont_ct(s, s);
  fr_mul_ct(s, s, lam);
  fr_add_ct(acc, acc, s);
}
// The end of it: the secret's bytes and the status from the public one (ids_status) and the mask ok; the scalar for
// the public key is left in secret_plain (zero unless the status is OK), keep_out says whether it is.
BLS_HD BLS_INLINE int recover_finish_ct(uint8_t* out32, fr& secret_plain, uint32_t& keep_out, const fr& acc,
                                        int ids_status, uint32_t ok) {
  const uint32_t pub_ok = gcd30::mask_eq((uint32_t)ids_status, (uint32_t)HIPBLS_OK);
  const uint32_t keep = pub_ok & ok;
  fr_from_mont_ct(secret_plain, acc);
  for (int i = 0; i < 8; ++i) secret_plain.v[i] &= keep;
  fr_store_be32_ct(out32, secret_plain, keep);
  keep_out = keep;
  const uint32_t st = gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
  return (int)gcd30::bfi(pub_ok, st, (uint32_t)ids_status);
}

// A whole group on one lane, for the host (the kernel runs the same pieces over the launch's largest group size).
BLS_HD BLS_INLINE int op_recover_ct(uint8_t* out32, uint8_t* pub48, int* pub_status, comb_ptr T, bool with_pub,
                                    const uint8_t* shares, const int64_t* ids, uint32_t m, uint32_t m_max) {
  const int ids_status = recover_ids_status(ids, m);
  fr acc;
  for (int i = 0; i < 8; ++i) acc.v[i] = 0;
  uint32_t ok = ~0u;
  for (uint32_t k = 0; k < m_max; ++k) {
    const bool act = k < m;  // public
    const uint32_t kk = act ? k : 0u;
    fr lam;
    lagrange_at_zero(lam, ids, act ? (int)m : 0, (int)kk);
    recover_term_ct(acc, ok, lam, shares + 32 * (size_t)kk, act ? ~0u : 0u);
  }
  fr secret;
  uint32_t keep;
  const int st = recover_finish_ct(out32, secret, keep, acc, ids_status, ok);
  if (with_pub) *pub_status = g1_pub_ct(pub48, T, secret, keep);
  return st;
}

}  // namespace bls
