// Secret-independent Sign and SecretToPublicKey (tbls/herumi.go Sign, SecretToPublicKey): the per-lane functions of
// k_sign_ct_mul and k_sk_to_pk_ct (sign_ct.hip), written once for the device and the host tests.
//
// Every function here that handles the secret carries the suffix _ct and follows one rule: the secret reaches data
// only.  No branch, no loop bound and no memory address depends on it; a choice is a lane mask (all ones / zero) and a
// bitwise select (gcd30::bfi: v_bfi_b32 on the device), a table read scans EVERY entry at compile-time indices.  They
// are force-inlined into their kernel, so the tables are stack objects of the kernel's own frame, addressed by
// constants.  What they call out of line is uniform by construction: the generated Fp / Fp2 product
// routines (straight-line), fp_inv / fp2_inv (select-only binary GCD, fixed iteration count) and jac_to_aff (one
// inversion, four products).  jac_add and the psi maps only build tables from the public point.
//
// Same bytes and statuses as op_sign / op_sk_to_pk (ops.h), which stay the variable-time batch generators.
#pragma once
#include "ops.h"

namespace bls {

// ---- masks and selects ----------------------------------------------------------------------------------------
BLS_HD BLS_INLINE uint32_t mask_nz_ct(uint32_t x) {  // all ones if x != 0
  return (uint32_t)((int32_t)(x | (0u - x)) >> 31);
}
BLS_HD BLS_INLINE uint32_t fp_zero_mask_ct(const fp& a) {  // all ones if a == 0
  uint32_t acc = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) acc |= a.v[i];
  return ~mask_nz_ct(acc);
}
// r = m ? a : b, limb by limb (m all ones or zero; r may be a or b)
BLS_HD BLS_INLINE void f_sel_ct(fp& r, uint32_t m, const fp& a, const fp& b) {
#pragma unroll
  for (int i = 0; i < 12; ++i) r.v[i] = gcd30::bfi(m, a.v[i], b.v[i]);
}
BLS_HD BLS_INLINE void f_sel_ct(fp2& r, uint32_t m, const fp2& a, const fp2& b) {
  f_sel_ct(r.c0, m, a.c0, b.c0);
  f_sel_ct(r.c1, m, a.c1, b.c1);
}
template <class F>
BLS_HD BLS_INLINE void jac_sel_ct(jac<F>& r, uint32_t m, const jac<F>& a, const jac<F>& b) {
  f_sel_ct(r.x, m, a.x, b.x);
  f_sel_ct(r.y, m, a.y, b.y);
  f_sel_ct(r.z, m, a.z, b.z);
}

// r = tab[d] for a secret d in [0, 16): every entry is read, the wanted one is kept by mask.  The table is walked in
// pieces of 24 words (one Fp2, or two Fp): a piece of every entry is loaded, then selected.  On the device a
// scheduling fence keeps each piece's loads together ahead of its selects, so that a piece costs one memory round
// trip; left alone, the compiler (at this kernel's register count) issues every word's load, wait and select one
// after the other.
#if defined(__HIP_DEVICE_COMPILE__)
#define BLS_CT_SCHED_FENCE() __builtin_amdgcn_sched_barrier(0)
#else
#define BLS_CT_SCHED_FENCE() ((void)0)
#endif
template <class F>
BLS_HD BLS_INLINE void jac_scan16_ct(jac<F>& r, const jac<F>* tab, uint32_t d) {
  constexpr int W = (int)(sizeof(jac<F>) / 4), PIECE = 24;
  static_assert(sizeof(jac<F>) % 4 == 0 && W % 12 == 0, "limbs only");
  uint32_t m[16];
#pragma unroll
  for (int j = 1; j < 16; ++j) m[j] = gcd30::mask_eq(d, (uint32_t)j);
  uint32_t* out = reinterpret_cast<uint32_t*>(&r);
#pragma unroll
  for (int w0 = 0; w0 < W; w0 += PIECE) {
    const int len = W - w0 < PIECE ? W - w0 : PIECE;
    uint32_t e[PIECE];
#pragma unroll
    for (int k = 0; k < len; ++k) e[k] = reinterpret_cast<const uint32_t*>(&tab[0])[w0 + k];
#pragma unroll
    for (int j = 1; j < 16; ++j) {
      uint32_t t[PIECE];
#pragma unroll
      for (int k = 0; k < len; ++k) t[k] = reinterpret_cast<const uint32_t*>(&tab[j])[w0 + k];
      BLS_CT_SCHED_FENCE();
#pragma unroll
      for (int k = 0; k < len; ++k) e[k] = gcd30::bfi(m[j], t[k], e[k]);
      BLS_CT_SCHED_FENCE();
    }
#pragma unroll
    for (int k = 0; k < len; ++k) out[w0 + k] = e[k];
  }
}

// add-2007-bl without its exceptional cases: r = p + q for p, q != infinity and p != +-q.  For any other operands the
// result is some field elements (never a fault); the callers discard it by mask.
template <class F>
BLS_HD BLS_INLINE void jac_add_ne_ct(jac<F>& r, const jac<F>& p, const jac<F>& q) {
  F z1z1, z2z2, u1, u2, s1, s2, h, i, j, rr, v, t;
  f_sqr(z1z1, p.z);
  f_sqr(z2z2, q.z);
  f_mul(u1, p.x, z2z2);
  f_mul(u2, q.x, z1z1);
  f_mul(s1, p.y, q.z);
  f_mul(s1, s1, z2z2);
  f_mul(s2, q.y, p.z);
  f_mul(s2, s2, z1z1);
  f_sub(h, u2, u1);
  f_sub(rr, s2, s1);
  f_add(rr, rr, rr);
  f_add(i, h, h);
  f_sqr(i, i);
  f_mul(j, h, i);
  f_mul(v, u1, i);
  F x3, y3, z3;
  f_sqr(x3, rr);
  f_sub(x3, x3, j);
  f_sub(x3, x3, v);
  f_sub(x3, x3, v);
  f_sub(t, v, x3);
  f_mul(y3, rr, t);
  f_mul(t, s1, j);
  f_add(t, t, t);
  f_sub(y3, y3, t);
  f_add(z3, p.z, q.z);
  f_sqr(z3, z3);
  f_sub(z3, z3, z1z1);
  f_sub(z3, z3, z2z2);
  f_mul(z3, z3, h);
  r.x = x3;
  r.y = y3;
  r.z = z3;
}

// One step of the fixed-pattern ladders below: acc <- acc + tab[d] with acc's "still infinity" state carried as the
// mask inf.  The addition always runs; the result is chosen among {acc, entry, sum} by the masks "d == 0" and inf.
template <class F>
BLS_HD BLS_INLINE void jac_step_ct(jac<F>& acc, uint32_t& inf, const jac<F>* tab, uint32_t d) {
  jac<F> ent, sum;
  jac_scan16_ct(ent, tab, d);
  jac_add_ne_ct(sum, acc, ent);
  const uint32_t d0 = gcd30::mask_eq(d, 0u);
  jac_sel_ct(sum, inf, ent, sum);
  jac_sel_ct(acc, d0, acc, sum);
  inf &= d0;
}

// ---- scalar decomposition -------------------------------------------------------------------------------------
// u256_divmod_xabs (curve.h) with the "subtract?" decision of each of the 256 shift-subtract steps as a mask.  The
// dividend leaves k at the top while the quotient enters at the bottom, so the step counter is a count and nothing
// else: no shift amount, no index.
BLS_HD BLS_INLINE uint64_t u256_divmod_xabs_ct(uint32_t* k) {
  uint64_t rem = 0;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int step = 0; step < 256; ++step) {
    const uint64_t top = rem >> 63;
    rem = (rem << 1) | (k[7] >> 31);
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 1) | (k[i - 1] >> 31);
    const uint64_t diff = rem - X_ABS;
    const uint64_t borrow = ((~rem & X_ABS) | ((~rem | X_ABS) & diff)) >> 63;  // rem < |x|
    const uint64_t take = top | (borrow ^ 1u);
    const uint32_t m = 0u - (uint32_t)take;
    const uint32_t lo = gcd30::bfi(m, (uint32_t)diff, (uint32_t)rem);
    const uint32_t hi = gcd30::bfi(m, (uint32_t)(diff >> 32), (uint32_t)(rem >> 32));
    rem = (uint64_t)hi << 32 | lo;
    k[0] = (k[0] << 1) | (uint32_t)take;
  }
  return rem;
}

// ---- G2: [k] P by the GLS-4 split, 64 x (double, scan, add, select) ----------------------------------------------
// k = e0 + e1|x| + e2|x|^2 + e3|x|^3 (base-|x| digits, as g2_mul_glv4) over the 16 subset sums of
// {P, -psi P, psi^2 P, -psi^3 P} = {[1]P, [|x|]P, [|x|^2]P, [|x|^3]P}.  P is public (H(m)); its table is built with
// the general addition.  inf_out: all ones when the result is the point at infinity (k = 0, or P = infinity); r then
// holds unspecified field elements.  For 0 < k < r no step's addition is exceptional.
BLS_HD BLS_INLINE void g2_mul_ct(g2j& r, uint32_t& inf_out, const g2j& p, const uint32_t* k_plain) {
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = k_plain[i];
  uint64_t e[4];
  for (int i = 0; i < 3; ++i) e[i] = u256_divmod_xabs_ct(k);
  e[3] = (uint64_t)k[0] | ((uint64_t)k[1] << 32);
  g2j tab[16];
  jac_set_inf(tab[0]);
  tab[1] = p;
  g2_psi(tab[2], tab[1]);
  jac_neg(tab[2], tab[2]);
  g2_psi2(tab[4], tab[1]);
  g2_psi(tab[8], tab[4]);
  jac_neg(tab[8], tab[8]);
  for (int d = 3; d < 16; ++d) {
    const int low = d & -d;
    if (d != low) jac_add(tab[d], tab[d ^ low], tab[low]);
  }
  g2j acc;
  jac_set_inf(acc);
  uint32_t inf = ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int step = 0; step < 64; ++step) {
    g2j t;
    jac_dbl_body(t, acc);  // Z = 0 stays Z = 0; a point of odd order never meets the doubling's exception
    acc = t;
    // the digits leave e[] at the top: the step counter is a count and nothing else
    const uint32_t d = (uint32_t)(e[0] >> 63) | (uint32_t)((e[1] >> 63) << 1) | (uint32_t)((e[2] >> 63) << 2) |
                       (uint32_t)((e[3] >> 63) << 3);
    for (int i = 0; i < 4; ++i) e[i] <<= 1;
    jac_step_ct(acc, inf, tab, d);
  }
  r = acc;
  inf_out = inf | (fp_zero_mask_ct(p.z.c0) & fp_zero_mask_ct(p.z.c1));
}

// ---- G1: [k] g1 by a fixed 4-bit window, 64 x (4 doublings, scan, add, select) ------------------------------------
BLS_HD BLS_INLINE void g1_mul_ct(g1j& r, uint32_t& inf_out, const uint32_t* k_plain) {
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = k_plain[i];
  g1j tab[16];
  jac_set_inf(tab[0]);
  tab[1].x = G1_GEN_X;
  tab[1].y = G1_GEN_Y;
  fp_set_one(tab[1].z);
  for (int d = 2; d < 16; ++d) jac_add(tab[d], tab[d - 1], tab[1]);  // public constants
  g1j acc;
  jac_set_inf(acc);
  uint32_t inf = ~0u;
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
  for (int step = 0; step < 64; ++step) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 1
#endif
    for (int s = 0; s < 4; ++s) {
      g1j t;
      jac_dbl_body(t, acc);
      acc = t;
    }
    const uint32_t d = k[7] >> 28;  // the windows leave k at the top
#pragma unroll
    for (int i = 7; i > 0; --i) k[i] = (k[i] << 4) | (k[i - 1] >> 28);
    k[0] <<= 4;
    jac_step_ct(acc, inf, tab, d);
  }
  r = acc;
  inf_out = inf;
}

// ---- compression: the sign flag by select, the infinity encoding by mask -----------------------------------------
BLS_HD BLS_INLINE uint32_t fp_plain_gt_half_mask_ct(const fp& a) {  // fp_plain_gt_half as a mask
  constexpr uint32_t H[12] = {0xffffd555u, 0xdcff7fffu, 0x58a9ffffu, 0x0f55ffffu, 0x7b587b12u, 0xb3986950u,
                              0x79c2895fu, 0xb23ba5c2u, 0x21a5d66bu, 0x258dd3dbu, 0x1cbff34du, 0x0d0088f5u};
  int64_t br = 0;
#pragma unroll
  for (int i = 0; i < 12; ++i) {
    br += (int64_t)H[i] - a.v[i];
    br >>= 32;
  }
  return (uint32_t)br;  // 0 or -1
}
BLS_HD BLS_INLINE uint32_t fp_lex_mask_ct(const fp& y) {
  fp t;
  fp_from_mont(t, y);
  return fp_plain_gt_half_mask_ct(t);
}
BLS_HD BLS_INLINE uint32_t fp2_lex_mask_ct(const fp2& y) {
  fp t1, t0;
  fp_from_mont(t1, y.c1);
  fp_from_mont(t0, y.c0);
  return gcd30::bfi(fp_zero_mask_ct(t1), fp_plain_gt_half_mask_ct(t0), fp_plain_gt_half_mask_ct(t1));
}
// keep: all ones to emit the encoding, zero to emit zero bytes (a bad status)
BLS_HD BLS_INLINE void g1_compress_ct(uint8_t* b, const g1j& p, uint32_t inf, uint32_t keep) {
  g1a a;
  jac_to_aff(a, p);
  fp x;
  fp_from_mont(x, a.x);
  fp_plain_to_be48(b, x);
  const uint32_t flags = 0x80u | (fp_lex_mask_ct(a.y) & 0x20u);
  b[0] = (uint8_t)(gcd30::bfi(inf, 0xc0u, (uint32_t)b[0] | flags) & keep);
  for (int i = 1; i < 48; ++i) b[i] = (uint8_t)((uint32_t)b[i] & ~inf & keep);
}
BLS_HD BLS_INLINE void g2_compress_ct(uint8_t* b, const g2j& p, uint32_t inf, uint32_t keep) {
  g2a a;
  jac_to_aff(a, p);
  fp x1, x0;
  fp_from_mont(x1, a.x.c1);
  fp_from_mont(x0, a.x.c0);
  fp_plain_to_be48(b, x1);
  fp_plain_to_be48(b + 48, x0);
  const uint32_t flags = 0x80u | (fp2_lex_mask_ct(a.y) & 0x20u);
  b[0] = (uint8_t)(gcd30::bfi(inf, 0xc0u, (uint32_t)b[0] | flags) & keep);
  for (int i = 1; i < 96; ++i) b[i] = (uint8_t)((uint32_t)b[i] & ~inf & keep);
}

// ---- the per-item operations ------------------------------------------------------------------------------------
// sk (32 big-endian bytes) -> limbs; returns the mask "sk < r"
BLS_HD BLS_INLINE uint32_t fr_load_mask_ct(fr& r, const uint8_t* b) {
  for (int i = 0; i < 8; ++i) {
    const uint8_t* q = b + 28 - 4 * i;
    r.v[i] = ((uint32_t)q[0] << 24) | ((uint32_t)q[1] << 16) | ((uint32_t)q[2] << 8) | (uint32_t)q[3];
  }
  int64_t br = 0;
  for (int i = 0; i < 8; ++i) {
    br += (int64_t)r.v[i] - FR_LIMBS[i];
    br >>= 32;
  }
  return (uint32_t)br;
}

// sigma = [sk] H for an already hashed message (H = hash_to_g2(msg, DST_POP), public).  Always writes 96 bytes: the
// signature, or zeros with HIPBLS_ERR_SECRET (sk >= r).  sk = 0 gives the infinity encoding, as op_sign does.
BLS_HD BLS_INLINE int op_sign_mul_ct(uint8_t* out96, const g2j& h, const uint8_t* sk32) {
  fr sk;
  const uint32_t ok = fr_load_mask_ct(sk, sk32);
  g2j s;
  uint32_t inf;
  g2_mul_ct(s, inf, h, sk.v);
  g2_compress_ct(out96, s, inf, ok);
  return (int)gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
}
BLS_HD BLS_INLINE int op_sign_ct(uint8_t* out96, const uint8_t* sk32, const uint8_t* msg, uint32_t msg_len) {
  g2j h;
  hash_to_g2(h, msg, msg_len, DST_POP, 43);  // the message is public: the hash is the existing, variable-time one
  return op_sign_mul_ct(out96, h, sk32);
}

// pk = [sk] g1.  Always writes 48 bytes: the key, or zeros with HIPBLS_ERR_SECRET (sk = 0 or sk >= r).
BLS_HD BLS_INLINE int op_sk_to_pk_ct(uint8_t* out48, const uint8_t* sk32) {
  fr sk;
  uint32_t ok = fr_load_mask_ct(sk, sk32);
  uint32_t any = 0;
  for (int i = 0; i < 8; ++i) any |= sk.v[i];
  ok &= mask_nz_ct(any);
  g1j pk;
  uint32_t inf;
  g1_mul_ct(pk, inf, sk.v);
  g1_compress_ct(out48, pk, inf, ok);
  return (int)gcd30::bfi(ok, (uint32_t)HIPBLS_OK, (uint32_t)HIPBLS_ERR_SECRET);
}

}  // namespace bls
