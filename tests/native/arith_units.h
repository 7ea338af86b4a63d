// Test-only per-lane entry points into every arithmetic layer of charon_amd/csrc, one fixed-size record in and one
// out per case.  The same text is compiled into tests/native/libhost_ops.so (x86, a loop over the cases: ht_arith)
// and into tests/native/libgpu_units.so (gfx950, one case per lane: gu_*_op), so tests/arith_cases.py's case lists
// and expected values run unchanged through both builds.  Include after ops.h / kernels.h.
//
// Records (word = little-endian uint32; "raw" = 12 words, the limbs exactly as given, Montgomery form; "be" = a
// canonical coefficient as 48 big-endian bytes, plain):
//   AU_FP    in  a raw | b raw | k                              25 words     out  r raw | flag          13 words
//   AU_FP2   in  a.c0 a.c1 b.c0 b.c1 raw                        48 words     out  r.c0 r.c1 raw | flag  25 words
//   AU_FP12  in  a | b, 12 be each (tower order)              1152 bytes     out  r, 12 be             576 bytes
//   AU_CURVE in  P jac | Q jac (X Y Z be; G1 three, G2 six coefficients, 288 bytes reserved each) |
//                k 8 words | c int64 | compressed point 96 bytes     720 bytes
//            out flag int32 | pad | R jac (X Y Z be, not normalised: the test divides by Z)   296 bytes
//   AU_H2C   in  len word | message (or u as c0 c1 be)   208 bytes     out  288 bytes (256 xmd bytes / jac / affine)
//   AU_PAIR  in  P0 (x y be) | Q0 (x0 x1 y0 y1 be) | P1 | Q1    576 bytes     out  12 be              576 bytes
#pragma once

namespace au {
using namespace bls;

enum { AU_FP = 0, AU_FP2 = 1, AU_FP12 = 2, AU_CURVE_G1 = 3, AU_CURVE_G2 = 4, AU_H2C = 5, AU_PAIR = 6, AU_LAYERS = 7 };
BLS_HD BLS_INLINE uint32_t in_bytes(int layer) {
  constexpr uint32_t t[AU_LAYERS] = {100, 192, 1152, 720, 720, 208, 576};
  return t[layer];
}
BLS_HD BLS_INLINE uint32_t out_bytes(int layer) {
  constexpr uint32_t t[AU_LAYERS] = {52, 100, 576, 296, 296, 288, 576};
  return t[layer];
}

BLS_HD BLS_INLINE void raw_in(fp& a, const uint32_t* w) {
  for (int i = 0; i < 12; ++i) a.v[i] = w[i];
}
BLS_HD BLS_INLINE void raw_out(uint32_t* w, const fp& a) {
  for (int i = 0; i < 12; ++i) w[i] = a.v[i];
}
BLS_HD BLS_INLINE void be_in(fp& a, const uint8_t* b) {
  fp_plain_from_be48(a, b);
  fp_to_mont(a, a);
}
BLS_HD BLS_INLINE void be_out(uint8_t* o, const fp& a) {
  fp t;
  fp_from_mont(t, a);
  fp_plain_to_be48(o, t);
}
BLS_HD BLS_INLINE void be_in(fp2& a, const uint8_t* b) {
  be_in(a.c0, b);
  be_in(a.c1, b + 48);
}
BLS_HD BLS_INLINE void be_out(uint8_t* o, const fp2& a) {
  be_out(o, a.c0);
  be_out(o + 48, a.c1);
}
BLS_HD BLS_INLINE uint32_t coeff_bytes(const fp&) { return 48; }
BLS_HD BLS_INLINE uint32_t coeff_bytes(const fp2&) { return 96; }
template <class F>
BLS_HD BLS_INLINE void jac_in(jac<F>& p, const uint8_t* b) {
  const uint32_t s = coeff_bytes(p.x);
  be_in(p.x, b);
  be_in(p.y, b + s);
  be_in(p.z, b + 2 * s);
}
template <class F>
BLS_HD BLS_INLINE void jac_out(uint8_t* o, const jac<F>& p) {
  const uint32_t s = coeff_bytes(p.x);
  be_out(o, p.x);
  be_out(o + s, p.y);
  be_out(o + 2 * s, p.z);
}

// ---- Fp on raw limbs:  0 add  1 sub  2 neg  3 half  4 dbl  5 mul_small(k)  6 add_lazy  7 sub_lazy  8 mul
//                        9 inv (binary GCD)  10 inv_pow (Fermat)  11 sqrt (flag = is a square)
BLS_HD BLS_INLINE void fp_case(int op, const uint8_t* in8, uint8_t* out8) {
  const uint32_t* in = (const uint32_t*)in8;
  uint32_t* out = (uint32_t*)out8;
  fp a, b, r;
  raw_in(a, in);
  raw_in(b, in + 12);
  const uint32_t k = in[24];
  uint32_t flag = 0;
  switch (op) {
    case 0: fp_add(r, a, b); break;
    case 1: fp_sub(r, a, b); break;
    case 2: fp_neg(r, a); break;
    case 3: fp_half(r, a); break;
    case 4: fp_dbl(r, a); break;
    case 5: fp_mul_small(r, a, k); break;
    case 6: fp_add_lazy(r, a, b); break;
    case 7: fp_sub_lazy(r, a, b); break;
    case 8: fp_mul(r, a, b); break;
    case 9: fp_inv(r, a); break;
    case 10: fp_inv_pow(r, a); break;
    case 11: flag = fp_sqrt(r, a) ? 1u : 0u; break;
    default: r = a;
  }
  raw_out(out, r);
  out[12] = flag;
}

// ---- Fp2 on raw limbs:  0 mul  1 sqr  2 sqr_c  3 mul_fp(a, b.c0)  4 mul_xi  5 mul_3b2  6 inv  7 sqrt (flag)
BLS_HD BLS_INLINE void fp2_case(int op, const uint8_t* in8, uint8_t* out8) {
  const uint32_t* in = (const uint32_t*)in8;
  uint32_t* out = (uint32_t*)out8;
  fp2 a, b, r;
  raw_in(a.c0, in);
  raw_in(a.c1, in + 12);
  raw_in(b.c0, in + 24);
  raw_in(b.c1, in + 36);
  uint32_t flag = 0;
  switch (op) {
    case 0: fp2_mul(r, a, b); break;
    case 1: fp2_sqr(r, a); break;
    case 2: fp2_sqr_c(r, a); break;
    case 3: fp2_mul_fp(r, a, b.c0); break;
    case 4: fp2_mul_xi(r, a); break;
    case 5: fp2_mul_3b2(r, a); break;
    case 6: fp2_inv(r, a); break;
    case 7: flag = fp2_sqrt(r, a) ? 1u : 0u; break;
    default: r = a;
  }
  raw_out(out, r.c0);
  raw_out(out + 12, r.c1);
  out[24] = flag;
}

// ---- Fp12:  0 mul  1 sqr  2 inv  3..5 Frobenius 1..3  6 cyclotomic sqr  7 sparse line product (b.c0.c0, b.c0.c1,
//             b.c1.c1 = g0, g1, h1)
BLS_HD BLS_INLINE void fp12_case(int op, const uint8_t* in, uint8_t* out) {
  fp12 a, b, r;
  fp* ca = &a.c0.c0.c0;
  fp* cb = &b.c0.c0.c0;
  for (int i = 0; i < 12; ++i) {
    be_in(ca[i], in + 48 * i);
    be_in(cb[i], in + 576 + 48 * i);
  }
  switch (op) {
    case 0: fp12_mul(r, a, b); break;
    case 1: fp12_sqr(r, a); break;
    case 2: fp12_inv(r, a); break;
    case 3: fp12_frobenius(r, a, 1); break;
    case 4: fp12_frobenius(r, a, 2); break;
    case 5: fp12_frobenius(r, a, 3); break;
    case 6: fp12_cyclotomic_sqr(r, a); break;
    case 7:
      fp12_mul_line(a, b.c0.c0, b.c0.c1, b.c1.c1);
      r = a;
      break;
    default: r = a;
  }
  const fp* d = &r.c0.c0.c0;
  for (int i = 0; i < 12; ++i) be_out(out + 48 * i, d[i]);
}

// ---- curve, F = fp / fp2:  0 jac_add(P, Q)  1 jac_add_aff(P, (Q.x, Q.y))  2 jac_dbl(P)  3 jac_mul_limbs(P, k, 8)
//      4 jac_mul_u64(P, k[0..1])  5 jac_eq(P, Q) -> flag  6 g*_in_subgroup(P) -> flag
//      10 / 11 g*_decompress(bytes, check off / on) -> flag = status, R = (x, y, 1) when DEC_OK
//      G2 only:  7 g2_mul_glv4(P, k)  8 g2_clear_cofactor(P)  9 g2_subgroup_and_mul_i64(P, c) -> flag, R
BLS_HD BLS_INLINE bool in_subgroup(const g1j& p) { return g1_in_subgroup(p); }
BLS_HD BLS_INLINE bool in_subgroup(const g2j& p) { return g2_in_subgroup(p); }
BLS_HD BLS_INLINE int decompress(g1a& a, const uint8_t* b, bool chk) { return g1_decompress(a, b, chk); }
BLS_HD BLS_INLINE int decompress(g2a& a, const uint8_t* b, bool chk) { return g2_decompress(a, b, chk); }
BLS_HD BLS_INLINE void g2_only(int, g1j&, const g1j&, const uint32_t*, int64_t, int32_t&) {}
BLS_HD BLS_INLINE void g2_only(int op, g2j& r, const g2j& p, const uint32_t* k, int64_t c, int32_t& flag) {
  if (op == 7)
    g2_mul_glv4(r, p, k);
  else if (op == 8)
    g2_clear_cofactor(r, p);
  else
    flag = g2_subgroup_and_mul_i64(r, p, c) ? 1 : 0;
}
template <class F>
BLS_HD BLS_INLINE void curve_case(int op, const uint8_t* in, uint8_t* out) {
  jac<F> p, q, r;
  jac_in(p, in);
  jac_in(q, in + 288);
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = ((const uint32_t*)(in + 576))[i];
  const uint32_t* cw = (const uint32_t*)(in + 608);
  const int64_t c = (int64_t)((uint64_t)cw[0] | (uint64_t)cw[1] << 32);
  int32_t flag = 0;
  jac_set_inf(r);
  switch (op) {
    case 0: jac_add(r, p, q); break;
    case 1: {
      aff<F> qa;
      qa.x = q.x;
      qa.y = q.y;
      jac_add_aff(r, p, qa);
      break;
    }
    case 2: jac_dbl(r, p); break;
    case 3: jac_mul_limbs(r, p, k, 8); break;
    case 4: jac_mul_u64(r, p, (uint64_t)k[0] | (uint64_t)k[1] << 32); break;
    case 5: flag = jac_eq(p, q) ? 1 : 0; break;
    case 6: flag = in_subgroup(p) ? 1 : 0; break;
    case 7:
    case 8:
    case 9: g2_only(op, r, p, k, c, flag); break;
    case 10:
    case 11: {
      aff<F> a;
      flag = decompress(a, in + 616, op == 11);
      if (flag == DEC_OK) jac_from_aff(r, a);
      break;
    }
    default: break;
  }
  *(int32_t*)out = flag;
  jac_out(out + 8, r);
}

// ---- hash to curve (the POP suite's DST):  0 expand_message_xmd_256 -> 256 bytes  1 hash_to_g2 -> jac (X Y Z be)
//      2 map_to_curve_sswu(u) -> affine (x y be) on the isogenous curve E2'
BLS_HD BLS_INLINE void h2c_case(int op, const uint8_t* in, uint8_t* out) {
  const uint32_t len = *(const uint32_t*)in;
  const uint8_t* msg = in + 4;
  if (op == 0) {
    uint32_t w[64];
    expand_message_xmd_256(w, msg, len, DST_POP, 43);
    for (int i = 0; i < 64; ++i) {
      out[4 * i] = (uint8_t)(w[i] >> 24);
      out[4 * i + 1] = (uint8_t)(w[i] >> 16);
      out[4 * i + 2] = (uint8_t)(w[i] >> 8);
      out[4 * i + 3] = (uint8_t)w[i];
    }
  } else if (op == 1) {
    g2j h;
    hash_to_g2(h, msg, len, DST_POP, 43);
    jac_out(out, h);
  } else {
    fp2 u;
    be_in(u, msg);
    g2a p;
    map_to_curve_sswu(p, u);
    be_out(out, p.x);
    be_out(out + 96, p.y);
  }
}

// ---- pairing on one lane:  0 miller_loop_n(1 pair) + final_exponentiation  1 miller_loop_n(2 pairs) + f.e.
//      2 miller_loop_2 (Verify's two-pair loop) + f.e.
BLS_HD BLS_INLINE void pair_case(int op, const uint8_t* in, uint8_t* out) {
  g1a P[2];
  g2a Q[2];
  bool skip[2] = {false, false};
  for (int i = 0; i < 2; ++i) {
    const uint8_t* b = in + 288 * i;
    be_in(P[i].x, b);
    be_in(P[i].y, b + 48);
    be_in(Q[i].x, b + 96);
    be_in(Q[i].y, b + 192);
  }
  fp12 f, e;
  if (op == 2)
    miller_loop_2(f, P[0], Q[0], P[1], Q[1]);
  else
    miller_loop_n(f, P, Q, skip, op == 1 ? 2 : 1);
  final_exponentiation(e, f);
  const fp* d = &e.c0.c0.c0;
  for (int i = 0; i < 12; ++i) be_out(out + 48 * i, d[i]);
}

}  // namespace au
