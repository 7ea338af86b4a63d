// herumi's blsPublicKeyShare and blsPublicKeyRecover in batches: the per-lane functions of the kernels in vss.hip,
// written once for the device and the host tests (tests/native/vss_host.cpp).  DESIGN.md 4.15.
//
// Everything here is PUBLIC data (Feldman commitments, pubshares, operator ids), so the arithmetic is the
// variable-time one of curve.h / ops.h, and every addition is the complete jac_add / jac_add_aff: an adversary chooses
// the operands, so [x] acc may equal A[j] (a doubling), equal -A[j] (the identity), or either may be the identity.
//
// Decoded points travel between the stages as k_g1_decode leaves them: affine, Montgomery, limb-major (word w of
// point i at pts[w n + i], 24 words) with a code per point (curve.h DEC_OK / DEC_BAD / DEC_INF; a point that is not
// DEC_OK has zero words).
#pragma once
#include "rlc.h"
#include "deal_ct.h"  // recover_ids_status

namespace bls {

constexpr uint32_t VSS_MAX_THRESHOLD = 65535;

// [c] P for a signed 64-bit c: the G1 twin of ops.h g2_mul_i64.  |c| <= 2^63 fits jac_mul_u64 (INT64_MIN included).
BLS_HD BLS_INLINE void g1_mul_i64(g1j& r, const g1j& p, int64_t c) {
  jac_mul_u64(r, p, c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c);
  if (c < 0) {
    g1j t = r;
    jac_neg(r, t);
  }
}

// Point i of a decoded array as a Jacobian point (the identity for DEC_INF)
BLS_HD BLS_INLINE void vss_load_point(g1j& p, const uint32_t* pts, const int32_t* code, uint64_t n, uint64_t i) {
  if (code[i] == DEC_OK) {
    g1a a;
    soa_load<24>(&a.x.v[0], pts, n, i);
    jac_from_aff(p, a);
  } else {
    jac_set_inf(p);
  }
}

// ---- PublicKeyShare ------------------------------------------------------------------------------------------------
// Dealer sum, lane (v, j): A[v][j] = sum_d C[v][d][j] over the decoded commitments (n_in = n_val n_dealers threshold
// points, C[v][d][j] at (v n_dealers + d) threshold + j), written in the same form as point v threshold + j of
// n_out = n_val threshold.  The code is DEC_BAD when any of the dealers' points is.
BLS_HD BLS_INLINE void vss_dealer_sum_lane(uint32_t* out_pts, int32_t* out_code, uint64_t n_out, const uint32_t* pts,
                                           const int32_t* code, uint64_t n_in, uint64_t v, uint32_t n_dealers,
                                           uint32_t threshold, uint32_t j) {
  const uint64_t o = v * threshold + j;
  g1j acc;
  jac_set_inf(acc);
  bool bad = false;
  for (uint32_t d = 0; d < n_dealers; ++d) {
    const uint64_t i = (v * n_dealers + d) * threshold + j;
    const int c = code[i];
    if (c == DEC_BAD) bad = true;
    if (c != DEC_OK) continue;  // the identity adds nothing
    g1a a;
    soa_load<24>(&a.x.v[0], pts, n_in, i);
    g1j t = acc;
    jac_add_aff(acc, t, a);
  }
  g1a r;
  f_set_zero(r.x);
  f_set_zero(r.y);
  int c = DEC_BAD;
  if (!bad) {
    c = DEC_INF;
    if (!jac_is_inf(acc)) {
      jac_to_aff(r, acc);
      c = DEC_OK;
    }
  }
  soa_store<24>(out_pts, n_out, o, &r.x.v[0]);
  out_code[o] = c;
}

// Evaluation, lane (v, i): out48 = sum_j [id^j] A[v][j] by Horner, from the top coefficient down, A[v][j] = point
// v threshold + j of n points.  Returns HIPBLS_OK, or HIPBLS_ERR_PUBKEY with zero bytes when a coefficient of v is bad.
BLS_HD BLS_INLINE int vss_eval_lane(uint8_t* out48, const uint32_t* pts, const int32_t* code, uint64_t n, uint64_t v,
                                    uint32_t threshold, int64_t id) {
  const uint64_t base = v * threshold;
  for (uint32_t j = 0; j < threshold; ++j)
    if (code[base + j] == DEC_BAD) {
      for (int b = 0; b < 48; ++b) out48[b] = 0;
      return HIPBLS_ERR_PUBKEY;
    }
  g1j acc;
  vss_load_point(acc, pts, code, n, base + threshold - 1u);
  for (uint32_t j = threshold - 1u; j != 0u; --j) {
    g1j t;
    g1_mul_i64(t, acc, id);
    if (code[base + j - 1u] == DEC_OK) {
      g1a a;
      soa_load<24>(&a.x.v[0], pts, n, base + j - 1u);
      jac_add_aff(acc, t, a);
    } else {
      acc = t;
    }
  }
  g1_compress(out48, acc);
  return HIPBLS_OK;
}

// ---- PublicKeyRecover: ThresholdAggregate's three stages over G1 ------------------------------------------------------
// Share k of group [g0, g0 + t), me = k - g0: decode, then [c_k] P on the small-integer path (ops.h lagrange_small, the
// group's decision) or [lambda_k] P off it.  out36 is Jacobian (the identity when the status is not OK).  Returns
// HIPBLS_ERR_COMBINE (the group's ids, decided first: nothing is decoded then), HIPBLS_ERR_PUBKEY or HIPBLS_OK.
BLS_HD BLS_INLINE int vss_scale_lane(g1j& out, const uint8_t* share48, const int64_t* gids, int t, int me) {
  jac_set_inf(out);
  if (recover_ids_status(gids, (uint32_t)t) != HIPBLS_OK) return HIPBLS_ERR_COMBINE;
  g1a a;
  const int dc = g1_decompress(a, share48, true);
  if (dc == DEC_BAD) return HIPBLS_ERR_PUBKEY;
  if (dc == DEC_INF) return HIPBLS_OK;
  g1j p;
  jac_from_aff(p, a);
  int64_t c;
  uint64_t L;
  if (lagrange_small(gids, t, me, c, L)) {
    g1_mul_i64(out, p, c);
  } else {
    fr lam;
    lagrange_at_zero(lam, gids, t, me);
    jac_mul_limbs(out, p, lam.v, 8);
  }
  return HIPBLS_OK;
}

// Group of t shares whose scaled points are points g0 .. g0 + t - 1 of n_parts (Jacobian, limb-major, 36 words) with
// statuses pstat: the sum, [L^-1 mod r] of it on the small-integer path, compressed.  Zero bytes unless OK.
BLS_HD BLS_INLINE int vss_sum_lane(uint8_t* out48, const uint32_t* pts, const int32_t* pstat, uint64_t n_parts,
                                   uint64_t g0, const int64_t* gids, int t) {
  int st = recover_ids_status(gids, (uint32_t)t);
  if (st == HIPBLS_OK)
    for (int k = 0; k < t; ++k)
      if (pstat[g0 + k] != HIPBLS_OK) st = pstat[g0 + k];
  if (st != HIPBLS_OK) {
    for (int b = 0; b < 48; ++b) out48[b] = 0;
    return st;
  }
  g1j acc;
  jac_set_inf(acc);
  for (int k = 0; k < t; ++k) {
    g1j p, x = acc;
    soa_load<36>(&p.x.v[0], pts, n_parts, g0 + k);
    jac_add(acc, x, p);
  }
  int64_t c;
  uint64_t L;
  if (lagrange_small(gids, t, 0, c, L) && !jac_is_inf(acc)) {
    fr lf, li, plain;
    fr_from_i64(lf, (int64_t)L);
    fr_inv(li, lf);
    fr_to_plain(plain, li);
    g1j x = acc;
    jac_mul_limbs(acc, x, plain.v, 8);
  }
  g1_compress(out48, acc);
  return HIPBLS_OK;
}

}  // namespace bls
