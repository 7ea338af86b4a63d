// G2 arithmetic dealt out over a lane quad, and the lone sigagg route's pieces built from it (verify_lat.hip
// k_tv_prep8 / k_tagg_sum8, verify_hex.hip k_tv_pair_lq16).  Split-Fp2 builds only (BLS_FP2_PAIR): a unit of work is an
// octet, the quad q = lane & 3 with its Fp2 twins on lanes 4-7, and every lane of the octet holds the same values, so
// every branch below is octet-uniform.  Different octets of a wave may diverge (the DPP moves stay inside the octet).
// Same formulas as the one-lane code (curve.h, ops.h): the points are the same group elements, so the compressed
// bytes and the statuses do not change.
#pragma once
#include "lg2.h"

namespace bls {

// G2 doubling (curve.h jac_dbl_body, dbl-2009-l) with its seven Fp2 products dealt out over the quad's lanes
// (q = lane & 3): level 1 X^2 | Y^2 | Y Z, level 2 B^2 | (X + B)^2 | E^2, level 3 E (D - X3) on every lane; each level's
// products are broadcast to the quad (lg2.h quad_bcast).  Three products of latency instead of seven; every lane
// ends with the same point.  All four lanes (and, here, their Fp2 twins) must be active.
__device__ __forceinline__ void g2_dbl_quad(g2j& r, const g2j& p, int q) {
  const uint32_t q1 = q == 1 ? ~0u : 0u, q2 = q == 2 ? ~0u : 0u;
  fp2 x, y, o;
  x = sel(q2, p.y, sel(q1, p.y, p.x));
  y = sel(q2, p.z, sel(q1, p.y, p.x));
  fp2_mul(o, x, y);  // X^2 | Y^2 | Y Z
  const fp2 A = quad_bcast<0>(o), B = quad_bcast<1>(o), YZ = quad_bcast<2>(o);
  fp2 XB, E;
  fp2_add(XB, p.x, B);
  fp2_add(E, A, A);
  fp2_add(E, E, A);
  x = sel(q2, E, sel(q1, XB, B));
  fp2_mul(o, x, x);  // C = B^2 | (X + B)^2 | F = E^2
  const fp2 C = quad_bcast<0>(o), T = quad_bcast<1>(o), Fv = quad_bcast<2>(o);
  fp2 t, D, x3, c8;
  fp2_sub(t, T, A);
  fp2_sub(t, t, C);
  fp2_add(D, t, t);
  fp2_sub(x3, Fv, D);
  fp2_sub(x3, x3, D);
  fp2_sub(t, D, x3);
  fp2_mul(t, E, t);
  fp2_add(c8, C, C);
  fp2_add(c8, c8, c8);
  fp2_add(c8, c8, c8);
  fp2_sub(r.y, t, c8);
  fp2_add(r.z, YZ, YZ);
  r.x = x3;
}

// G2 addition (curve.h jac_add_body, add-2007-bl: 11 products + 5 squarings) dealt out over the quad in five levels
// of one product per lane, each level broadcast to the quad:
//   1: Z1^2 | Z2^2 | Y1 Z2 | Y2 Z1          2: U1 = X1 Z2^2 | U2 = X2 Z1^2 | S1 = Y1 Z2^3 | S2 = Y2 Z1^3
//   3: I = (2H)^2 | R^2 | (Z1 + Z2)^2        4: J = H I | V = U1 I | Z3 = ((Z1 + Z2)^2 - Z1^2 - Z2^2) H
//   5: R (V - X3) | S1 J
// Five products of latency instead of sixteen; squarings as products of equal operands (the same canonical values).
// The exceptional cases (an input at infinity, H = 0) take jac_add on every lane: the values are the same on all
// four lanes, so those branches are quad-uniform.  All four lanes (and their Fp2 twins) must be active.
__device__ __forceinline__ void g2_add_quad(g2j& r, const g2j& p, const g2j& qp, int q) {
  if (jac_is_inf(p) || jac_is_inf(qp)) {
    jac_add(r, p, qp);
    return;
  }
  const uint32_t q1 = q == 1 ? ~0u : 0u, q2 = q == 2 ? ~0u : 0u, q3 = q == 3 ? ~0u : 0u;
  fp2 x, y, o;
  x = sel(q3, qp.y, sel(q2, p.y, sel(q1, qp.z, p.z)));
  y = sel(q3, p.z, sel(q2, qp.z, sel(q1, qp.z, p.z)));
  fp2_mul(o, x, y);
  const fp2 z1z1 = quad_bcast<0>(o), z2z2 = quad_bcast<1>(o), s1a = quad_bcast<2>(o), s2a = quad_bcast<3>(o);
  x = sel(q3, s2a, sel(q2, s1a, sel(q1, qp.x, p.x)));
  y = sel(q3, z1z1, sel(q2, z2z2, sel(q1, z1z1, z2z2)));
  fp2_mul(o, x, y);
  const fp2 u1 = quad_bcast<0>(o), u2 = quad_bcast<1>(o), s1 = quad_bcast<2>(o), s2 = quad_bcast<3>(o);
  fp2 h, rr;
  fp2_sub(h, u2, u1);
  fp2_sub(rr, s2, s1);
  if (fp2_is_zero(h)) {  // the same on all four lanes
    if (fp2_is_zero(rr))
      jac_dbl(r, p);
    else
      jac_set_inf(r);
    return;
  }
  fp2_add(rr, rr, rr);
  fp2 h2, zs;
  fp2_add(h2, h, h);
  fp2_add(zs, p.z, qp.z);
  x = sel(q2, zs, sel(q1, rr, h2));
  fp2_mul(o, x, x);
  const fp2 i = quad_bcast<0>(o), r2 = quad_bcast<1>(o), zz = quad_bcast<2>(o);
  fp2 zc;
  fp2_sub(zc, zz, z1z1);
  fp2_sub(zc, zc, z2z2);
  x = sel(q2, zc, sel(q1, u1, h));
  y = sel(q2, h, i);
  fp2_mul(o, x, y);
  const fp2 j = quad_bcast<0>(o), v = quad_bcast<1>(o), z3 = quad_bcast<2>(o);
  fp2 x3, t;
  fp2_sub(x3, r2, j);
  fp2_sub(x3, x3, v);
  fp2_sub(x3, x3, v);
  fp2_sub(t, v, x3);
  x = sel(q1, s1, rr);
  y = sel(q1, j, t);
  fp2_mul(o, x, y);
  const fp2 y3a = quad_bcast<0>(o), s1j = quad_bcast<1>(o);
  fp2 y3, s1j2;
  fp2_add(s1j2, s1j, s1j);
  fp2_sub(y3, y3a, s1j2);
  r.x = x3;
  r.y = y3;
  r.z = z3;
}

// The called forms: the scalar multiplications below loop over them, and an inlined copy per call site would only
// grow the code (the operands are 288 bytes each either way).
__device__ __noinline__ void g2_dbl_quad_call(g2j& r, const g2j& p_in, int q) {
  const g2j p = p_in;
  g2j t;
  g2_dbl_quad(t, p, q);
  r = t;
}
__device__ __noinline__ void g2_add_quad_call(g2j& r, const g2j& p_in, const g2j& q_in, int q) {
  const g2j p = p_in, qp = q_in;
  g2j t;
  g2_add_quad(t, p, qp, q);
  r = t;
}

// ---------------------------------------------------------------- the lone sigagg route (hipbls.hip use_tagg_lat)
// ops.h g2_subgroup_and_mul_i64 with its doublings and additions on the quad: the points 2^i sig (i < 64) serve both
// [|x|] sig (the explicit G2 membership test psi(sig) == [x] sig: a partial meets no Miller loop before it is summed)
// and [|c|] sig.  63 doublings of three products and ~24 additions of five, instead of seven and sixteen.  Returns
// whether sig is in G2 (sig affine, not infinity).
__device__ __noinline__ bool g2_subgroup_and_mul_i64_quad(g2j& out, const g2j& sj, int64_t c, int q) {
  const uint64_t k = c < 0 ? (uint64_t)0 - (uint64_t)c : (uint64_t)c;
  g2j pw = sj, ax, ac;
  jac_set_inf(ax);
  jac_set_inf(ac);
  for (int i = 0; i < 64; ++i) {
    if ((X_ABS >> i) & 1ull) g2_add_quad_call(ax, ax, pw, q);
    if ((k >> i) & 1ull) g2_add_quad_call(ac, ac, pw, q);  // octet-uniform
    if (i < 63 && ((X_ABS | k) >> (i + 1)) != 0) g2_dbl_quad_call(pw, pw, q);
  }
  if (c < 0) {
    g2j t = ac;
    jac_neg(ac, t);
  }
  out = ac;
  g2j nq, ps;
  jac_neg(nq, ax);  // [x] sig, x < 0
  g2_psi(ps, sj);
  return jac_eq(nq, ps);
}

// curve.h g2_mul_glv4 (the four-dimensional GLS split, 64 doublings and <= 64 additions over a 16-entry table) with
// the table's additions, the doublings and the additions on the quad.
__device__ __noinline__ void g2_mul_glv4_quad(g2j& r, const g2j& p_in, const uint32_t* k_plain, int q) {
  const g2j p = p_in;
  uint32_t k[8];
  for (int i = 0; i < 8; ++i) k[i] = k_plain[i];
  uint64_t e[4];
  for (int i = 0; i < 3; ++i) e[i] = u256_divmod_xabs(k);
  e[3] = (uint64_t)k[0] | ((uint64_t)k[1] << 32);
  g2j tab[16];
  jac_set_inf(tab[0]);
  tab[1] = p;                   // P
  g2_psi(tab[2], tab[1]);
  jac_neg(tab[2], tab[2]);      // -psi(P)
  g2_psi2(tab[4], tab[1]);      // psi^2(P)
  g2_psi(tab[8], tab[4]);
  jac_neg(tab[8], tab[8]);      // -psi^3(P)
  for (int d = 3; d < 16; ++d) {
    const int low = d & -d;
    if (d != low) g2_add_quad_call(tab[d], tab[d ^ low], tab[low], q);
  }
  g2j acc;
  jac_set_inf(acc);
  for (int bit = 63; bit >= 0; --bit) {
    if (!jac_is_inf(acc)) g2_dbl_quad_call(acc, acc, q);  // the same on every lane of the octet
    const int d = (int)((e[0] >> bit) & 1u) | (int)(((e[1] >> bit) & 1u) << 1) |
                  (int)(((e[2] >> bit) & 1u) << 2) | (int)(((e[3] >> bit) & 1u) << 3);
    if (d) g2_add_quad_call(acc, acc, tab[d], q);
  }
  r = acc;
}

// kernels.h tagg_scale_lane on an octet: partial k's decode, explicit subgroup test and [c_k] sig_k (small ids) on the
// quad; the groups whose ids leave the small-integer path (ops.h lagrange_small) take tagg_scale_point's field-path
// formulas, the same on all eight lanes.  The lead lane writes the status and the scaled point as tagg_scale_lane does.
__device__ __forceinline__ void tagg_scale_octet(uint64_t k, int q, bool lead, const uint8_t* __restrict__ sigs,
                                                 const int64_t* __restrict__ ids, const uint64_t* __restrict__ goffs,
                                                 uint64_t n_groups, uint64_t n_parts, uint32_t* __restrict__ pts,
                                                 int32_t* __restrict__ pstat) {
  uint64_t lo = 0, hi = n_groups;  // find g with goffs[g] <= k < goffs[g+1]
  while (hi - lo > 1) {
    const uint64_t mid = (lo + hi) / 2;
    if (goffs[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t g0 = goffs[lo], g1 = goffs[lo + 1];
  const int t = (int)(g1 - g0);
  const int me = (int)(k - g0);
  g2j acc;
  jac_set_inf(acc);
  int st = HIPBLS_OK;
  for (int a = 0; a < t; ++a) {  // ids non-zero and distinct within the group (herumi Recover fails otherwise)
    if (ids[g0 + a] == 0) st = HIPBLS_ERR_COMBINE;
    for (int b = a + 1; b < t; ++b)
      if (ids[g0 + a] == ids[g0 + b]) st = HIPBLS_ERR_COMBINE;
  }
  g2a s;
  int64_t c;
  uint64_t L;
  const bool small = st == HIPBLS_OK && lagrange_small(ids + g0, t, me, c, L);
  int ds = g2_decompress(s, sigs + 96 * k, !small);
  if (small && ds == DEC_OK) {
    g2j sj;
    jac_from_aff(sj, s);
    if (!g2_subgroup_and_mul_i64_quad(acc, sj, c, q)) {
      ds = DEC_BAD;
      jac_set_inf(acc);
    }
  }
  if (ds == DEC_BAD) st = HIPBLS_ERR_SIGNATURE;
  if (st == HIPBLS_OK && ds == DEC_OK && !small) {
    g2j sj;
    jac_from_aff(sj, s);
    tagg_scale_point(acc, sj, ids + g0, t, me);  // lambda_k sig_k (field path)
  }
  if (lead) {
    soa_store<72>(pts, n_parts, k, &acc.x.c0.v[0]);
    pstat[k] = st;
  }
}

// Group g's status composed in k_tagg_sum_s's order (empty: cannot combine; any ERR_SIGNATURE before any combine
// error) and, when it is OK, S = the sum of its scaled partials: a chain of quad additions in the partials' order.
// Returns the status; every lane of the octet ends with the same S.
__device__ __forceinline__ int tagg_sum_octet(g2j& acc, const uint32_t* __restrict__ pts,
                                              const int32_t* __restrict__ pstat, const uint64_t* __restrict__ goffs,
                                              uint64_t g, uint64_t n_parts, int q) {
  const uint64_t g0 = goffs[g], g1 = goffs[g + 1];
  int st = g1 > g0 ? HIPBLS_OK : HIPBLS_ERR_COMBINE;
  for (uint64_t k = g0; k < g1; ++k)
    if (pstat[k] == HIPBLS_ERR_SIGNATURE) st = HIPBLS_ERR_SIGNATURE;
  if (st == HIPBLS_OK)
    for (uint64_t k = g0; k < g1; ++k)
      if (pstat[k] != HIPBLS_OK) st = pstat[k];
  jac_set_inf(acc);
  if (st == HIPBLS_OK) {
    for (uint64_t k = g0; k < g1; ++k) {
      g2j p;
      soa_load<72>(&p.x.c0.v[0], pts, n_parts, k);
      g2_add_quad_call(acc, acc, p, q);
    }
  }
  return st;
}

// kernels.h tagg_unscale_lane on an octet: sigma = [L^-1] S on the small-integer path (S itself otherwise), compressed;
// zeros for a group that did not combine, c0 00.. for an aggregate at infinity.  S as tagg_sum_octet left it.
__device__ __forceinline__ void tagg_unscale_octet(const g2j& S, int st, uint64_t g, const int64_t* __restrict__ ids,
                                                   const uint64_t* __restrict__ goffs, uint8_t* __restrict__ out,
                                                   int q, bool lead) {
  g2j acc;
  jac_set_inf(acc);
  if (st == HIPBLS_OK && !jac_is_inf(S)) {
    acc = S;
    const uint64_t g0 = goffs[g], g1 = goffs[g + 1];
    int64_t c;
    uint64_t L;
    if (lagrange_small(ids + g0, (int)(g1 - g0), 0, c, L)) {  // ops.h tagg_unscale
      fr lf, li, plain;
      fr_from_i64(lf, (int64_t)L);
      fr_inv(li, lf);
      fr_to_plain(plain, li);
      g2_mul_glv4_quad(acc, S, plain.v, q);
    }
  }
  uint8_t sig[96];
  g2_compress(sig, acc);
  if (lead)
    for (int b = 0; b < 96; ++b) out[96 * g + b] = st == HIPBLS_OK ? sig[b] : (uint8_t)0;
}

}  // namespace bls
