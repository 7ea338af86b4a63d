// FastAggregateVerify's two key sources and two H(m) sources, as the loaders that the shared bodies
// of the check kernels are templated on (verify_hex.hip fav_pair_lq16_body, kernels.h fav_batch_body), so that the
// wire-format kernels and their `_keys` twins cannot drift apart:
//   * fav_wire_keys: key k of the call, decoded by k_fav_prep8 / k_g1_decode (affine SoA with stride nkeys, DEC_* code);
//   * fav_tab_keys:  key k of the call is table[key_idx[k]] of the resident pubshare table (rlc.h PUBTAB_WORDS: the 24
//     affine words first, the DEC_* code in tcode), loaded and subgroup-tested once by hipbls_pubshare_table_load.  A
//     group that the host cut into slices (fav_split.h) comes as Jacobian partial sums instead, one per slice, which
//     kernels.h k_fav_sum_keys folded: partials [poff[g], poff[g + 1]) of `parts` (36 words, SoA over n_slices) with
//     the slice's bad and identity flags in pflags[2 p], pflags[2 p + 1];
//   * fav_h_cols:    group g's H(m) from one of two SoA tables, as kernels.h tv_h_word: column hcol[g] & ~bit 31 of the
//     context's H(m) cache (stride cstride) when bit 31 is set, else column hcol[g] of the call's own table Hc (stride
//     hstride); without hcol (the _device call: one hash per group) column g of Hc.
// fav_fold is the one strided key sum of all of them: 64 lanes, lane tid takes keys k0 + tid, k0 + tid + 64, ...
#pragma once
#include "rlc.h"

namespace bls {

constexpr int FAV_KEY_ARG = 4;  // beside DEC_OK / DEC_BAD / DEC_INF: a key index outside the table
constexpr uint32_t kFavHCached = 0x80000000u;

struct fav_wire_keys {
  static constexpr bool kIndexed = false;
  const uint32_t* pts;
  const int32_t* kcode;
  uint64_t nkeys;
  __device__ __forceinline__ int code(uint64_t k, uint64_t& col) const {
    col = k;
    return kcode[k];
  }
  __device__ __forceinline__ void point(g1a& a, uint64_t col) const { soa_load<24>(&a.x.v[0], pts, nkeys, col); }
};

struct fav_tab_keys {
  static constexpr bool kIndexed = true;
  const uint32_t* key_idx;
  uint64_t T;
  const int32_t* tcode;
  const uint32_t* tab;
  // the split key sum's partials (poff == nullptr: no group of the call was cut)
  const uint64_t* poff;
  const uint32_t* parts;
  const int32_t* pflags;
  uint64_t n_slices;
  __device__ __forceinline__ int code(uint64_t k, uint64_t& col) const {
    col = key_idx[k];
    return col < T ? tcode[col] : FAV_KEY_ARG;  // the loads stay inside the table
  }
  __device__ __forceinline__ void point(g1a& a, uint64_t col) const { soa_load<24>(&a.x.v[0], tab, T, col); }
};

// Lane tid's share of the keys [k0, k1) added into acc (mixed additions; a repeated key doubles), bad |= 1 for a key
// that failed to decode or load, bad |= 2 for an index outside the table, inf = 1 for the identity key.
template <class Keys>
__device__ __forceinline__ void fav_fold(g1j& acc, int& bad, int& inf, const Keys& keys, uint64_t k0, uint64_t k1,
                                         int tid) {
  for (uint64_t k = k0 + tid; k < k1; k += 64) {
    uint64_t col;
    const int c = keys.code(k, col);
    if (c == DEC_BAD) {
      bad |= 1;
    } else if (c == DEC_INF) {
      inf = 1;
    } else if (Keys::kIndexed && c == FAV_KEY_ARG) {
      bad |= 2;
    } else {
      g1a a;
      keys.point(a, col);
      jac_add_aff(acc, acc, a);
    }
  }
}

// Group g's key sum on lane tid: its slices' partials where the host cut it, else its keys [k0, k1).
template <class Keys>
__device__ __forceinline__ void fav_fold_group(g1j& acc, int& bad, int& inf, const Keys& keys, uint64_t g, uint64_t k0,
                                               uint64_t k1, int tid) {
  if constexpr (Keys::kIndexed) {
    const uint64_t p0 = keys.poff ? keys.poff[g] : 0, p1 = keys.poff ? keys.poff[g + 1] : 0;
    if (p1 > p0) {
      for (uint64_t p = p0 + tid; p < p1; p += 64) {
        bad |= keys.pflags[2 * p];
        inf |= keys.pflags[2 * p + 1];
        g1j x;
        soa_load<36>(&x.x.v[0], keys.parts, keys.n_slices, p);
        jac_add(acc, acc, x);
      }
      return;
    }
  }
  fav_fold(acc, bad, inf, keys, k0, k1, tid);
}

// The LDS tree over the 64 lanes' Jacobian sums in red (36 words, SoA over 64): the total ends in column 0.  Every
// thread of the workgroup calls it and reaches every barrier.
__device__ __forceinline__ void fav_tree(uint32_t* red, int tid) {
  for (int half = 32; half >= 1; half >>= 1) {
    if (tid < half) {
      g1j x, y;
      for (int w = 0; w < 36; ++w) {
        (&x.x.v[0])[w] = red[w * 64 + tid];
        (&y.x.v[0])[w] = red[w * 64 + tid + half];
      }
      jac_add(x, x, y);
      for (int w = 0; w < 36; ++w) red[w * 64 + tid] = (&x.x.v[0])[w];
    }
    __syncthreads();
  }
}

struct fav_h_cols {
  const uint32_t* hcol;
  const uint32_t* Hcache;
  uint64_t cstride;
  const uint32_t* Hc;
  uint64_t hstride;
  __device__ __forceinline__ void load(g2a& hm, uint64_t g) const {
    const uint32_t src = hcol ? hcol[g] : (uint32_t)g;
    if (src & kFavHCached)
      soa_load<48>(&hm.x.c0.v[0], Hcache, cstride, src & ~kFavHCached);
    else
      soa_load<48>(&hm.x.c0.v[0], Hc, hstride, src);
  }
};

}  // namespace bls
