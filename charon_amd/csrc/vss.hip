// PublicKeyShare / PublicKeyRecover kernels in batches (vss.h) in a translation unit of their own,
// namespace bls_vss: the out-of-line callees are this unit's private copies, so adding these kernels leaves every other
// code object of the library as it was.  C linkage, launched by hipbls.hip.  Public data only.
//
//   k_vss_dealer_sum  one lane per (validator v, coefficient j): the n_dealers decoded commitments added (joint dealing).
//   k_vss_eval        one lane per (v, id i): sum_j [x_i^j] A[v][j] by Horner with complete additions, compressed.
//   k_vss_scale       one lane per pubshare: decode + subgroup test, then [c_k] P or [lambda_k] P.
//   k_vss_sum         one lane per group: the sum, [L^-1] of it on the small-integer path, compressed.
//
// The commitments of a share call are decoded by hipbls.hip's k_g1_decode, one lane per point.  A lane beyond the end
// returns before any load; every other lane reads and writes inside its call's arrays.
#define bls bls_vss
#include <hip/hip_runtime.h>

#include "vss.h"

constexpr int kVssBlock = 64;  // hipbls.hip kBlock

// n = n_val threshold lanes
extern "C" __global__ void __launch_bounds__(kVssBlock)
k_vss_dealer_sum(const uint32_t* __restrict__ pts, const int32_t* __restrict__ code, uint32_t n, uint32_t n_dealers,
                 uint32_t threshold, uint32_t* __restrict__ out_pts, int32_t* __restrict__ out_code) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  bls::vss_dealer_sum_lane(out_pts, out_code, n, pts, code, (uint64_t)n * n_dealers, i / threshold, n_dealers, threshold,
                           i % threshold);
}

// n = n_val n_ids lanes, validator fastest (lane = i n_val + v): the lanes of a wave share their id, so the
// double-and-add over the id's bits is one path for the wave.  n_pts = n_val threshold.
extern "C" __global__ void __launch_bounds__(kVssBlock)
k_vss_eval(const uint32_t* __restrict__ pts, const int32_t* __restrict__ code, uint32_t n_val, uint32_t threshold,
           const int64_t* __restrict__ ids, uint32_t n_ids, uint8_t* __restrict__ out_pubs,
           int32_t* __restrict__ status) {
  const uint32_t l = blockIdx.x * blockDim.x + threadIdx.x;
  if (l >= n_val * n_ids) return;
  const uint32_t i = l / n_val, v = l - i * n_val;
  uint8_t pub[48];
  const int st = bls::vss_eval_lane(pub, pts, code, (uint64_t)n_val * threshold, v, threshold, ids[i]);
  uint8_t* const d = out_pubs + 48 * ((uint64_t)v * n_ids + i);
  for (int b = 0; b < 48; ++b) d[b] = pub[b];
  if (i == 0) status[v] = st;
}

// n_parts >= 1 lanes over n_groups >= 1 groups
extern "C" __global__ void __launch_bounds__(kVssBlock)
k_vss_scale(const uint8_t* __restrict__ shares, const int64_t* __restrict__ ids, const uint64_t* __restrict__ goffs,
            uint32_t n_groups, uint32_t n_parts, uint32_t* __restrict__ pts, int32_t* __restrict__ pstat) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= n_parts) return;
  uint32_t lo = 0, hi = n_groups;  // find g with goffs[g] <= k < goffs[g+1]
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) / 2;
    if (goffs[mid] <= k)
      lo = mid;
    else
      hi = mid;
  }
  const uint64_t g0 = goffs[lo];
  bls::g1j p;
  pstat[k] = bls::vss_scale_lane(p, shares + 48 * (uint64_t)k, ids + g0, (int)(goffs[lo + 1] - g0), (int)(k - g0));
  bls::soa_store<36>(pts, n_parts, k, &p.x.v[0]);
}

extern "C" __global__ void __launch_bounds__(kVssBlock)
k_vss_sum(const uint32_t* __restrict__ pts, const int32_t* __restrict__ pstat, const int64_t* __restrict__ ids,
          const uint64_t* __restrict__ goffs, uint32_t n_groups, uint32_t n_parts, uint8_t* __restrict__ out,
          int32_t* __restrict__ status) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  const uint64_t g0 = goffs[g];
  uint8_t pub[48];
  // an empty group reads no id and no point (its status is decided by t = 0)
  status[g] = bls::vss_sum_lane(pub, pts, pstat, n_parts, g0, ids + g0, (int)(goffs[g + 1] - g0));
  uint8_t* const d = out + 48 * (uint64_t)g;
  for (int b = 0; b < 48; ++b) d[b] = pub[b];
}
