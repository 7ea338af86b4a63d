// Secret-independent ThresholdSplit / RecoverSecret kernels in batches (deal_ct.h) in a translation
// unit of their own, namespace bls_deal: the out-of-line callees are this unit's private copies, so adding these
// kernels leaves every other code object of the library as it was.  C linkage, launched by hipbls.hip.
//
//   k_g1_comb_build  once per context: T[w][j-1] = [j 16^w] g1, affine, Montgomery (public, variable-time).
//   k_deal_ct        one lane per (validator v, k = 0..total): f_v(k) by Horner, [f_v(k)] g1 over the comb, compressed.
//   k_recover_plan   the launch's largest group size (public), the uniform trip count of k_recover_ct.
//   k_recover_ct     one lane per group: sum of lambda_k s_k, then the public key of the recovered secret.
//
// k_deal_ct and k_recover_ct run ONE instruction stream on every lane and hold no branch on a vector condition at
// all.  A lane beyond the end works on the last item's data.  The stores are not skipped but steered: a lane whose
// public position says "no store" (i >= n; k = 0 for the share bytes; k != 0 for the validator's status) writes zeros
// to the context's 64-byte sink instead, so the guard is an address select on public values, not a branch.  Whether
// public keys are wanted at all is a kernel argument, the same for the whole launch (a scalar branch).
#define bls bls_deal
#include <hip/hip_runtime.h>

#include "rlc.h"
#include "deal_ct.h"

constexpr int kDealBlock = 64;  // hipbls.hip kBlock

extern "C" __global__ void __launch_bounds__(kDealBlock) k_g1_comb_build(uint32_t* __restrict__ T) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (uint32_t)(bls::COMB_WINDOWS * 15)) return;
  uint32_t e[24];
  bls::comb_build_entry(e, (int)(i / 15u), (int)(i % 15u) + 1);
  for (int k = 0; k < 24; ++k) T[24 * i + k] = e[k];
}

// A mask the compiler knows nothing about (it must not turn the steered stores below back into a guarded block).
__device__ __forceinline__ uint32_t opaque_mask(uint32_t m) {
  asm volatile("" : "+v"(m));
  return m;
}
// m ? real : sink as address arithmetic on public values (global address space)
template <class P>
__device__ __forceinline__ P* steer(P* real, uint8_t* sink, uint32_t m) {
  const uint64_t a = (uint64_t)real, s = (uint64_t)sink, mm = ((uint64_t)m << 32) | m;
  return (P*)(__attribute__((address_space(1))) P*)(s ^ ((a ^ s) & mm));
}

// n = n_val (total + 1) lanes, n < 2^31 (the host checks).  sink: 64 writable bytes nobody reads.
extern "C" __global__ void __launch_bounds__(kDealBlock)
k_deal_ct(const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ tails, uint32_t n, uint32_t total,
          uint32_t threshold, const uint32_t* __restrict__ T, uint8_t* __restrict__ out_shares,
          int32_t* __restrict__ status, uint8_t* __restrict__ out_pubs, int32_t* __restrict__ pub_status,
          uint8_t* __restrict__ sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t in = opaque_mask(i < n ? ~0u : 0u);
  const uint32_t j = (i & in) | ((n - 1u) & ~in);  // n >= 1: every lane reads inside the arrays
  const uint32_t v = j / (total + 1u), k = j - v * (total + 1u);
  uint8_t share[32];
  bls::fr scalar;
  uint32_t ok;
  const int st = bls::op_deal_ct(share, scalar, ok, secrets + 32 * (uint64_t)v,
                                 tails + 32 * (uint64_t)(threshold - 1u) * v, threshold, k);
  // the share bytes: lanes k >= 1
  const uint32_t ms = in & opaque_mask(k >= 1u ? ~0u : 0u);
  uint8_t* const ds = steer(out_shares + 32 * ((uint64_t)total * v + (k - 1u)), sink, ms);
#pragma unroll
  for (int b = 0; b < 32; ++b) ds[b] = (uint8_t)(share[b] & ms);
  // the validator's status: lane k = 0
  const uint32_t mv = in & ~ms;
  *steer(status + v, sink + 48, mv) = (int32_t)((uint32_t)st & mv);
  if (out_pubs != nullptr) {  // a kernel argument: the same for every lane of the launch
    uint8_t pub[48];
    const int pst = bls::g1_pub_ct(pub, BLS_COMB_PTR(T), scalar, ok);
    uint8_t* const dp = steer(out_pubs + 48 * (uint64_t)i, sink, in);
#pragma unroll
    for (int b = 0; b < 48; ++b) dp[b] = (uint8_t)(pub[b] & in);
    *steer(pub_status + i, sink + 52, in) = (int32_t)((uint32_t)pst & in);
  }
}

// *m_max (zeroed by the host) = the largest group size of the launch.  Public.
extern "C" __global__ void __launch_bounds__(kDealBlock)
k_recover_plan(const uint64_t* __restrict__ offs, uint32_t n_groups, uint32_t* __restrict__ m_max) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= n_groups) return;
  atomicMax(m_max, (uint32_t)(offs[g + 1] - offs[g]));
}

// n_groups >= 1.  n_parts = offs[n_groups]; with n_parts = 0 every group is empty, *m_max is 0 and nothing is read.
extern "C" __global__ void __launch_bounds__(kDealBlock)
k_recover_ct(const uint8_t* __restrict__ shares, const int64_t* __restrict__ ids, const uint64_t* __restrict__ offs,
             uint32_t n_groups, uint32_t n_parts, const uint32_t* __restrict__ m_max_p, const uint32_t* __restrict__ T,
             uint8_t* __restrict__ out_secrets, int32_t* __restrict__ status, uint8_t* __restrict__ out_pubkeys,
             int32_t* __restrict__ pk_status, uint8_t* __restrict__ sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t in = opaque_mask(i < n_groups ? ~0u : 0u);
  const uint32_t g = (i & in) | ((n_groups - 1u) & ~in);
  const uint32_t m_max = __builtin_amdgcn_readfirstlane(*m_max_p);
  const uint32_t last = n_parts - 1u;  // unused when n_parts = 0 (m_max = 0)
  const uint32_t g0 = (uint32_t)offs[g], m = (uint32_t)offs[g + 1] - g0;
  const uint32_t base = g0 < n_parts ? g0 : last;  // an empty group at the very end still points inside the arrays
  const int ids_status = bls::recover_ids_status(ids + base, m);  // reads m ids: none when every group is empty
  bls::fr acc;
  for (int w = 0; w < 8; ++w) acc.v[w] = 0;
  uint32_t ok = ~0u;
#pragma unroll 1
  for (uint32_t k = m_max; k != 0u; --k) {  // the launch's largest group, highest share first
    const uint32_t kx = k - 1u;
    const uint32_t act = opaque_mask(kx < m ? ~0u : 0u);  // public: the lane's group has this share
    const uint32_t kk = kx & act;
    bls::fr lam;
    bls::lagrange_at_zero(lam, ids + base, (int)(m & act), (int)kk);
    bls::recover_term_ct(acc, ok, lam, shares + 32 * (uint64_t)(base + kk), act);
  }
  uint8_t sec[32];
  bls::fr secret;
  uint32_t keep;
  const int st = bls::recover_finish_ct(sec, secret, keep, acc, ids_status, ok);
  uint8_t* const ds = steer(out_secrets + 32 * (uint64_t)i, sink, in);
#pragma unroll
  for (int b = 0; b < 32; ++b) ds[b] = (uint8_t)(sec[b] & in);
  *steer(status + i, sink + 48, in) = (int32_t)((uint32_t)st & in);
  if (out_pubkeys != nullptr) {  // a kernel argument: the same for every lane of the launch
    uint8_t pub[48];
    const int pst = bls::g1_pub_ct(pub, BLS_COMB_PTR(T), secret, keep);
    uint8_t* const dp = steer(out_pubkeys + 48 * (uint64_t)i, sink, in);
#pragma unroll
    for (int b = 0; b < 48; ++b) dp[b] = (uint8_t)(pub[b] & in);
    *steer(pk_status + i, sink + 52, in) = (int32_t)((uint32_t)pst & in);
  }
}
