// A joint-Feldman dealing round in batches (dkg_ct.h) in a translation unit of its own, namespace
// bls_dkg: the out-of-line callees are this unit's private copies, so adding these kernels leaves every other code
// object of the library as it was.  C linkage, launched by hipbls.hip.
//
//   k_commit_ct       one lane per (validator v, coefficient j): [a_j] g1 over the comb, compressed.
//   k_share_check_ct  one lane per (v, dealer d): [share] g1 over the comb, compressed, against the expected bytes.
//   k_share_sum_ct    one lane per validator: the sum of the included dealers' shares, then its pubshare.
//
// As deal_ct.hip's kernels they run ONE instruction stream on every lane and hold no branch on a vector condition.  A
// lane beyond the end works on the last item's data; its stores are steered to the context's 64-byte sink by address
// arithmetic on public values.  Whether the pubshares are wanted is a kernel argument, the same for the whole launch (a
// scalar branch); "no include mask" is a stride of 0 over one readable byte.  The comb table is the context's
// (k_g1_comb_build).
#define bls bls_dkg
#include <hip/hip_runtime.h>

#include "rlc.h"
#include "dkg_ct.h"

constexpr int kDkgBlock = 64;  // hipbls.hip kBlock

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

// n = n_val threshold lanes, 1 <= n < 2^31 (the host checks).  sink: 64 writable bytes nobody reads.
extern "C" __global__ void __launch_bounds__(kDkgBlock)
k_commit_ct(const uint8_t* __restrict__ secrets, const uint8_t* __restrict__ tails, uint32_t n, uint32_t threshold,
            const uint32_t* __restrict__ T, uint8_t* __restrict__ out_commitments, int32_t* __restrict__ com_status,
            uint8_t* __restrict__ sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t in = opaque_mask(i < n ? ~0u : 0u);
  const uint32_t l = (i & in) | ((n - 1u) & ~in);  // every lane reads inside the arrays
  const uint32_t v = l / threshold, j = l - v * threshold;
  uint8_t com[48];
  const int st = bls::op_commit_ct(com, BLS_COMB_PTR(T), secrets + 32 * (uint64_t)v,
                                   tails + 32 * (uint64_t)(threshold - 1u) * v, threshold, j);
  uint8_t* const dc = steer(out_commitments + 48 * (uint64_t)i, sink, in);
#pragma unroll
  for (int b = 0; b < 48; ++b) dc[b] = (uint8_t)(com[b] & in);
  *steer(com_status + i, sink + 52, in) = (int32_t)((uint32_t)st & in);
}

// n = n_val n_dealers lanes, 1 <= n < 2^31.  expected[48 l ..] and decode_status[l] are k_vss_eval's outputs for the
// commitments of lane l evaluated at the receiver's id: public.
extern "C" __global__ void __launch_bounds__(kDkgBlock)
k_share_check_ct(const uint8_t* __restrict__ shares, const uint8_t* __restrict__ expected,
                 const int32_t* __restrict__ decode_status, uint32_t n, const uint32_t* __restrict__ T,
                 int32_t* __restrict__ status, uint8_t* __restrict__ sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t in = opaque_mask(i < n ? ~0u : 0u);
  const uint32_t l = (i & in) | ((n - 1u) & ~in);
  uint8_t want[48];
  const uint8_t* const e = expected + 48 * (uint64_t)l;
#pragma unroll
  for (int b = 0; b < 48; ++b) want[b] = e[b];
  const int st = bls::op_share_check_ct(BLS_COMB_PTR(T), shares + 32 * (uint64_t)l, want, decode_status[l]);
  *steer(status + i, sink + 48, in) = (int32_t)((uint32_t)st & in);
}

// n_val lanes, 1 <= n_val, n_val n_dealers < 2^31.  include: one public byte per (v, d) with include_stride = 1; for
// "every dealer" the host passes any readable byte (the sink) with include_stride = 0, and the byte read is overridden:
// one loop body, and no test of "was a mask given" inside it.
extern "C" __global__ void __launch_bounds__(kDkgBlock)
k_share_sum_ct(const uint8_t* __restrict__ shares, const uint8_t* include, uint32_t include_stride, uint32_t n_val,
               uint32_t n_dealers, const uint32_t* __restrict__ T, uint8_t* __restrict__ out_shares,
               int32_t* __restrict__ status, uint8_t* __restrict__ out_pubs, int32_t* __restrict__ pub_status,
               uint8_t* sink) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t in = opaque_mask(i < n_val ? ~0u : 0u);
  const uint32_t v = (i & in) | ((n_val - 1u) & ~in);
  const uint32_t base = v * n_dealers;
  bls::fr acc;
  for (int w = 0; w < 8; ++w) acc.v[w] = 0;
  uint32_t ok = ~0u, any = 0u;
  const uint32_t all = include_stride - 1u;  // all ones without a mask
#pragma unroll 1
  for (uint32_t d = 0; d < n_dealers; ++d) {  // the public dealer count
    const uint32_t act = opaque_mask(include[(uint64_t)(base + d) * include_stride] != 0 ? ~0u : 0u) | all;  // public
    any |= act;
    bls::share_sum_term_ct(acc, ok, shares + 32 * (uint64_t)(base + d), act);
  }
  uint8_t sec[32];
  bls::fr sum;
  uint32_t keep;
  const int st = bls::share_sum_finish_ct(sec, sum, keep, acc, any, ok);
  uint8_t* const ds = steer(out_shares + 32 * (uint64_t)i, sink, in);
#pragma unroll
  for (int b = 0; b < 32; ++b) ds[b] = (uint8_t)(sec[b] & in);
  *steer(status + i, sink + 48, in) = (int32_t)((uint32_t)st & in);
  if (out_pubs != nullptr) {  // a kernel argument: the same for every lane of the launch
    uint8_t pub[48];
    const int pst = bls::g1_pub_ct(pub, BLS_COMB_PTR(T), sum, keep);
    uint8_t* const dp = steer(out_pubs + 48 * (uint64_t)i, sink, in);
#pragma unroll
    for (int b = 0; b < 48; ++b) dp[b] = (uint8_t)(pub[b] & in);
    *steer(pub_status + i, sink + 52, in) = (int32_t)((uint32_t)pst & in);
  }
}
