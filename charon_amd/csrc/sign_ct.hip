// Secret-independent Sign and SecretToPublicKey kernels (sign_ct.h) in a translation unit of their
// own, namespace bls_ct: the out-of-line callees (the Fp routines, fp_inv, jac_to_aff, the table-building jac_add,
// hash_to_g2) are this unit's private copies, so adding these kernels leaves every other code object of the library
// as it was.  The kernels have C linkage so that hipbls.hip can launch them.
//
//   k_sign_ct_hash  one lane per item: H(m) = hash_to_g2(msg, DST_POP), Jacobian, limb-major SoA (72 words x n).
//                   The message is public; this is the existing hashing code.
//   k_sign_ct_mul   one lane per item, the only Sign kernel that sees sk: [sk] H(m), compressed, with the status.
//   k_sk_to_pk_ct   one lane per item: [sk] g1, compressed, with the status.
//
// The two kernels that see a secret run ONE instruction stream on every lane: a lane beyond n works on item n - 1's
// data, a lane with a bad secret works on whatever its bytes decode to, and only the final stores are guarded (by
// the public i < n); a bad status zero-fills the output by mask.
#define bls bls_ct
#include <hip/hip_runtime.h>

#include "rlc.h"
#include "sign_ct.h"

constexpr int kCtBlock = 64;  // hipbls.hip kBlock

extern "C" __global__ void __launch_bounds__(kCtBlock)
k_sign_ct_hash(const uint8_t* __restrict__ msgs, const uint64_t* __restrict__ offs, uint64_t n,
               uint32_t* __restrict__ H) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t o0 = offs[i], o1 = offs[i + 1];
  bls::g2j h;
  bls::hash_to_g2(h, msgs + o0, (uint32_t)(o1 - o0), bls::DST_POP, 43);
  bls::soa_store<72>(H, n, i, &h.x.c0.v[0]);
}

extern "C" __global__ void __launch_bounds__(kCtBlock)
k_sign_ct_mul(const uint8_t* __restrict__ sks, const uint32_t* __restrict__ H, uint64_t n,
              uint8_t* __restrict__ out, int32_t* __restrict__ status) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t j = i < n ? i : n - 1;  // n >= 1: every lane reads inside the arrays
  bls::g2j h;
  bls::soa_load<72>(&h.x.c0.v[0], H, n, j);
  uint8_t sk[32], sig[96];
  for (int k = 0; k < 32; ++k) sk[k] = sks[32 * j + k];
  const int st = bls::op_sign_mul_ct(sig, h, sk);
  if (i < n) {
    for (int k = 0; k < 96; ++k) out[96 * i + k] = sig[k];
    status[i] = st;
  }
}

extern "C" __global__ void __launch_bounds__(kCtBlock)
k_sk_to_pk_ct(const uint8_t* __restrict__ sks, uint64_t n, uint8_t* __restrict__ out, int32_t* __restrict__ status) {
  const uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x;
  const uint64_t j = i < n ? i : n - 1;
  uint8_t sk[32], pk[48];
  for (int k = 0; k < 32; ++k) sk[k] = sks[32 * j + k];
  const int st = bls::op_sk_to_pk_ct(pk, sk);
  if (i < n) {
    for (int k = 0; k < 48; ++k) out[48 * i + k] = pk[k];
    status[i] = st;
  }
}
