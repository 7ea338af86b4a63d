// Test-only GPU library (tests/native/libgpu_units_pair.so): the split-Fp2 build of the field and tower headers
// (BLS_FP2_PAIR, as charon_amd/csrc/verify_lat.hip sets it), for tests/test_gpu_arith_layers.py.  Not part of the
// product.  An Fp2 value is held in full on lanes l and l ^ 4; each lane forms one coefficient of a product or square
// and one DPP exchange gives both the whole result.  Four cases share a group of eight lanes (case 4 g + (l & 3) on
// lanes l and l ^ 4 of group g), and BOTH lanes' results are returned, so the test sees that the twins agree.
//   op 0  fp2_mul(a, b)      op 1  fp2_sqr(a)      op 2  fp2_mul_fp(a, b.c0)
//   op 3  fp_pow(a.c0, (p + 1) / 4)      op 4  fp_pow(a.c0, (p - 3) / 4)      (fp_pow_twin: the twins share one chain)
// In: a.c0 a.c1 b.c0 b.c1 as raw 12 x u32 Montgomery limbs (48 words per case); out: 2 x (r.c0 r.c1) (48 words per
// case: the c0-side lane's result, then its twin's).  The exchanges need all eight lanes of a group active: a group
// leaves as a whole, and in a partial last group the lanes past n run the last case again and store nothing.
#define BLS_FP2_PAIR 1
#define bls bls_fp2p
#include <hip/hip_runtime.h>

#include "tower.h"

using namespace bls;

namespace {

__global__ void __launch_bounds__(64) k_gup(const uint32_t* in, uint32_t* out, uint32_t n, int op) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t grp = t >> 3, w = t & 7;
  if (grp * 4 >= n) return;  // uniform over the group's eight lanes
  uint32_t i = grp * 4 + (w & 3);
  const bool live = i < n;
  if (!live) i = n - 1;
  fp2 a, b, r;
  for (int k = 0; k < 12; ++k) {
    a.c0.v[k] = in[48 * i + k];
    a.c1.v[k] = in[48 * i + 12 + k];
    b.c0.v[k] = in[48 * i + 24 + k];
    b.c1.v[k] = in[48 * i + 36 + k];
  }
  fp2_set_zero(r);
  if (op == 0)
    fp2_mul(r, a, b);
  else if (op == 1)
    fp2_sqr(r, a);
  else if (op == 2)
    fp2_mul_fp(r, a, b.c0);
  else if (op == 3)
    fp_pow(r.c0, a.c0, EXP_SQRT, 378);
  else
    fp_pow(r.c0, a.c0, EXP_SQRT_M1, 378);
  if (live) {
    uint32_t* o = out + 48 * i + 24 * (w >> 2);
    for (int k = 0; k < 12; ++k) {
      o[k] = r.c0.v[k];
      o[12 + k] = r.c1.v[k];
    }
  }
}

int check(hipError_t e) { return e == hipSuccess ? 0 : 1; }

}  // namespace

extern "C" int gup_run(int op, const uint32_t* in, uint32_t* out, uint32_t n) {
  if (!n || op < 0 || op > 4) return 2;
  const size_t bytes = 192 * (size_t)n;
  uint32_t *din = nullptr, *dout = nullptr;
  if (check(hipMalloc(&din, bytes)) || check(hipMalloc(&dout, bytes))) return 1;
  int rc = check(hipMemcpy(din, in, bytes, hipMemcpyHostToDevice)) || check(hipMemset(dout, 0, bytes));
  if (!rc) {
    const uint32_t lanes = 8 * ((n + 3) / 4);
    hipLaunchKernelGGL(k_gup, dim3((lanes + 63) / 64), dim3(64), 0, 0, din, dout, n, op);
    rc = check(hipGetLastError()) || check(hipDeviceSynchronize()) ||
         check(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}
