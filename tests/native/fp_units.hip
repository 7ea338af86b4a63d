// Test-only GPU library (tests/native/libfp_units.so): the device Fp squaring routine and fp_pow on raw operands,
// one lane per element, for tests/test_gpu_fp_sqr.py.  Not part of the product.
// Elements cross the ABI as 12 little-endian 32-bit limbs, untouched: the routines see exactly the limbs given (lazy
// operands in [p, 2^382) included), and a result is Montgomery's a*a/2^384 mod p of those limbs.
//   op 0  fp_sqr(a)                       the single entry
//   op 1  fp_mul(a, a)                    the product routine on the same lane
//   op 2  fp_sqr_n(a, n)                  the run entry
//   op 3  n calls of fp_sqr
//   op 4  fp_pow(a, (p + 1) / 4)          the square-root chain of fp_sqrt and hash-to-G2
//   op 5  fp_pow(a, (p - 3) / 4)          the chain of the G2 decompression
#include <hip/hip_runtime.h>

#include "field.h"

using namespace bls;

namespace {

__global__ void __launch_bounds__(64) k_fpu(const uint32_t* in, uint32_t* out, uint32_t lanes, int op, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= lanes) return;
  fp a, r;
  for (int k = 0; k < 12; ++k) a.v[k] = in[12 * i + k];
  if (op == 0) {
    fp_sqr(r, a);
  } else if (op == 1) {
    fp_mul(r, a, a);
  } else if (op == 2) {
    fp_sqr_n(r, a, n);
  } else if (op == 3) {
    r = a;
#pragma unroll 1
    for (uint32_t t = 0; t < n; ++t) fp_sqr(r, r);
  } else if (op == 4) {
    fp_pow(r, a, EXP_SQRT, 378);
  } else {
    fp_pow(r, a, EXP_SQRT_M1, 378);
  }
  for (int k = 0; k < 12; ++k) out[12 * i + k] = r.v[k];
}

int check(hipError_t e) { return e == hipSuccess ? 0 : 1; }

}  // namespace

extern "C" int fpu_run(const uint32_t* in, uint32_t* out, uint32_t lanes, int op, uint32_t n) {
  if (!lanes || op < 0 || op > 5 || ((op == 2 || op == 3) && !n)) return 2;
  const size_t bytes = 48 * (size_t)lanes;
  uint32_t *din = nullptr, *dout = nullptr;
  if (check(hipMalloc(&din, bytes)) || check(hipMalloc(&dout, bytes))) return 1;
  int rc = check(hipMemcpy(din, in, bytes, hipMemcpyHostToDevice));
  if (!rc) {
    hipLaunchKernelGGL(k_fpu, dim3((lanes + 63) / 64), dim3(64), 0, 0, din, dout, lanes, op, n);
    rc = check(hipGetLastError()) || check(hipDeviceSynchronize()) ||
         check(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
  }
  (void)hipFree(din);
  (void)hipFree(dout);
  return rc;
}
