// Test-only host library (tests/native/libfp_units_host.so): the host build of fp_pow (field.h) on raw limbs, the
// reference of tests/test_gpu_fp_sqr.py for the device's square-root chains.
#include "../../charon_amd/csrc/field.h"

using namespace bls;

extern "C" void fpuh_pow(const uint32_t* in, uint32_t* out, uint32_t count, int minus1) {
  for (uint32_t i = 0; i < count; ++i) {
    fp a, r;
    for (int k = 0; k < 12; ++k) a.v[k] = in[12 * i + k];
    fp_pow(r, a, minus1 ? EXP_SQRT_M1 : EXP_SQRT, 378);
    for (int k = 0; k < 12; ++k) out[12 * i + k] = r.v[k];
  }
}
