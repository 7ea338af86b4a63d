// Host build of sigagg's key role (tests/test_sigagg_keys_static.py): the lane body the keyed kernels run
// (charon_amd/csrc/rlc.h tv_key_lane, over a table built by pubtab_load_lane) beside the wire-format lane's steps
// (kernels.h k_tv_prep_pk: g1_decompress + subgroup test, then g1_scale_affine by the group's L).  Test-only.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../charon_amd/csrc/ops.h"
#include "../../charon_amd/csrc/rlc.h"

using namespace bls;

extern "C" {

// Loads tab_pks[0..T) into a table (load_status[k] as hipbls_pubshare_table_load) and runs the keyed lane for entry k
// and the group's t ids.  Returns the lane's status (-1 pending); out24 = [L] pk when pending, zeros otherwise.
int sk_keyed_lane(const uint8_t* tab_pks, uint64_t T, uint64_t k, const int64_t* ids, int t, uint32_t* out24,
                  int32_t* load_status) {
  std::vector<int32_t> code(T ? T : 1);
  std::vector<uint32_t> tab((T ? T : 1) * PUBTAB_WORDS);
  for (uint64_t j = 0; j < T; ++j) load_status[j] = pubtab_load_lane(j, tab_pks, T, code.data(), tab.data());
  g1a pk;
  memset(out24, 0, 24 * sizeof(uint32_t));
  const int st = tv_key_lane(pk, k, T, code.data(), tab.data(), ids, t);
  if (st == RLC_PENDING) memcpy(out24, &pk.x.v[0], 24 * sizeof(uint32_t));
  return st;
}

// The wire-format lane for the same key bytes.
int sk_wire_lane(const uint8_t* pk48, const int64_t* ids, int t, uint32_t* out24) {
  memset(out24, 0, 24 * sizeof(uint32_t));
  g1a pk;
  const int dp = g1_decompress(pk, pk48, true);
  if (dp == DEC_BAD) return HIPBLS_ERR_PUBKEY;
  if (dp == DEC_INF) return HIPBLS_ERR_VERIFY;
  g1_scale_affine(pk, tagg_group_L(ids, t));
  memcpy(out24, &pk.x.v[0], 24 * sizeof(uint32_t));
  return RLC_PENDING;
}

}  // extern "C"
