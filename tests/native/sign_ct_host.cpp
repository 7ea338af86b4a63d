// Host program for the secret-independent Sign / SecretToPublicKey lane functions (charon_amd/csrc/sign_ct.h),
// built and run by tests/test_sign_ct_host.py (plain, and under AddressSanitizer + UBSan).
//
//   sign_ct_host <secrets file>
//
// The file lists one secret per line: 64 hex digits (big-endian) and the status the test expects for it (0, or
// HIPBLS_ERR_SECRET for a secret >= r; the test compares every entry with r itself).  Checks:
//   1. op_sign_ct == op_sign and op_sk_to_pk_ct == op_sk_to_pk in status and bytes, three messages;
//   2. with the operation trace (field.h BLS_CT_TRACE) and the product counters reset after the hash, the digest and
//      both counts of op_sign_mul_ct and of op_sk_to_pk_ct are the same for EVERY secret of the list;
//   3. the same instrument around g2_mul_glv4 and jac_mul_limbs tells sk = 1 from sk = r - 1.
#define BLS_COUNT_OPS 1
#define BLS_CT_TRACE 1
#include "../../charon_amd/csrc/sign_ct.h"

#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace bls {
thread_local uint64_t g_fp_mul_count = 0;
thread_local uint64_t g_fp_sqr_count = 0;
thread_local uint64_t g_ct_trace = 0;
}  // namespace bls
using namespace bls;

struct Secret {
  uint8_t b[32];
  int want;
};
struct Trace {
  uint64_t digest, mul, sqr;
  bool operator==(const Trace& o) const { return digest == o.digest && mul == o.mul && sqr == o.sqr; }
};

static int g_fail = 0;
#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      if (g_fail++ < 20) {               \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");               \
      }                                  \
    }                                    \
  } while (0)

static void trace_reset() { g_ct_trace = g_fp_mul_count = g_fp_sqr_count = 0; }
static Trace trace_get() { return Trace{g_ct_trace, g_fp_mul_count, g_fp_sqr_count}; }

static std::string hex(const uint8_t* b, int n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < n; ++i) {
    s += d[b[i] >> 4];
    s += d[b[i] & 15];
  }
  return s;
}

static bool read_secrets(const char* path, std::vector<Secret>& out) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char h[80];
  int want;
  while (std::fscanf(f, "%79s %d", h, &want) == 2) {
    if (std::strlen(h) != 64) {
      std::fclose(f);
      return false;
    }
    Secret s;
    for (int i = 0; i < 32; ++i) {
      unsigned v;
      if (std::sscanf(h + 2 * i, "%2x", &v) != 1) {
        std::fclose(f);
        return false;
      }
      s.b[i] = (uint8_t)v;
    }
    s.want = want;
    out.push_back(s);
  }
  std::fclose(f);
  return true;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: sign_ct_host <secrets file>\n");
    return 2;
  }
  std::vector<Secret> secrets;
  if (!read_secrets(argv[1], secrets) || secrets.empty()) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }

  // the three messages: a 32-byte root, the empty message, 100 bytes
  uint8_t root[32], long_msg[100];
  for (int i = 0; i < 32; ++i) root[i] = (uint8_t)(0xa5 ^ (7 * i));
  for (int i = 0; i < 100; ++i) long_msg[i] = (uint8_t)(i * i + 3);
  const uint8_t* msgs[3] = {root, root /* length 0 */, long_msg};
  const uint32_t lens[3] = {32, 0, 100};

  // 1. bytes and statuses
  size_t n_ok = 0;
  for (int m = 0; m < 3; ++m) {
    for (const Secret& s : secrets) {
      uint8_t a[96], b[96];
      std::memset(a, 0xee, 96);
      std::memset(b, 0xee, 96);
      const int sa = op_sign(a, s.b, msgs[m], lens[m]);
      const int sb = op_sign_ct(b, s.b, msgs[m], lens[m]);
      CHECK(sa == s.want, "op_sign status %d, expected %d, sk %s", sa, s.want, hex(s.b, 32).c_str());
      CHECK(sb == sa, "op_sign_ct status %d != op_sign %d, sk %s msg %d", sb, sa, hex(s.b, 32).c_str(), m);
      if (sa == HIPBLS_OK) {
        CHECK(!std::memcmp(a, b, 96), "op_sign_ct bytes differ, sk %s msg %d:\n  %s\n  %s", hex(s.b, 32).c_str(), m,
              hex(a, 96).c_str(), hex(b, 96).c_str());
        ++n_ok;
      } else {
        uint8_t z = 0;
        for (int i = 0; i < 96; ++i) z |= b[i];
        CHECK(z == 0, "op_sign_ct output not zero-filled on status %d, sk %s", sb, hex(s.b, 32).c_str());
      }
    }
  }
  for (const Secret& s : secrets) {
    uint8_t a[48], b[48];
    std::memset(a, 0xee, 48);
    std::memset(b, 0xee, 48);
    const int sa = op_sk_to_pk(a, s.b);
    const int sb = op_sk_to_pk_ct(b, s.b);
    uint8_t nz = 0;
    for (int i = 0; i < 32; ++i) nz |= s.b[i];
    const int want = nz ? s.want : HIPBLS_ERR_SECRET;
    CHECK(sa == want, "op_sk_to_pk status %d, expected %d, sk %s", sa, want, hex(s.b, 32).c_str());
    CHECK(sb == sa, "op_sk_to_pk_ct status %d != op_sk_to_pk %d, sk %s", sb, sa, hex(s.b, 32).c_str());
    if (sa == HIPBLS_OK) {
      CHECK(!std::memcmp(a, b, 48), "op_sk_to_pk_ct bytes differ, sk %s:\n  %s\n  %s", hex(s.b, 32).c_str(),
            hex(a, 48).c_str(), hex(b, 48).c_str());
    } else {
      uint8_t z = 0;
      for (int i = 0; i < 48; ++i) z |= b[i];
      CHECK(z == 0, "op_sk_to_pk_ct output not zero-filled on status %d, sk %s", sb, hex(s.b, 32).c_str());
    }
  }

  // 2. one operation stream for every secret (the hash of the public message is outside the trace)
  g2j h;
  hash_to_g2(h, root, 32, DST_POP, 43);
  Trace sign_ref{}, pk_ref{};
  for (size_t i = 0; i < secrets.size(); ++i) {
    uint8_t out[96];
    trace_reset();
    (void)op_sign_mul_ct(out, h, secrets[i].b);
    const Trace t = trace_get();
    if (i == 0) sign_ref = t;
    CHECK(t == sign_ref, "op_sign_mul_ct trace differs for sk %s: digest %016llx mul %llu sqr %llu",
          hex(secrets[i].b, 32).c_str(), (unsigned long long)t.digest, (unsigned long long)t.mul,
          (unsigned long long)t.sqr);
    trace_reset();
    (void)op_sk_to_pk_ct(out, secrets[i].b);
    const Trace u = trace_get();
    if (i == 0) pk_ref = u;
    CHECK(u == pk_ref, "op_sk_to_pk_ct trace differs for sk %s: digest %016llx mul %llu sqr %llu",
          hex(secrets[i].b, 32).c_str(), (unsigned long long)u.digest, (unsigned long long)u.mul,
          (unsigned long long)u.sqr);
  }
  CHECK(sign_ref.mul + sign_ref.sqr > 1000 && pk_ref.mul + pk_ref.sqr > 1000, "the trace saw no products");

  // 3. the instrument tells the variable-time forms apart: sk = 1 against sk = r - 1
  fr one, rm1;
  for (int i = 0; i < 8; ++i) {
    one.v[i] = i == 0;
    rm1.v[i] = FR_LIMBS[i];
  }
  rm1.v[0] -= 1;  // r is odd: no borrow
  g2j s2;
  trace_reset();
  g2_mul_glv4(s2, h, one.v);
  const Trace v1 = trace_get();
  trace_reset();
  g2_mul_glv4(s2, h, rm1.v);
  const Trace v2 = trace_get();
  CHECK(v1.digest != v2.digest, "g2_mul_glv4: the trace does not tell sk = 1 from sk = r - 1");
  g1j g, s1;
  g.x = G1_GEN_X;
  g.y = G1_GEN_Y;
  fp_set_one(g.z);
  trace_reset();
  jac_mul_limbs(s1, g, one.v, 8);
  const Trace w1 = trace_get();
  trace_reset();
  jac_mul_limbs(s1, g, rm1.v, 8);
  const Trace w2 = trace_get();
  CHECK(w1.digest != w2.digest, "jac_mul_limbs: the trace does not tell sk = 1 from sk = r - 1");

  if (g_fail) {
    std::printf("sign_ct_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("sign_ct_host ok: %zu secrets x 3 messages (%zu signatures compared); sign_ct_mul trace %016llx, %llu mul + "
              "%llu sqr; sk_to_pk_ct trace %016llx, %llu mul + %llu sqr; variable-time products sk=1 / sk=r-1: sign "
              "%llu / %llu, sk_to_pk %llu / %llu\n",
              secrets.size(), n_ok, (unsigned long long)sign_ref.digest, (unsigned long long)sign_ref.mul,
              (unsigned long long)sign_ref.sqr, (unsigned long long)pk_ref.digest, (unsigned long long)pk_ref.mul,
              (unsigned long long)pk_ref.sqr, (unsigned long long)(v1.mul + v1.sqr),
              (unsigned long long)(v2.mul + v2.sqr), (unsigned long long)(w1.mul + w1.sqr),
              (unsigned long long)(w2.mul + w2.sqr));
  return 0;
}
