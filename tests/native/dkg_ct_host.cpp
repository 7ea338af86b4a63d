// Host program for the lane functions of a joint-Feldman dealing round (charon_amd/csrc/dkg_ct.h), built and run by
// tests/test_dkg_ct_host.py (plain, and under AddressSanitizer + UBSan).
//
//   dkg_ct_host <vectors file>
//
// The file (tests/dkg_vectors.py writes it, expectations from the Python oracle) holds, as tokens:
//   C <threshold> <status> <secret hex> <threshold-1 tail hex>   then threshold times
//       M <j> <commitment status> <commitment hex>
//   K <decode status> <share hex> <expected hex> <status>        one lane of the share check
//   U <n_dealers> <mask given> <status> <sum hex> <pub status> <pub hex>   then n_dealers times   H <include> <share hex>
//   S <secret hex>                                               a secret for the trace comparison
// Checks:
//   1. every M lane: op_commit_ct == the file == op_sk_to_pk for a non-zero coefficient of a good validator;
//   2. every K lane: op_share_check_ct == the file;
//   3. every U validator: op_share_sum_ct == the file, with and without the pubshare;
//   4. with the operation trace (field.h BLS_CT_TRACE) the digest and both product counts of each of the three lane
//      functions are the same for EVERY S secret at a fixed public shape.
#define BLS_COUNT_OPS 1
#define BLS_CT_TRACE 1
#include "../../charon_amd/csrc/dkg_ct.h"

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

struct Trace {
  uint64_t digest, mul, sqr;
  bool operator==(const Trace& o) const { return digest == o.digest && mul == o.mul && sqr == o.sqr; }
};
static void trace_reset() { g_ct_trace = g_fp_mul_count = g_fp_sqr_count = 0; }
static Trace trace_get() { return Trace{g_ct_trace, g_fp_mul_count, g_fp_sqr_count}; }

static int g_fail = 0;
#define CHECK(cond, ...)                   \
  do {                                     \
    if (!(cond)) {                         \
      if (g_fail++ < 20) {                 \
        std::printf("FAIL: " __VA_ARGS__); \
        std::printf("\n");                 \
      }                                    \
    }                                      \
  } while (0)

static std::string hex(const uint8_t* b, int n) {
  static const char* d = "0123456789abcdef";
  std::string s;
  for (int i = 0; i < n; ++i) {
    s += d[b[i] >> 4];
    s += d[b[i] & 15];
  }
  return s;
}
static bool unhex(const char* h, uint8_t* out, size_t n) {
  if (std::strlen(h) != 2 * n) return false;
  for (size_t i = 0; i < n; ++i) {
    unsigned v;
    if (std::sscanf(h + 2 * i, "%2x", &v) != 1) return false;
    out[i] = (uint8_t)v;
  }
  return true;
}

struct Commit {
  uint32_t threshold;
  int status;
  uint8_t secret[32];
  std::vector<uint8_t> tail, coms;  // 32 (threshold - 1) (+1 spare byte), 48 threshold
  std::vector<int> com_status;
};
struct ShareCheck {
  int decode_status, status;
  uint8_t share[32], expected[48];
};
struct Sum {
  uint32_t n_dealers;
  bool masked;
  int status, pub_status;
  uint8_t out[32], pub[48];
  std::vector<uint8_t> include, shares;
};

static std::vector<Commit> g_commits;
static std::vector<ShareCheck> g_checks;
static std::vector<Sum> g_sums;
static std::vector<std::vector<uint8_t>> g_secrets;

static bool read_vectors(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char tag[8], a[200], b[200];
  bool ok = true;
  while (ok && std::fscanf(f, "%7s", tag) == 1) {
    if (!std::strcmp(tag, "C")) {
      Commit c;
      ok = std::fscanf(f, "%u %d %199s", &c.threshold, &c.status, a) == 3 && unhex(a, c.secret, 32) &&
           c.threshold >= 1 && c.threshold <= 64;
      if (!ok) break;
      c.tail.resize(32 * (c.threshold - 1) + 1);
      for (uint32_t j = 0; ok && j + 1 < c.threshold; ++j)
        ok = std::fscanf(f, "%199s", a) == 1 && unhex(a, c.tail.data() + 32 * j, 32);
      c.coms.assign(48 * c.threshold, 0);
      c.com_status.assign(c.threshold, -1);
      for (uint32_t j = 0; ok && j < c.threshold; ++j) {
        unsigned jj;
        ok = std::fscanf(f, "%7s %u %d %199s", tag, &jj, &c.com_status[j], a) == 4 && !std::strcmp(tag, "M") &&
             jj == j && unhex(a, c.coms.data() + 48 * j, 48);
      }
      if (ok) g_commits.push_back(c);
    } else if (!std::strcmp(tag, "K")) {
      ShareCheck k;
      ok = std::fscanf(f, "%d %199s %199s %d", &k.decode_status, a, b, &k.status) == 4 && unhex(a, k.share, 32) &&
           unhex(b, k.expected, 48);
      if (ok) g_checks.push_back(k);
    } else if (!std::strcmp(tag, "U")) {
      Sum u;
      int masked;
      ok = std::fscanf(f, "%u %d %d %199s %d %199s", &u.n_dealers, &masked, &u.status, a, &u.pub_status, b) == 6 &&
           unhex(a, u.out, 32) && unhex(b, u.pub, 48) && u.n_dealers >= 1 && u.n_dealers <= 64;
      if (!ok) break;
      u.masked = masked != 0;
      u.include.resize(u.n_dealers);
      u.shares.resize(32 * u.n_dealers);
      for (uint32_t d = 0; ok && d < u.n_dealers; ++d) {
        unsigned inc;
        ok = std::fscanf(f, "%7s %u %199s", tag, &inc, a) == 3 && !std::strcmp(tag, "H") && inc <= 255 &&
             unhex(a, u.shares.data() + 32 * d, 32);
        u.include[d] = (uint8_t)inc;
      }
      if (ok) g_sums.push_back(u);
    } else if (!std::strcmp(tag, "S")) {
      std::vector<uint8_t> s(32);
      ok = std::fscanf(f, "%199s", a) == 1 && unhex(a, s.data(), 32);
      if (ok) g_secrets.push_back(s);
    } else {
      ok = false;
    }
  }
  std::fclose(f);
  return ok;
}

static uint32_t g_T[COMB_WORDS];

static bool all_zero(const uint8_t* b, int n) {
  uint8_t z = 0;
  for (int i = 0; i < n; ++i) z |= b[i];
  return z == 0;
}

static size_t check_commits() {
  size_t lanes = 0;
  for (const Commit& c : g_commits)
    for (uint32_t j = 0; j < c.threshold; ++j, ++lanes) {
      uint8_t com[48], ref[48];
      std::memset(com, 0xee, 48);
      const uint8_t* tail = c.threshold > 1 ? c.tail.data() : nullptr;
      const int st = op_commit_ct(com, g_T, c.secret, tail, c.threshold, j);
      CHECK(st == c.com_status[j] && !std::memcmp(com, c.coms.data() + 48 * j, 48),
            "commitment %u of %u: %d %s, the oracle has %d %s", j, c.threshold, st, hex(com, 48).c_str(),
            c.com_status[j], hex(c.coms.data() + 48 * j, 48).c_str());
      CHECK((st == HIPBLS_OK) == (c.status == HIPBLS_OK), "commitment status %d beside validator status %d", st, c.status);
      if (st != HIPBLS_OK) {
        CHECK(all_zero(com, 48), "a bad validator's commitment is not zero bytes");
        continue;
      }
      const uint8_t* coef = j == 0 ? c.secret : c.tail.data() + 32 * (j - 1);
      if (all_zero(coef, 32)) {
        CHECK(com[0] == 0xc0 && all_zero(com + 1, 47), "a zero coefficient is not the infinity encoding");
      } else {
        CHECK(op_sk_to_pk(ref, coef) == HIPBLS_OK && !std::memcmp(ref, com, 48), "commitment %u differs from op_sk_to_pk", j);
      }
    }
  return lanes;
}

static void check_checks() {
  for (const ShareCheck& k : g_checks) {
    const int st = op_share_check_ct(g_T, k.share, k.expected, k.decode_status);
    CHECK(st == k.status, "share check: %d, the oracle has %d (share %s, decode status %d)", st, k.status,
          hex(k.share, 32).c_str(), k.decode_status);
  }
}

static void check_sums() {
  for (const Sum& u : g_sums)
    for (int with_pub = 0; with_pub < 2; ++with_pub) {
      uint8_t out[32], pub[48];
      std::memset(out, 0xee, 32);
      std::memset(pub, 0xee, 48);
      int pst = -7;
      const int st = op_share_sum_ct(out, pub, &pst, g_T, with_pub != 0, u.shares.data(),
                                     u.masked ? u.include.data() : nullptr, u.n_dealers);
      CHECK(st == u.status && !std::memcmp(out, u.out, 32), "sum over %u dealers: %d %s, the oracle has %d %s",
            u.n_dealers, st, hex(out, 32).c_str(), u.status, hex(u.out, 32).c_str());
      if (st != HIPBLS_OK) CHECK(all_zero(out, 32), "a failed sum is not zero bytes");
      if (with_pub)
        CHECK(pst == u.pub_status && !std::memcmp(pub, u.pub, 48), "pubshare of the sum: %d %s, the oracle has %d %s", pst,
              hex(pub, 48).c_str(), u.pub_status, hex(u.pub, 48).c_str());
      else
        CHECK(pst == -7 && pub[0] == 0xee && pub[47] == 0xee, "an unwanted pubshare was written");
    }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: dkg_ct_host <vectors file>\n");
    return 2;
  }
  if (!read_vectors(argv[1]) || g_commits.empty() || g_checks.empty() || g_sums.empty() || g_secrets.size() < 7) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  for (int w = 0; w < COMB_WINDOWS; ++w)
    for (int j = 1; j <= 15; ++j) comb_build_entry(g_T + (w * 15 + j - 1) * 24, w, j);

  const size_t lanes = check_commits();
  check_checks();
  check_sums();

  // 4. one operation stream for every secret at a fixed public shape.  Commitments: threshold 7, lane j = 3, the
  //    secret under test as that coefficient with the others rotating through the list (so the root secret and every
  //    other coefficient are under test too).  Share check: the secret as the share, fixed expected bytes and decode
  //    status.  Sum: 4 dealers with the mask 1, 0, 1, 1, the secret in every position in turn (by rotation), with
  //    the pubshare.
  Trace com_ref{}, chk_ref{}, sum_ref{};
  static const uint8_t include[4] = {1, 0, 1, 1};
  const size_t ns = g_secrets.size();
  for (size_t i = 0; i < ns; ++i) {
    uint8_t root[32], tail[32 * 6], shares[32 * 4], out48[48], out32[32];
    std::memcpy(root, g_secrets[(i + 5) % ns].data(), 32);
    for (int j = 0; j < 6; ++j) std::memcpy(tail + 32 * j, g_secrets[(i + j + ns - 2) % ns].data(), 32);  // tail[2]: secret i
    for (int j = 0; j < 4; ++j) std::memcpy(shares + 32 * j, g_secrets[(i + j) % ns].data(), 32);
    trace_reset();
    (void)op_commit_ct(out48, g_T, root, tail, 7, 3);
    const Trace t = trace_get();
    if (i == 0) com_ref = t;
    CHECK(t == com_ref, "commit trace differs for secret %s", hex(g_secrets[i].data(), 32).c_str());
    trace_reset();
    (void)op_share_check_ct(g_T, g_secrets[i].data(), g_checks[0].expected, HIPBLS_OK);
    const Trace u = trace_get();
    if (i == 0) chk_ref = u;
    CHECK(u == chk_ref, "share check trace differs for secret %s", hex(g_secrets[i].data(), 32).c_str());
    int pst;
    trace_reset();
    (void)op_share_sum_ct(out32, out48, &pst, g_T, true, shares, include, 4);
    const Trace v = trace_get();
    if (i == 0) sum_ref = v;
    CHECK(v == sum_ref, "sum trace differs for secret %s", hex(g_secrets[i].data(), 32).c_str());
  }
  CHECK(com_ref.mul + com_ref.sqr > 500 && chk_ref.mul + chk_ref.sqr > 500 && sum_ref.mul + sum_ref.sqr > 500 &&
            sum_ref.digest != 0,
        "the trace saw no operations");

  if (g_fail) {
    std::printf("dkg_ct_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("dkg_ct_host ok: %zu validators (%zu commitment lanes), %zu check lanes, %zu sums, %zu trace secrets; "
              "commit trace %016llx, %llu mul + %llu sqr; check trace %016llx, %llu mul + %llu sqr; sum trace %016llx, "
              "%llu mul + %llu sqr\n",
              g_commits.size(), lanes, g_checks.size(), g_sums.size(), g_secrets.size(),
              (unsigned long long)com_ref.digest, (unsigned long long)com_ref.mul, (unsigned long long)com_ref.sqr,
              (unsigned long long)chk_ref.digest, (unsigned long long)chk_ref.mul, (unsigned long long)chk_ref.sqr,
              (unsigned long long)sum_ref.digest, (unsigned long long)sum_ref.mul, (unsigned long long)sum_ref.sqr);
  return 0;
}
