// Host program for the secret-independent split / recover lane functions (charon_amd/csrc/deal_ct.h), built and run
// by tests/test_deal_ct_host.py (plain, and under AddressSanitizer + UBSan).
//
//   deal_ct_host <vectors file>
//
// The file (tests/deal_ct_vectors.py writes it, expectations from the Python oracle) holds, as tokens:
//   D <total> <threshold> <status> <secret hex> <threshold-1 tail hex>   then total+1 times
//       P <k> <share hex | -> <pub status> <pub hex>                     k = 0..total (no share bytes for k = 0)
//   R <m> <status> <secret hex> <pk status> <pk hex>   then m times   I <id> <share hex>
//   S <secret hex>                                     a secret for the trace comparison
// Checks:
//   1. fr_add_ct / fr_sub_ct / fr_mul_ct == fr_add / fr_sub / fr_mul on edge and seeded random elements;
//   2. every D lane: op_deal_ct + g1_pub_ct == the file == the variable-time forms (fr.h Horner, op_sk_to_pk);
//   3. the comb: [j 16^w] g1 for all 960 (w, j) and [16^w - 1] g1 against op_sk_to_pk;
//   4. every R group: op_recover_ct == the file == the variable-time forms;
//   5. with the operation trace (field.h BLS_CT_TRACE) the digest and both product counts of the split evaluation,
//      the comb multiplication and the recovery are the same for EVERY S secret at a fixed public shape, while
//      jac_mul_limbs' trace tells sk = 1 from sk = r - 1.
#define BLS_COUNT_OPS 1
#define BLS_CT_TRACE 1
#include "../../charon_amd/csrc/deal_ct.h"

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

struct Deal {
  uint32_t total, threshold;
  int status;
  uint8_t secret[32];
  std::vector<uint8_t> tail;           // 32 (threshold - 1)
  std::vector<uint8_t> shares, pubs;   // 32 (total + 1) (entry 0 unused), 48 (total + 1)
  std::vector<int> pub_status;
};
struct Recover {
  int status, pk_status;
  uint8_t secret[32], pk[48];
  std::vector<int64_t> ids;
  std::vector<uint8_t> shares;
};

static std::vector<Deal> g_deals;
static std::vector<Recover> g_recs;
static std::vector<std::vector<uint8_t>> g_secrets;

static bool read_vectors(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char tag[8], a[200], b[200];
  bool ok = true;
  while (ok && std::fscanf(f, "%7s", tag) == 1) {
    if (!std::strcmp(tag, "D")) {
      Deal d;
      ok = std::fscanf(f, "%u %u %d %199s", &d.total, &d.threshold, &d.status, a) == 4 && unhex(a, d.secret, 32);
      ok = ok && d.total >= 1 && d.total <= 64 && d.threshold >= 1 && d.threshold <= 64;
      if (!ok) break;
      d.tail.resize(32 * (d.threshold - 1) + 1);
      for (uint32_t j = 0; ok && j + 1 < d.threshold; ++j)
        ok = std::fscanf(f, "%199s", a) == 1 && unhex(a, d.tail.data() + 32 * j, 32);
      d.shares.assign(32 * (d.total + 1), 0);
      d.pubs.assign(48 * (d.total + 1), 0);
      d.pub_status.assign(d.total + 1, -1);
      for (uint32_t k = 0; ok && k <= d.total; ++k) {
        unsigned kk;
        int ps;
        ok = std::fscanf(f, "%7s %u %199s %d %199s", tag, &kk, a, &ps, b) == 5 && !std::strcmp(tag, "P") && kk == k;
        if (!ok) break;
        if (k >= 1) ok = unhex(a, d.shares.data() + 32 * k, 32);
        ok = ok && unhex(b, d.pubs.data() + 48 * k, 48);
        d.pub_status[k] = ps;
      }
      if (ok) g_deals.push_back(d);
    } else if (!std::strcmp(tag, "R")) {
      Recover r;
      unsigned m;
      ok = std::fscanf(f, "%u %d %199s %d %199s", &m, &r.status, a, &r.pk_status, b) == 5 && m <= 64 &&
           unhex(a, r.secret, 32) && unhex(b, r.pk, 48);
      if (!ok) break;
      r.shares.resize(32 * m + 32);  // one spare entry: an empty group still has something to point at
      for (unsigned k = 0; ok && k < m; ++k) {
        long long id;
        ok = std::fscanf(f, "%7s %lld %199s", tag, &id, a) == 3 && !std::strcmp(tag, "I") &&
             unhex(a, r.shares.data() + 32 * k, 32);
        r.ids.push_back((int64_t)id);
      }
      if (ok) g_recs.push_back(r);
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

// ---- the variable-time forms (what k_threshold_split and k_recover_secret computed) ------------------------------
static int vt_split(uint8_t* out32, const uint8_t* secret, const uint8_t* tail, uint32_t threshold, uint32_t i) {
  fr coef, acc, x, r2;
  for (int w = 0; w < 8; ++w) r2.v[w] = FR_R2[w], acc.v[w] = 0;
  fr_from_u32(x, i);
  bool ok = true;
  for (int j = (int)threshold - 1; j >= 0; --j) {
    const uint8_t* c = j == 0 ? secret : tail + 32 * (j - 1);
    if (!fr_plain_from_be32(coef, c)) ok = false;
    fr_mul(coef, coef, r2);
    fr_mul(acc, acc, x);
    fr_add(acc, acc, coef);
  }
  fr plain;
  fr_to_plain(plain, acc);
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) out32[31 - 4 * w - b] = ok ? (uint8_t)(plain.v[w] >> (8 * b)) : (uint8_t)0;
  return ok ? HIPBLS_OK : HIPBLS_ERR_SECRET;
}
static int vt_recover(uint8_t* out32, const uint8_t* shares, const int64_t* ids, uint32_t n) {
  int st = n > 0 ? HIPBLS_OK : HIPBLS_ERR_COMBINE;
  for (uint32_t a = 0; a < n; ++a) {
    if (ids[a] == 0) st = HIPBLS_ERR_COMBINE;
    for (uint32_t b = a + 1; b < n; ++b)
      if (ids[a] == ids[b]) st = HIPBLS_ERR_COMBINE;
  }
  fr acc, r2;
  for (int w = 0; w < 8; ++w) acc.v[w] = 0, r2.v[w] = FR_R2[w];
  for (uint32_t k = 0; k < n && st == HIPBLS_OK; ++k) {
    fr s, lam;
    if (!fr_plain_from_be32(s, shares + 32 * k)) {
      st = HIPBLS_ERR_SECRET;
      break;
    }
    lagrange_at_zero(lam, ids, (int)n, (int)k);
    fr_mul(lam, lam, r2);
    fr_mul(s, s, r2);
    fr_mul(s, s, lam);
    fr_add(acc, acc, s);
  }
  fr plain;
  fr_to_plain(plain, acc);
  for (int w = 0; w < 8; ++w)
    for (int b = 0; b < 4; ++b) out32[31 - 4 * w - b] = st == HIPBLS_OK ? (uint8_t)(plain.v[w] >> (8 * b)) : (uint8_t)0;
  return st;
}
static bool all_zero(const uint8_t* b, int n) {
  uint8_t z = 0;
  for (int i = 0; i < n; ++i) z |= b[i];
  return z == 0;
}

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd32() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}
static void rnd_fr(fr& a) {  // below r: the top limb below r's
  for (int i = 0; i < 8; ++i) a.v[i] = rnd32();
  a.v[7] %= FR_LIMBS[7];
}

static void check_fr() {
  std::vector<fr> v;
  fr z, one, rm1;
  for (int i = 0; i < 8; ++i) z.v[i] = 0, one.v[i] = i == 0, rm1.v[i] = FR_LIMBS[i];
  rm1.v[0] -= 1;
  v.push_back(z);
  v.push_back(one);
  v.push_back(rm1);
  for (int i = 0; i < 61; ++i) {
    fr a;
    rnd_fr(a);
    v.push_back(a);
  }
  for (const fr& a : v)
    for (const fr& b : v) {
      fr x, y;
      fr_add(x, a, b);
      fr_add_ct(y, a, b);
      CHECK(!std::memcmp(&x, &y, sizeof x), "fr_add_ct differs");
      fr_sub(x, a, b);
      fr_sub_ct(y, a, b);
      CHECK(!std::memcmp(&x, &y, sizeof x), "fr_sub_ct differs");
      fr_mul(x, a, b);
      fr_mul_ct(y, a, b);
      CHECK(!std::memcmp(&x, &y, sizeof x), "fr_mul_ct differs");
    }
}

static size_t check_deals() {
  size_t lanes = 0;
  for (const Deal& d : g_deals) {
    for (uint32_t k = 0; k <= d.total; ++k, ++lanes) {
      uint8_t share[32], pub[48], ref[32], refpk[48];
      std::memset(share, 0xee, 32);
      std::memset(pub, 0xee, 48);
      fr scalar;
      uint32_t ok;
      const int st = op_deal_ct(share, scalar, ok, d.secret, d.tail.data(), d.threshold, k);
      const int pst = g1_pub_ct(pub, g_T, scalar, ok);
      CHECK(st == d.status, "deal status %d, expected %d (total %u threshold %u secret %s)", st, d.status, d.total,
            d.threshold, hex(d.secret, 32).c_str());
      const int vst = vt_split(ref, d.secret, d.tail.data(), d.threshold, k);
      CHECK(vst == st && !std::memcmp(ref, share, 32), "lane k=%u differs from the variable-time split: %s / %s", k,
            hex(share, 32).c_str(), hex(ref, 32).c_str());
      if (k >= 1)
        CHECK(!std::memcmp(share, d.shares.data() + 32 * k, 32), "share %u: %s, the oracle has %s", k,
              hex(share, 32).c_str(), hex(d.shares.data() + 32 * k, 32).c_str());
      else if (st == HIPBLS_OK)
        CHECK(!std::memcmp(share, d.secret, 32), "f(0) is not the secret");
      if (st != HIPBLS_OK) CHECK(all_zero(share, 32) && all_zero(pub, 48), "a bad validator's outputs are not zero");
      CHECK(pst == d.pub_status[k] && !std::memcmp(pub, d.pubs.data() + 48 * k, 48),
            "pub %u: status %d %s, the oracle has %d %s", k, pst, hex(pub, 48).c_str(), d.pub_status[k],
            hex(d.pubs.data() + 48 * k, 48).c_str());
      std::memset(refpk, 0, 48);
      const int vpst = st == HIPBLS_OK ? op_sk_to_pk(refpk, share) : HIPBLS_ERR_SECRET;
      if (vpst != HIPBLS_OK) std::memset(refpk, 0, 48);
      CHECK(vpst == pst && !std::memcmp(refpk, pub, 48), "pub %u differs from op_sk_to_pk", k);
    }
  }
  return lanes;
}

static size_t check_comb() {
  size_t n = 0;
  for (int w = 0; w < COMB_WINDOWS; ++w)
    for (int j = 0; j <= 15; ++j, ++n) {  // j = 0 stands for 16^w - 1
      uint32_t k[8];
      if (j) {
        comb_entry_scalar(k, w, j);
      } else {
        for (int i = 0; i < 8; ++i) k[i] = 0;
        for (int i = 0; i < w; ++i) k[i >> 3] |= 15u << (4 * (i & 7));
      }
      fr s;
      uint8_t sk[32], a[48], b[48];
      for (int i = 0; i < 8; ++i) s.v[i] = k[i];
      fr_store_be32_ct(sk, s, ~0u);
      fr chk;
      const bool below = fr_plain_from_be32(chk, sk);
      std::memset(a, 0, 48);
      const int sa = op_sk_to_pk(a, sk);
      if (sa != HIPBLS_OK) std::memset(a, 0, 48);
      const int sb = g1_pub_ct(b, g_T, s, below ? ~0u : 0u);
      CHECK(sa == sb && !std::memcmp(a, b, 48), "comb w=%d j=%d: %d %s, op_sk_to_pk %d %s", w, j, sb,
            hex(b, 48).c_str(), sa, hex(a, 48).c_str());
    }
  return n;
}

static void check_recovers() {
  static const int64_t spare_id[1] = {1};
  for (const Recover& r : g_recs) {
    const uint32_t m = (uint32_t)r.ids.size();
    const int64_t* ids = m ? r.ids.data() : spare_id;
    for (uint32_t m_max : {m, m + 3u}) {  // the launch's largest group may be larger than this one
      uint8_t sec[32], pk[48], ref[32];
      std::memset(sec, 0xee, 32);
      std::memset(pk, 0xee, 48);
      int pst = -1;
      const int st = op_recover_ct(sec, pk, &pst, g_T, true, r.shares.data(), ids, m, m_max);
      CHECK(st == r.status && !std::memcmp(sec, r.secret, 32), "recover (m %u): %d %s, the oracle has %d %s", m, st,
            hex(sec, 32).c_str(), r.status, hex(r.secret, 32).c_str());
      CHECK(pst == r.pk_status && !std::memcmp(pk, r.pk, 48), "recover (m %u) key: %d %s, the oracle has %d %s", m,
            pst, hex(pk, 48).c_str(), r.pk_status, hex(r.pk, 48).c_str());
      const int vst = vt_recover(ref, r.shares.data(), ids, m);
      CHECK(vst == st && !std::memcmp(ref, sec, 32), "recover (m %u) differs from the variable-time form", m);
      if (st != HIPBLS_OK) CHECK(all_zero(sec, 32) && all_zero(pk, 48), "a failed group's outputs are not zero");
    }
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::printf("usage: deal_ct_host <vectors file>\n");
    return 2;
  }
  if (!read_vectors(argv[1]) || g_deals.empty() || g_recs.empty() || g_secrets.size() < 2) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  for (int w = 0; w < COMB_WINDOWS; ++w)
    for (int j = 1; j <= 15; ++j) comb_build_entry(g_T + (w * 15 + j - 1) * 24, w, j);

  check_fr();
  const size_t lanes = check_deals();
  const size_t combs = check_comb();
  check_recovers();

  // 5. one operation stream for every secret at a fixed public shape: 7-of-10, lane k = 3; ids 1, 2, 3 of a launch
  //    whose largest group has 4 shares.  The secret under test is the root secret, every tail coefficient in turn
  //    (by rotation), the comb's scalar, and every share.
  Trace split_ref{}, comb_ref{}, rec_ref{};
  const int64_t ids[3] = {1, 2, 3};
  for (size_t i = 0; i < g_secrets.size(); ++i) {
    uint8_t tail[32 * 6], shares[32 * 4], out[48], sh[32];
    for (int j = 0; j < 6; ++j) std::memcpy(tail + 32 * j, g_secrets[(i + 1 + j) % g_secrets.size()].data(), 32);
    for (int j = 0; j < 4; ++j) std::memcpy(shares + 32 * j, g_secrets[(i + j) % g_secrets.size()].data(), 32);
    fr scalar;
    uint32_t ok;
    trace_reset();
    (void)op_deal_ct(sh, scalar, ok, g_secrets[i].data(), tail, 7, 3);
    const Trace t = trace_get();
    if (i == 0) split_ref = t;
    CHECK(t == split_ref, "split trace differs for secret %s", hex(g_secrets[i].data(), 32).c_str());
    fr raw;
    (void)fr_load_mask_ct(raw, g_secrets[i].data());  // the limbs as they are, also >= r
    g1j p;
    uint32_t inf;
    trace_reset();
    g1_mul_comb_ct(p, inf, g_T, raw.v);
    (void)g1_pub_ct(out, g_T, scalar, ok);
    const Trace u = trace_get();
    if (i == 0) comb_ref = u;
    CHECK(u == comb_ref, "comb trace differs for secret %s: %016llx mul %llu sqr %llu", hex(g_secrets[i].data(), 32).c_str(),
          (unsigned long long)u.digest, (unsigned long long)u.mul, (unsigned long long)u.sqr);
    int pst;
    trace_reset();
    (void)op_recover_ct(sh, out, &pst, g_T, true, shares, ids, 3, 4);
    const Trace v = trace_get();
    if (i == 0) rec_ref = v;
    CHECK(v == rec_ref, "recover trace differs for secret %s", hex(g_secrets[i].data(), 32).c_str());
  }
  CHECK(split_ref.digest != 0 && comb_ref.mul + comb_ref.sqr > 1000 && rec_ref.mul + rec_ref.sqr > 500,
        "the trace saw no operations");

  // the instrument tells the variable-time form apart: sk = 1 against sk = r - 1
  fr one, rm1;
  for (int i = 0; i < 8; ++i) one.v[i] = i == 0, rm1.v[i] = FR_LIMBS[i];
  rm1.v[0] -= 1;
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
    std::printf("deal_ct_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("deal_ct_host ok: %zu validators (%zu lanes), %zu groups, %zu comb scalars, %zu trace secrets; split trace "
              "%016llx; comb + key trace %016llx, %llu mul + %llu sqr; recover trace %016llx, %llu mul + %llu sqr; "
              "variable-time products sk=1 / sk=r-1: %llu / %llu\n",
              g_deals.size(), lanes, g_recs.size(), combs, g_secrets.size(), (unsigned long long)split_ref.digest,
              (unsigned long long)comb_ref.digest, (unsigned long long)comb_ref.mul, (unsigned long long)comb_ref.sqr,
              (unsigned long long)rec_ref.digest, (unsigned long long)rec_ref.mul, (unsigned long long)rec_ref.sqr,
              (unsigned long long)(w1.mul + w1.sqr), (unsigned long long)(w2.mul + w2.sqr));
  return 0;
}
