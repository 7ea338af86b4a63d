// Host program for the PublicKeyShare / PublicKeyRecover lane functions (charon_amd/csrc/vss.h), built and run by
// tests/test_vss_host.py (plain, and under AddressSanitizer + UBSan) and by charon_amd/tools/vss_timing.py.
//
//   vss_host <vectors file>             check every vector, print the work counts
//   vss_host --time <threads> <rounds>  the timing shape of DESIGN.md 4.15 on the host (a port, not a product)
//
// The file (tests/vss_vectors.py writes it, expectations from the Python oracle) holds, as tokens:
//   S <n_val> <n_dealers> <threshold> <n_ids> <ids ...>     then n_val times
//       V <status> <n_dealers threshold commitments, hex>   and   O <n_ids outputs, hex>
//   G <m> <status> <key hex>   then m times   I <id> <pubshare hex>
// A share call runs as the kernels do: one decode lane per commitment into the limb-major arrays (k_g1_decode's
// code), one dealer-sum lane per coefficient when n_dealers > 1, one evaluation lane per (validator, id).  All groups
// run as ONE recover launch: a scale lane per pubshare, a sum lane per group.  Every array is allocated at its exact
// size, so a lane that leaves its arrays is an AddressSanitizer report.
#define BLS_COUNT_OPS 1
#include "../../charon_amd/csrc/vss.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace bls {
thread_local uint64_t g_fp_mul_count = 0;
thread_local uint64_t g_fp_sqr_count = 0;
}  // namespace bls
using namespace bls;

static uint64_t ops() { return g_fp_mul_count + g_fp_sqr_count; }

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

struct ShareCall {
  uint32_t n_val, n_dealers, threshold, n_ids;
  std::vector<int64_t> ids;
  std::vector<uint8_t> commitments, pubs;  // 48 n_val n_dealers threshold, 48 n_val n_ids
  std::vector<int> status;
};
struct Groups {
  std::vector<uint64_t> offs{0};
  std::vector<int64_t> ids;
  std::vector<uint8_t> shares, keys;
  std::vector<int> status;
};
static std::vector<ShareCall> g_calls;
static Groups g_groups;

static bool read_vectors(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  char tag[8], a[200];
  bool ok = true;
  while (ok && std::fscanf(f, "%7s", tag) == 1) {
    if (!std::strcmp(tag, "S")) {
      ShareCall c;
      ok = std::fscanf(f, "%u %u %u %u", &c.n_val, &c.n_dealers, &c.threshold, &c.n_ids) == 4 && c.n_val >= 1 &&
           c.n_val <= 4096 && c.n_dealers >= 1 && c.n_dealers <= 64 && c.threshold >= 1 && c.threshold <= 64 &&
           c.n_ids >= 1 && c.n_ids <= 64;
      for (uint32_t i = 0; ok && i < c.n_ids; ++i) {
        long long id;
        ok = std::fscanf(f, "%lld", &id) == 1;
        c.ids.push_back((int64_t)id);
      }
      if (!ok) break;
      const size_t per = (size_t)c.n_dealers * c.threshold;
      c.commitments.resize(48 * per * c.n_val);
      c.pubs.resize(48 * (size_t)c.n_ids * c.n_val);
      for (uint32_t v = 0; ok && v < c.n_val; ++v) {
        int st;
        ok = std::fscanf(f, "%7s %d", tag, &st) == 2 && !std::strcmp(tag, "V");
        c.status.push_back(st);
        for (size_t k = 0; ok && k < per; ++k)
          ok = std::fscanf(f, "%199s", a) == 1 && unhex(a, c.commitments.data() + 48 * (per * v + k), 48);
        ok = ok && std::fscanf(f, "%7s", tag) == 1 && !std::strcmp(tag, "O");
        for (uint32_t i = 0; ok && i < c.n_ids; ++i)
          ok = std::fscanf(f, "%199s", a) == 1 && unhex(a, c.pubs.data() + 48 * ((size_t)c.n_ids * v + i), 48);
      }
      if (ok) g_calls.push_back(c);
    } else if (!std::strcmp(tag, "G")) {
      unsigned m;
      int st;
      uint8_t key[48], sh[48];
      ok = std::fscanf(f, "%u %d %199s", &m, &st, a) == 3 && m <= 64 && unhex(a, key, 48);
      for (unsigned k = 0; ok && k < m; ++k) {
        long long id;
        ok = std::fscanf(f, "%7s %lld %199s", tag, &id, a) == 3 && !std::strcmp(tag, "I") && unhex(a, sh, 48);
        g_groups.ids.push_back((int64_t)id);
        g_groups.shares.insert(g_groups.shares.end(), sh, sh + 48);
      }
      if (!ok) break;
      g_groups.offs.push_back(g_groups.ids.size());
      g_groups.keys.insert(g_groups.keys.end(), key, key + 48);
      g_groups.status.push_back(st);
    } else {
      ok = false;
    }
  }
  std::fclose(f);
  return ok;
}

// k_g1_decode's lane
static void decode_lane(const uint8_t* pks, uint64_t n, uint64_t i, uint32_t* pts, int32_t* code) {
  g1a a;
  const int st = g1_decompress(a, pks + 48 * i, true);
  const uint32_t* src = &a.x.v[0];
  for (int w = 0; w < 24; ++w) pts[(uint64_t)w * n + i] = st == DEC_OK ? src[w] : 0u;
  code[i] = st;
}

// One share call over validators [v0, v1) of it, as launch_pk_share runs it.  Returns the products + squarings of
// (decode, dealer sum, evaluation).
struct ShareOps {
  uint64_t decode, sum, eval;
};
static ShareOps run_share(const uint8_t* commitments, uint32_t n_val, uint32_t n_dealers, uint32_t threshold,
                          const int64_t* ids, uint32_t n_ids, uint8_t* out_pubs, int32_t* status) {
  const uint64_t n_coef = (uint64_t)n_val * threshold, n_pts = n_coef * n_dealers;
  std::vector<uint32_t> pts(24 * n_pts), sum;
  std::vector<int32_t> code(n_pts), scode;
  ShareOps o{};
  uint64_t t0 = ops();
  for (uint64_t i = 0; i < n_pts; ++i) decode_lane(commitments, n_pts, i, pts.data(), code.data());
  o.decode = ops() - t0;
  const uint32_t* p = pts.data();
  const int32_t* c = code.data();
  if (n_dealers > 1) {
    sum.resize(24 * n_coef);
    scode.resize(n_coef);
    t0 = ops();
    for (uint64_t i = 0; i < n_coef; ++i)
      vss_dealer_sum_lane(sum.data(), scode.data(), n_coef, pts.data(), code.data(), n_pts, i / threshold, n_dealers,
                          threshold, (uint32_t)(i % threshold));
    o.sum = ops() - t0;
    p = sum.data();
    c = scode.data();
  }
  t0 = ops();
  for (uint64_t l = 0; l < (uint64_t)n_val * n_ids; ++l) {  // k_vss_eval's lane order: validator fastest
    const uint32_t i = (uint32_t)(l / n_val), v = (uint32_t)(l % n_val);
    const int st = vss_eval_lane(out_pubs + 48 * ((uint64_t)v * n_ids + i), p, c, n_coef, v, threshold, ids[i]);
    if (i == 0) status[v] = st;
  }
  o.eval = ops() - t0;
  return o;
}

// One recover launch, as launch_pk_recover runs it.  ops_by_share, when given, receives each scale lane's count.
static void run_recover(const uint8_t* shares, const int64_t* ids, const uint64_t* offs, uint64_t n_groups,
                        uint8_t* out, int32_t* status, std::vector<uint64_t>* ops_by_share = nullptr) {
  const uint64_t n_parts = offs[n_groups];
  std::vector<uint32_t> pts(36 * (n_parts ? n_parts : 1));
  std::vector<int32_t> pstat(n_parts ? n_parts : 1);
  for (uint64_t g = 0; g < n_groups; ++g)
    for (uint64_t k = offs[g]; k < offs[g + 1]; ++k) {
      g1j p;
      const uint64_t t0 = ops();
      pstat[k] = vss_scale_lane(p, shares + 48 * k, ids + offs[g], (int)(offs[g + 1] - offs[g]), (int)(k - offs[g]));
      if (ops_by_share) ops_by_share->push_back(ops() - t0);
      soa_store<36>(pts.data(), n_parts, k, &p.x.v[0]);
    }
  for (uint64_t g = 0; g < n_groups; ++g)
    status[g] = vss_sum_lane(out + 48 * g, pts.data(), pstat.data(), n_parts, offs[g], ids + offs[g],
                             (int)(offs[g + 1] - offs[g]));
}

static bool all_zero(const uint8_t* b, int n) {
  uint8_t z = 0;
  for (int i = 0; i < n; ++i) z |= b[i];
  return z == 0;
}

// [k] g1 compressed
static void pub_of(uint8_t* out48, uint64_t k) {
  g1j g, p;
  g.x = G1_GEN_X;
  g.y = G1_GEN_Y;
  fp_set_one(g.z);
  jac_mul_u64(p, g, k);
  g1_compress(out48, p);
}

// The timing shape: 1,024 validators, 7-of-10, 9 dealers, ids 0..10; then verify_pubshares for every validator
// (4 groups of 7 pubshares each).  The inputs are [k] g1 for small k: the decode and the arithmetic do not care.
static int time_mode(int threads, int rounds) {
  const uint32_t n_val = 1024, n_dealers = 9, threshold = 7, n_ids = 11;
  std::vector<uint8_t> com(48 * (size_t)n_val * n_dealers * threshold);
  for (size_t i = 0; i < com.size() / 48; ++i) pub_of(com.data() + 48 * i, 1000003ull * (i + 1));
  std::vector<int64_t> ids(n_ids);
  for (uint32_t i = 0; i < n_ids; ++i) ids[i] = i;
  std::vector<uint8_t> pubs(48 * (size_t)n_val * n_ids);
  std::vector<int32_t> st(n_val);
  auto share_all = [&] {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        const uint32_t lo = (uint32_t)((uint64_t)n_val * t / threads), hi = (uint32_t)((uint64_t)n_val * (t + 1) / threads);
        if (hi > lo)
          run_share(com.data() + 48 * (size_t)lo * n_dealers * threshold, hi - lo, n_dealers, threshold, ids.data(),
                    n_ids, pubs.data() + 48 * (size_t)lo * n_ids, st.data() + lo);
      });
    for (auto& t : th) t.join();
  };
  share_all();
  // the recover call of verify_pubshares: per validator, shares 1..7 at their ids, then shifted by 8, 9, 10
  const uint64_t n_groups = 4ull * n_val;
  std::vector<uint8_t> sh(48 * 7 * n_groups), keys(48 * n_groups);
  std::vector<int64_t> gid(7 * n_groups);
  std::vector<uint64_t> offs(n_groups + 1);
  std::vector<int32_t> gst(n_groups);
  for (uint64_t g = 0; g <= n_groups; ++g) offs[g] = 7 * g;
  for (uint32_t v = 0; v < n_val; ++v)
    for (int q = 0; q < 4; ++q)
      for (int k = 0; k < 7; ++k) {
        const uint64_t at = 7 * (4ull * v + q) + k;
        std::memcpy(sh.data() + 48 * at, pubs.data() + 48 * ((size_t)v * n_ids + k + 1), 48);
        gid[at] = (k + 1) - (q ? 7 + q : 0);
      }
  auto recover_all = [&] {
    std::vector<std::thread> th;
    for (int t = 0; t < threads; ++t)
      th.emplace_back([&, t] {
        const uint64_t lo = n_groups * t / threads, hi = n_groups * (t + 1) / threads;
        if (hi <= lo) return;
        std::vector<uint64_t> o(hi - lo + 1);
        for (uint64_t g = lo; g <= hi; ++g) o[g - lo] = offs[g] - offs[lo];
        run_recover(sh.data() + 48 * offs[lo], gid.data() + offs[lo], o.data(), hi - lo, keys.data() + 48 * lo,
                    gst.data() + lo);
      });
    for (auto& t : th) t.join();
  };
  for (int r = 0; r < rounds; ++r) {
    const auto a = std::chrono::steady_clock::now();
    share_all();
    const auto b = std::chrono::steady_clock::now();
    recover_all();
    const auto c = std::chrono::steady_clock::now();
    int good = 0;
    for (uint32_t v = 0; v < n_val; ++v) {
      bool ok = st[v] == HIPBLS_OK;
      for (int q = 0; q < 4; ++q) {
        const uint8_t* want = pubs.data() + 48 * ((size_t)v * n_ids + (q ? 7 + q : 0));
        ok = ok && gst[4 * v + q] == HIPBLS_OK && !std::memcmp(keys.data() + 48 * (4ull * v + q), want, 48);
      }
      good += ok;
    }
    std::printf("round %d share_ms %.3f recover_ms %.3f verified %d\n", r,
                std::chrono::duration<double, std::milli>(b - a).count(),
                std::chrono::duration<double, std::milli>(c - b).count(), good);
    if (good != (int)n_val) return 1;
  }
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !std::strcmp(argv[1], "--time")) {
    const int threads = std::atoi(argv[2]), rounds = std::atoi(argv[3]);
    if (threads < 1 || threads > 256 || rounds < 1) return 2;
    return time_mode(threads, rounds);
  }
  if (argc != 2) {
    std::printf("usage: vss_host <vectors file> | --time <threads> <rounds>\n");
    return 2;
  }
  if (!read_vectors(argv[1]) || g_calls.empty() || g_groups.status.empty()) {
    std::printf("cannot read %s\n", argv[1]);
    return 2;
  }
  size_t lanes = 0;
  for (size_t n = 0; n < g_calls.size(); ++n) {
    const ShareCall& c = g_calls[n];
    std::vector<uint8_t> out(48 * (size_t)c.n_val * c.n_ids, 0xee);
    std::vector<int32_t> st(c.n_val, -1);
    run_share(c.commitments.data(), c.n_val, c.n_dealers, c.threshold, c.ids.data(), c.n_ids, out.data(), st.data());
    for (uint32_t v = 0; v < c.n_val; ++v) {
      CHECK(st[v] == c.status[v], "share call %zu validator %u: status %d, the oracle has %d", n, v, st[v],
            c.status[v]);
      for (uint32_t i = 0; i < c.n_ids; ++i, ++lanes) {
        const uint8_t* got = out.data() + 48 * ((size_t)c.n_ids * v + i);
        const uint8_t* want = c.pubs.data() + 48 * ((size_t)c.n_ids * v + i);
        CHECK(!std::memcmp(got, want, 48), "share call %zu validator %u id %lld: %s, the oracle has %s", n, v,
              (long long)c.ids[i], hex(got, 48).c_str(), hex(want, 48).c_str());
        if (st[v] != HIPBLS_OK) CHECK(all_zero(got, 48), "a bad validator's outputs are not zero");
      }
    }
  }
  const size_t n_groups = g_groups.status.size();
  {
    std::vector<uint8_t> out(48 * n_groups, 0xee);
    std::vector<int32_t> st(n_groups, -1);
    if (g_groups.ids.empty()) g_groups.ids.push_back(1);
    run_recover(g_groups.shares.data(), g_groups.ids.data(), g_groups.offs.data(), n_groups, out.data(), st.data());
    for (size_t g = 0; g < n_groups; ++g) {
      CHECK(st[g] == g_groups.status[g] && !std::memcmp(out.data() + 48 * g, g_groups.keys.data() + 48 * g, 48),
            "group %zu: %d %s, the oracle has %d %s", g, st[g], hex(out.data() + 48 * g, 48).c_str(),
            g_groups.status[g], hex(g_groups.keys.data() + 48 * g, 48).c_str());
      if (st[g] != HIPBLS_OK) CHECK(all_zero(out.data() + 48 * g, 48), "a failed group's output is not zero");
    }
  }

  // the work counts of DESIGN.md 4.15 (Fp products + squarings): one validator, 7 coefficients, 9 dealers, ids 0..10;
  // one 7-of-10 group on the small-integer path (ids 1..7) and off it (ids 2^40 + 1..7)
  uint8_t com[48 * 63], pubs[48 * 11], key[48];
  for (int i = 0; i < 63; ++i) pub_of(com + 48 * i, 1000003ull * (i + 1));
  int64_t ids[11];
  for (int i = 0; i < 11; ++i) ids[i] = i;
  int32_t st1;
  const ShareOps so = run_share(com, 1, 9, 7, ids, 11, pubs, &st1);
  CHECK(st1 == HIPBLS_OK, "the counting call failed");
  uint64_t rec[2], sums[2];
  for (int path = 0; path < 2; ++path) {
    int64_t gid[7];
    const uint64_t offs[2] = {0, 7};
    for (int k = 0; k < 7; ++k) gid[k] = (path ? ((int64_t)1 << 40) : 0) + k + 1;
    std::vector<uint64_t> by_share;
    const uint64_t t0 = ops();
    run_recover(pubs + 48, gid, offs, 1, key, &st1, &by_share);
    const uint64_t total = ops() - t0;
    rec[path] = 0;
    for (uint64_t x : by_share) rec[path] += x;
    sums[path] = total - rec[path];
    rec[path] /= 7;
    CHECK(st1 == HIPBLS_OK, "the counting group failed");
    if (path == 0) CHECK(!std::memcmp(key, pubs, 48), "ids 1..7 do not recover the key at id 0");
  }
  if (g_fail) {
    std::printf("vss_host: %d checks failed\n", g_fail);
    return 1;
  }
  std::printf("vss_host ok: %zu share calls (%zu lanes), %zu groups; products + squarings: decode %llu per commitment, "
              "dealer sum %llu per coefficient (9 dealers), evaluation %llu per lane (7 coefficients, ids 0..10 mean), "
              "recovered share %llu small path / %llu field path, group sum %llu / %llu\n",
              g_calls.size(), lanes, n_groups, (unsigned long long)(so.decode / 63), (unsigned long long)(so.sum / 7),
              (unsigned long long)(so.eval / 11), (unsigned long long)rec[0], (unsigned long long)rec[1],
              (unsigned long long)sums[0], (unsigned long long)sums[1]);
  return 0;
}
