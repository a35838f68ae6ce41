// Drives the device-free planner of the discrete-trait engine
// (phylostan_amd/csrc/geo_plan.h) over generated trees under a host sanitizer
// (tests/test_geo_cpu.py builds it with -fsanitize=address,undefined).  Every
// plan is checked as a schedule (each row once, children on lower levels, the
// root row alone on top), its LDS layout against the 160 KiB, and every refusal
// of phy_geo_create as PHY_EINVAL with a message.
#include <cstdio>

#include "geo_plan.h"

static unsigned long long g_lcg = 4711;
static unsigned rnd(unsigned n) {
  g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned)(g_lcg >> 33) % n;
}

// kind 0 caterpillar, 1 balanced, 2 random; internal nodes in creation order, last row (x, 2S-3, 2S-2)
static std::vector<int32_t> make_peel(int S, int kind) {
  std::vector<int> live(S);
  for (int i = 0; i < S; ++i) live[i] = i;
  std::vector<int32_t> peel;
  for (int nxt = S; live.size() > 1; ++nxt) {
    size_t i = 0, j = 1;
    if (kind == 0 && nxt > S) i = live.size() - 1, j = 0;
    if (kind == 2) {
      i = rnd((unsigned)live.size());
      j = rnd((unsigned)live.size() - 1);
      if (j >= i) ++j;
    }
    int a = live[i], b = live[j];
    if (live.size() == 2 && b != 2 * S - 3) std::swap(a, b);
    live.erase(live.begin() + std::max(i, j));
    live.erase(live.begin() + std::min(i, j));
    if (kind == 1) live.push_back(nxt); else live.insert(live.begin(), nxt);
    if (kind == 2) std::swap(live[0], live[rnd((unsigned)live.size())]);
    peel.insert(peel.end(), {a, b, nxt});
  }
  return peel;
}

static int g_bad = 0;
static void expect(bool ok, const char* what, int S, int K) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (S %d K %d): %s\n", what, S, K, g_err.c_str());
  ++g_bad;
}
static bool refused(int rc) { return rc == PHY_EINVAL && !g_err.empty(); }

static void check_plan(const GeoPlan& p, const std::vector<int32_t>& peel, int S, int K, int max_draws) {
  const int N = 2 * S - 1;
  expect(p.B == 2 * S - 3 && p.N == N && p.R == K * (K - 1) / 2, "sizes", S, K);
  expect((int)p.lvl_off.size() == p.nlev + 1 && p.lvl_off[0] == 0 && p.lvl_off[p.nlev] == S - 1, "level offsets", S, K);
  expect((int)p.rows.size() == (S - 1) * GR_INTS, "row count", S, K);
  std::vector<int> level(N, -1), seen(N, 0);
  for (int t = 0; t < S; ++t) level[t] = 0;
  int widest = 0;
  for (int l = 0; l < p.nlev; ++l) {
    expect(p.lvl_off[l] < p.lvl_off[l + 1], "empty level", S, K);
    widest = std::max(widest, p.lvl_off[l + 1] - p.lvl_off[l]);
    for (int r = p.lvl_off[l]; r < p.lvl_off[l + 1]; ++r) {
      const int32_t* w = &p.rows[(size_t)r * GR_INTS];
      expect(level[w[GR_A]] >= 0 && level[w[GR_A]] <= l && level[w[GR_B]] >= 0 && level[w[GR_B]] <= l,
             "child not on a lower level", S, K);
      expect(w[GR_LAST] == (w[GR_P] == 2 * S - 2), "last flag", S, K);
      ++seen[w[GR_P]];
    }
    for (int r = p.lvl_off[l]; r < p.lvl_off[l + 1]; ++r) level[p.rows[(size_t)r * GR_INTS + GR_P]] = l + 1;
  }
  for (int v = S; v < N; ++v) expect(seen[v] == 1, "a row missing or doubled", S, K);
  expect(p.lvl_off[p.nlev] - p.lvl_off[p.nlev - 1] == 1 && p.rows[(size_t)(S - 2) * GR_INTS + GR_LAST] == 1,
         "root row not alone on top", S, K);
  expect(widest == p.widest, "widest level", S, K);
  const GeoLds L(K);
  expect(L.KP % 2 == 1 && L.KP >= K, "row stride", S, K);
  expect(L.V() >= K * L.KP && L.W() - L.V() >= K * L.KP && L.vecs(0) - L.W() >= K * L.KP, "matrices overlap", S, K);
  expect(L.vecs(1) - L.vecs(0) >= K && L.cs() >= L.vecs(GEO_NVEC - 1) + K, "vectors overlap", S, K);
  expect(p.lds_bytes == (size_t)L.doubles() * 8 && p.lds_bytes <= GEO_LDS_CAP, "LDS bytes", S, K);
  expect(p.threads == 256 || p.threads == GEO_MAX_THREADS, "threads", S, K);
  expect((p.threads & (p.threads - 1)) == 0 && p.threads / 2 >= K / 2, "threads cover a round's pairs", S, K);
  expect(p.ws_doubles >= (size_t)GEO_WS_ARRAYS * N * K + 2 * (size_t)N, "workspace", S, K);
  expect(p.workgroups >= 1 && p.workgroups <= max_draws, "workgroups", S, K);
  expect((size_t)p.workgroups * p.ws_doubles * 8 <= GEO_WS_BUDGET || p.workgroups == 1, "workspace budget", S, K);
  (void)peel;
}

int main() {
  long plans = 0, refusals = 0;
  for (int S : {3, 4, 5, 12, 69, 200, 700})
    for (int kind = 0; kind < 3; ++kind) {
      const std::vector<int32_t> peel = make_peel(S, kind);
      for (int K : {2, 3, 4, 5, 17, 33, 64})
        for (int max_draws : {1, 100, 5000}) {
          GeoPlan p;
          const int rc = geo_plan(S, K, peel.data(), max_draws, 256, p);
          expect(rc == PHY_OK, "geo_plan", S, K);
          if (rc == PHY_OK) check_plan(p, peel, S, K, max_draws);
          ++plans;
          if (kind == 0 && rc == PHY_OK) expect(p.nlev == S - 1 && p.widest == 1, "caterpillar: one node per level", S, K);
        }
      GeoPlan p;
      // the refusals
      expect(refused(geo_plan(S, 1, peel.data(), 4, 256, p)), "K = 1 accepted", S, 1);
      expect(refused(geo_plan(S, 65, peel.data(), 4, 256, p)), "K = 65 accepted", S, 65);
      expect(refused(geo_plan(S, 0, peel.data(), 4, 256, p)), "K = 0 accepted", S, 0);
      expect(refused(geo_plan(2, 4, peel.data(), 4, 256, p)), "S = 2 accepted", 2, 4);
      expect(refused(geo_plan(S, 4, nullptr, 4, 256, p)), "NULL peel accepted", S, 4);
      expect(refused(geo_plan(S, 4, peel.data(), 0, 256, p)), "max_draws = 0 accepted", S, 4);
      refusals += 6;
      for (int bad = 0; bad < 6; ++bad) {
        std::vector<int32_t> q = peel;
        const size_t last = (size_t)(S - 2) * 3;
        switch (bad) {
          case 0: q[0] = 2 * S + 5; break;               // id out of range
          case 1: q[1] = q[0]; break;                    // the same child twice
          case 2: q[last + 1] = q[last]; q[last] = 2 * S - 3; break;  // merged child first
          case 3: q[2] = 2 * S - 2; break;               // the root made early
          case 4: q[0] = -1; break;                      // negative id
          case 5: if (S > 3) q[3] = q[0]; else q[0] = 2 * S - 2; break;  // a child with two parents / used before made
        }
        expect(refused(geo_plan(S, 4, q.data(), 4, 256, p)), "malformed peel accepted", S, bad);
        ++refusals;
      }
    }
  std::printf("geo_plan_check: %ld plans, %ld refusals, %d failures\n", plans, refusals, g_bad);
  return g_bad ? 1 : 0;
}
