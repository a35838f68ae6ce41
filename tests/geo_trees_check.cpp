// Drives the device-free planner of the tree-sample engine
// (phylostan_amd/csrc/geo_plan.h, geo_trees_plan) over generated samples under
// a host sanitizer (tests/test_geo_trees_cpu.py builds it with
// -fsanitize=address,undefined).  Every tree's schedule is checked against a
// brute-force levelisation of its peel, the tree -> group partition as a
// partition that does not depend on max_draws, the budgets, and every refusal
// as PHY_EINVAL with a message that names the tree.
#include <cstdio>
#include <cstring>

#include "geo_plan.h"

static unsigned long long g_lcg = 90210;
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
static void expect(bool ok, const char* what, int S, int T) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (S %d T %d): %s\n", what, S, T, g_err.c_str());
  ++g_bad;
}
static bool refused_naming(int rc, int tree) {
  const std::string want = "tree " + std::to_string(tree) + ":";
  return rc == PHY_EINVAL && g_err.find(want) != std::string::npos;
}

// levels by repeated relaxation over the rows in any order: shares nothing with the planner's single pass
static std::vector<int> brute_levels(const int32_t* peel, int S) {
  std::vector<int> level(2 * S - 1, 0);
  for (bool moved = true; moved;) {
    moved = false;
    for (int r = S - 2; r >= 0; --r) {
      const int want = 1 + std::max(level[peel[3 * r]], level[peel[3 * r + 1]]);
      if (level[peel[3 * r + 2]] != want) level[peel[3 * r + 2]] = want, moved = true;
    }
  }
  return level;
}

static void check_sample(const GeoTreesPlan& p, const std::vector<int32_t>& peels, int S, int K, int T, int cus) {
  const int N = 2 * S - 1;
  expect(p.S == S && p.K == K && p.T == T && p.B == 2 * S - 3 && p.N == N && p.R == K * (K - 1) / 2, "sizes", S, T);
  expect((int)p.lvl_start.size() == T + 1 && p.lvl_start[0] == 0 && p.lvl_start[T] == (int)p.lvl_off.size(),
         "level block offsets", S, T);
  expect(p.rows.size() == (size_t)T * (S - 1) * GR_INTS, "row blocks", S, T);
  int widest = 0, deepest = 0;
  for (int t = 0; t < T; ++t) {
    const int32_t* peel = &peels[(size_t)t * (S - 1) * 3];
    const std::vector<int> level = brute_levels(peel, S);
    const int nlev = p.lvl_start[t + 1] - p.lvl_start[t] - 1;
    const int32_t* lvl = &p.lvl_off[p.lvl_start[t]];
    const int32_t* rows = &p.rows[(size_t)t * (S - 1) * GR_INTS];
    expect(nlev == level[N - 1] && lvl[0] == 0 && lvl[nlev] == S - 1, "level count", S, t);
    deepest = std::max(deepest, nlev);
    std::vector<int> seen(N, 0);
    for (int l = 0; l < nlev; ++l) {
      expect(lvl[l] < lvl[l + 1], "empty level", S, t);
      widest = std::max(widest, lvl[l + 1] - lvl[l]);
      for (int r = lvl[l]; r < lvl[l + 1]; ++r) {
        const int32_t* w = rows + (size_t)r * GR_INTS;
        expect(level[w[GR_P]] == l + 1, "a row on the wrong level", S, t);
        expect(w[GR_LAST] == (w[GR_P] == N - 1), "last flag", S, t);
        bool found = false;  // the row is a row of this tree's peel
        for (int q = 0; q < S - 1; ++q)
          found |= peel[3 * q] == w[GR_A] && peel[3 * q + 1] == w[GR_B] && peel[3 * q + 2] == w[GR_P];
        expect(found, "a row that is not the tree's", S, t);
        ++seen[w[GR_P]];
      }
    }
    for (int v = S; v < N; ++v) expect(seen[v] == 1, "a row missing or doubled", S, t);
  }
  expect(widest == p.widest && deepest == p.max_nlev, "widest level / level count over trees", S, T);
  // the partition: consecutive, every tree exactly once, no empty group
  const int per_cu = p.lds_bytes * 2 <= GEO_LDS_CAP ? 2 : 1;  // resident workgroups per CU
  expect(p.G >= 1 && p.G <= T && p.G <= per_cu * cus && p.G <= GEO_MAX_THREADS, "G", S, T);
  expect((int)p.grp_off.size() == p.G + 1 && p.grp_off[0] == 0 && p.grp_off[p.G] == T, "group offsets", S, T);
  std::vector<int> owner(T, 0);
  for (int g = 0; g < p.G; ++g) {
    expect(p.grp_off[g] < p.grp_off[g + 1], "empty group", S, T);
    for (int t = p.grp_off[g]; t < p.grp_off[g + 1] && t < T; ++t) ++owner[t];
  }
  for (int t = 0; t < T; ++t) expect(owner[t] == 1, "a tree in no group or in two", S, t);
  // budgets
  expect(p.workgroups >= 1 && p.workgroups <= per_cu * cus && (K < 64 || per_cu == 1), "workgroups", S, T);
  expect((size_t)p.workgroups * p.ws_doubles * 8 <= GEO_WS_BUDGET || p.workgroups == 1, "workspace budget", S, T);
  expect(p.ws_doubles >= (size_t)GEO_WS_ARRAYS * N * K + 2 * (size_t)N, "workspace", S, T);
  expect(p.chunk_draws >= 1, "chunk", S, T);
  expect((size_t)p.chunk_draws * p.G * p.slot_doubles * 8 <= GEO_TREES_SLOT_BUDGET || p.chunk_draws == 1, "slot budget",
         S, T);
  expect(p.slot_doubles == (size_t)GS_HEAD + (size_t)K * K + 2 * K && p.rec_doubles == (size_t)GT_HEAD + 2 * K + (size_t)K * K,
         "slot and record sizes", S, T);
  expect(p.data_bytes <= GEO_TREES_DATA_BUDGET, "data budget", S, T);
  expect(p.lds_bytes == (size_t)GeoLds(K).doubles() * 8 && p.lds_bytes <= GEO_LDS_CAP, "LDS bytes", S, T);
  expect(p.threads == (K <= 16 ? 256 : GEO_MAX_THREADS), "threads", S, T);
}

int main() {
  long plans = 0, refusals = 0;
  for (int S : {3, 4, 7, 12, 69, 300})
    for (int T : {1, 2, 3, 7, 255, 256, 257, 513, 1100}) {
      if ((long)S * T > 40000) continue;
      std::vector<int32_t> peels;
      for (int t = 0; t < T; ++t) {
        const std::vector<int32_t> one = make_peel(S, t % 3);
        peels.insert(peels.end(), one.begin(), one.end());
      }
      for (int K : {2, 5, 64})
        for (int cus : {1, 8, 256, 1000}) {
          GeoTreesPlan a, b;
          const int ra = geo_trees_plan(S, K, T, peels.data(), 1, cus, a);
          const int rb = geo_trees_plan(S, K, T, peels.data(), 300, cus, b);
          expect(ra == PHY_OK && rb == PHY_OK, "geo_trees_plan", S, T);
          if (ra != PHY_OK || rb != PHY_OK) continue;
          check_sample(a, peels, S, K, T, cus);
          check_sample(b, peels, S, K, T, cus);
          // what decides a draw's sums does not depend on max_draws
          expect(a.G == b.G && a.grp_off == b.grp_off && a.rows == b.rows && a.lvl_off == b.lvl_off &&
                     a.lvl_start == b.lvl_start && a.workgroups == b.workgroups,
                 "the partition depends on max_draws", S, T);
          expect(a.chunk_draws == 1 && b.chunk_draws <= 300, "chunk over max_draws", S, T);
          plans += 2;
        }
      // the refusals, each naming its tree
      GeoTreesPlan p;
      if (T >= 3) {
        const size_t at = (size_t)2 * (S - 1) * 3;  // tree 2
        for (int bad = 0; bad < 4; ++bad) {
          std::vector<int32_t> q = peels;
          const size_t last = at + (size_t)(S - 2) * 3;
          switch (bad) {
            case 0: q[at] = 2 * S + 5; break;                              // id out of range
            case 1: q[at + 1] = q[at]; break;                              // the same child twice
            case 2: q[last + 1] = q[last]; q[last] = 2 * S - 3; break;     // merged child first
            case 3: q[at + 2] = 2 * S - 2; break;                          // the root made early
          }
          expect(refused_naming(geo_trees_plan(S, 4, T, q.data(), 4, 256, p), 2), "malformed tree 2 accepted", S, bad);
          ++refusals;
        }
        std::vector<int32_t> q = peels;
        q[(size_t)(T - 1) * (S - 1) * 3] = -1;
        expect(refused_naming(geo_trees_plan(S, 4, T, q.data(), 4, 256, p), T - 1), "malformed last tree accepted", S, T);
        ++refusals;
      }
      expect(refused_naming(geo_trees_plan(S, 65, T, peels.data(), 4, 256, p), 0), "K = 65 accepted", S, T);
      expect(refused_naming(geo_trees_plan(S, 1, T, peels.data(), 4, 256, p), 0), "K = 1 accepted", S, T);
      expect(refused_naming(geo_trees_plan(2, 4, T, peels.data(), 4, 256, p), 0), "S = 2 accepted", 2, T);
      expect(refused_naming(geo_trees_plan(S, 4, T, peels.data(), 0, 256, p), 0), "max_draws = 0 accepted", S, T);
      expect(geo_trees_plan(S, 4, 0, peels.data(), 4, 256, p) == PHY_EINVAL && g_err.find("T = 0") != std::string::npos,
             "T = 0 accepted", S, 0);
      expect(geo_trees_plan(S, 4, -3, peels.data(), 4, 256, p) == PHY_EINVAL, "T < 0 accepted", S, -3);
      expect(geo_trees_plan(S, 4, T, nullptr, 4, 256, p) == PHY_EINVAL && !g_err.empty(), "NULL peels accepted", S, T);
      refusals += 7;
    }
  {  // the data budget is checked from S and T before a tree is read: one tree's worth of peel is enough here
    const int S = 69;
    const std::vector<int32_t> one = make_peel(S, 1);
    const size_t per_tree = (size_t)(S - 1) * GR_INTS * 4 + (size_t)S * 4 + (size_t)(2 * S - 3) * 8 + 8;
    const int over = (int)(GEO_TREES_DATA_BUDGET / per_tree) + 1;
    GeoTreesPlan p;
    const int rc = geo_trees_plan(S, 4, over, one.data(), 4, 256, p);
    expect(rc == PHY_EINVAL && g_err.find(std::to_string(over)) != std::string::npos &&
               g_err.find(std::to_string(GEO_TREES_DATA_BUDGET)) != std::string::npos,
           "a sample over the data budget accepted, or refused without the numbers", S, over);
    ++refusals;
  }
  {  // the workspace budget caps the resident workgroups and with them G: 700 tips at K = 64
    const int S = 700, T = 150;
    std::vector<int32_t> peels;
    for (int t = 0; t < T; ++t) {
      const std::vector<int32_t> one = make_peel(S, 2);
      peels.insert(peels.end(), one.begin(), one.end());
    }
    GeoTreesPlan p;
    expect(geo_trees_plan(S, 64, T, peels.data(), 8, 256, p) == PHY_OK, "700 tips", S, T);
    check_sample(p, peels, S, 64, T, 256);
    expect(p.workgroups < T && p.G == p.workgroups, "the workspace budget does not cap G", S, T);
    ++plans;
  }
  std::printf("geo_trees_check: %ld plans, %ld refusals, %d failures\n", plans, refusals, g_bad);
  return g_bad ? 1 : 0;
}
