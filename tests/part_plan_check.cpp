// Drives the device-free planner of the partitioned engine
// (phylostan_amd/csrc/part_plan.h) under a host sanitizer
// (tests/test_part_cpu.py builds it with -fsanitize=address,undefined).  The
// block ranges and the padded-column map are held against statements that walk
// the padded alignment column by column instead of reusing the planner's
// arithmetic.
#include <cstdio>
#include <cstring>
#include <set>

#include "part_plan.h"

// a caterpillar on S tips; internal nodes numbered in creation order
static std::vector<int32_t> make_peel(int S, bool rooted) {
  std::vector<int32_t> peel = {0, 1, S};
  for (int k = 2; k < S; ++k) peel.insert(peel.end(), {S + k - 2, k, S + k - 1});
  if (!rooted) {  // the last row's second child is node 2S-3
    const size_t r = peel.size() - 3;
    if (peel[r + 1] != 2 * S - 3) std::swap(peel[r], peel[r + 1]);
  }
  return peel;
}

static int g_bad = 0;
static void expect(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s: %s\n", what, g_err.c_str());
  ++g_bad;
}
static bool refused_naming(int rc, const char* part) { return rc == PHY_EINVAL && g_err.find(part) != std::string::npos; }

// codes[k]: the tip codes partition k draws from
static std::vector<uint8_t> make_tips(int S, const std::vector<int>& Pk, const std::vector<std::vector<int>>& codes) {
  int psum = 0;
  for (int p : Pk) psum += p;
  std::vector<uint8_t> tips((size_t)S * psum);
  unsigned long long lcg = 99;
  for (int t = 0; t < S; ++t) {
    int off = 0;
    for (size_t k = 0; k < Pk.size(); ++k) {
      for (int i = 0; i < Pk[k]; ++i) {
        lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
        const std::vector<int>& cs = codes[k % codes.size()];
        tips[(size_t)t * psum + off + i] = (uint8_t)cs[(size_t)(lcg >> 33) % cs.size()];
      }
      off += Pk[k];
    }
  }
  return tips;
}

static long check(int S, const std::vector<int>& Pk, int C, int rooted, int max_draws, int cols) {
  const int K = (int)Pk.size();
  const std::vector<std::vector<int>> codes = {{1, 2, 4, 8}, {1, 2, 4, 8, 15, 3, 5, 10, 6}};
  const std::vector<uint8_t> tips = make_tips(S, Pk, codes);
  int psum = 0;
  for (int p : Pk) psum += p;
  std::vector<double> w(psum);
  for (int i = 0; i < psum; ++i) w[i] = 1.0 + i % 3;
  const std::vector<int32_t> peel = make_peel(S, rooted != 0);
  std::vector<int32_t> pk32(Pk.begin(), Pk.end());
  Prefs prefs;
  prefs.cols = cols;
  PartPlan pp;
  expect(part_plan(S, K, pk32.data(), C, rooted, PHY_GTR, tips.data(), w.data(), peel.data(), max_draws, prefs, 256, pp) == PHY_OK,
         "part_plan");
  if (g_bad) return 1;
  const int P = pp.pb.P, bw = 64 * pp.plan.K;
  expect(cols == 0 || pp.plan.K == cols, "the forced column plan");
  expect(pp.pb.max_draws == max_draws * K && pp.Psum == psum, "rows and patterns");
  expect((int)pp.col_part.size() == P && (int)pp.col_pat.size() == P && (int)pp.pb.tips.size() == S * P, "sizes");
  // the map, column by column: partitions in order, patterns in order, gaps of mask 15 and weight 0 between them,
  // every partition's first column on a 128-column boundary, no trailing gap
  int k = -1, next = 0, seen = 0;
  std::vector<int> first(K, -1), last(K, -1);
  for (int c = 0; c < P; ++c) {
    const int part = pp.col_part[c], pat = pp.col_pat[c];
    if (part < 0) {
      expect(pat == -1 && pp.pb.w[c] == 0.0, "a gap column has no pattern and weight 0");
      for (int t = 0; t < S; ++t) expect(pp.pb.tips[(size_t)t * P + c] == 15, "a gap column is all mask 15");
      expect(k >= 0 && next == Pk[k], "a gap only after a whole partition");
      continue;
    }
    if (part != k) {
      expect(part == k + 1 && (k < 0 || next == Pk[k]) && pat == 0, "partitions in order, each whole");
      expect(c % 128 == 0, "a partition starts on a 128-column boundary");
      k = part;
      next = 0;
      first[k] = c;
      expect(pp.col0[k] == c, "col0");
    }
    expect(pat == next, "patterns in order");
    int off = 0;
    for (int j = 0; j < k; ++j) off += Pk[j];
    expect(pp.off[k] == off && pp.pb.w[c] == w[off + pat], "the caller's weight");
    for (int t = 0; t < S; ++t)
      expect(pp.pb.tips[(size_t)t * P + c] == tips[(size_t)t * psum + off + pat], "the caller's tip code");
    last[k] = c;
    ++next;
    ++seen;
  }
  expect(k == K - 1 && next == Pk[K - 1] && seen == psum && pp.col_part[P - 1] == K - 1, "every pattern once, no trailing gap");
  // block ranges: exactly the blocks that hold a column of the partition, and no block holds two partitions
  expect((int)pp.blk.size() == 2 * K && pp.plan.nblk == (P + bw - 1) / bw, "block table");
  for (int b = 0; b < pp.plan.nblk; ++b) {
    std::set<int> owners;
    for (int c = b * bw; c < std::min(P, (b + 1) * bw); ++c)
      if (pp.col_part[c] >= 0) owners.insert(pp.col_part[c]);
    expect(owners.size() <= 1, "a block holds columns of one partition at most");
    for (int j = 0; j < K; ++j) {
      const bool in = b >= pp.blk[2 * j] && b < pp.blk[2 * j + 1];
      expect(in == (owners.count(j) == 1), "a partition's range is exactly the blocks holding its columns");
    }
  }
  for (int j = 0; j < K; ++j)
    expect(pp.blk[2 * j] == first[j] / bw && pp.blk[2 * j + 1] == last[j] / bw + 1 && pp.blk[2 * j + 1] <= pp.plan.nblk &&
               (size_t)pp.blk[2 * j + 1] * bw <= (size_t)pp.pb.Ppad,
           "block range from the first and last column, inside the padded tips");
  // R and extra are the union's: 15 always, 3 5 10 6 when an ambiguous partition exists
  {
    std::set<int> masks;
    for (uint8_t t : tips)
      if (t != 1 && t != 2 && t != 4 && t != 8) masks.insert(t);
    masks.insert(15);
    std::set<int> got;
    for (int r = 4; r < pp.pb.R; ++r) got.insert((int)((pp.pb.extra >> (4 * (r - 4))) & 15));
    expect(got == masks && pp.pb.R == 4 + (int)masks.size(), "R and extra of the union of the tip masks");
  }
  expect(pp.fin == 0 || pp.fin == 1, "epilogue form");
  return 1;
}

int main() {
  long plans = 0;
  const std::vector<std::vector<int>> widths = {{1}, {1, 1}, {63, 65}, {64, 128, 129}, {127, 1, 200}, {130, 3, 64, 257},
                                                {128, 128}, {129, 1, 1, 1, 640}};
  for (const auto& Pk : widths)
    for (int S : {3, 7, 12})
      for (int C : {1, 4})
        for (int rooted = 0; rooted < 2; ++rooted)
          for (int max_draws : {1, 64, 300})
            for (int cols : {0, 1, 2}) plans += check(S, Pk, C, rooted, max_draws, cols);
  // refusals
  {
    const int S = 8, C = 2;
    const std::vector<int> Pk = {20, 30};
    const std::vector<uint8_t> tips = make_tips(S, Pk, {{1, 2, 4, 8}});
    const std::vector<double> w(50, 1.0);
    const std::vector<int32_t> peel = make_peel(S, false);
    PartPlan pp;
    const Prefs prefs;
    auto plan = [&](int s, int K, const std::vector<int32_t>& pk, int c, int kind, const uint8_t* tp, const int32_t* pl, int md) {
      return part_plan(s, K, pk.data(), c, 0, kind, tp, w.data(), pl, md, prefs, 256, pp);
    };
    const std::vector<int32_t> ok = {20, 30};
    expect(refused_naming(plan(S, 0, ok, C, PHY_JC69, tips.data(), peel.data(), 8), "K >= 1"), "K");
    expect(refused_naming(plan(S, 2, {20, 0}, C, PHY_JC69, tips.data(), peel.data(), 8), "partition 1"), "empty partition");
    expect(refused_naming(plan(S, 2, {-3, 30}, C, PHY_JC69, tips.data(), peel.data(), 8), "partition 0"), "negative P_k");
    expect(refused_naming(plan(S, 2, ok, C, PHY_JC69, tips.data(), peel.data(), 32768), "65535"), "grid rows");
    expect(plan(S, 2, ok, C, PHY_JC69, tips.data(), peel.data(), 32767) == PHY_OK, "65534 rows pass");
    ++plans;
    expect(refused_naming(plan(S, 2, ok, C, PHY_JC69, tips.data(), peel.data(), 0), "max_draws"), "max_draws");
    expect(refused_naming(plan(2, 2, ok, C, PHY_JC69, tips.data(), peel.data(), 8), "S >= 3"), "S");
    expect(refused_naming(plan(S, 2, ok, 17, PHY_JC69, tips.data(), peel.data(), 8), "C must"), "C");
    expect(refused_naming(plan(S, 2, ok, C, 7, tips.data(), peel.data(), 8), "unknown model"), "model");
    expect(refused_naming(plan(S, 2, ok, C, PHY_JC69, nullptr, peel.data(), 8), "NULL"), "NULL tips");
    expect(refused_naming(plan(S, 2, ok, C, PHY_JC69, tips.data(), nullptr, 8), "NULL"), "NULL peel");
    std::vector<uint8_t> badtips = tips;
    badtips[5] = 16;
    expect(refused_naming(plan(S, 2, ok, C, PHY_JC69, badtips.data(), peel.data(), 8), "tip code"), "tip code");
    std::vector<int32_t> bad = peel;
    bad[1] = 99;  // a child out of range
    expect(plan(S, 2, ok, C, PHY_JC69, tips.data(), bad.data(), 8) == PHY_EINVAL, "malformed tree");
    expect(plan(S, 2, ok, C, PHY_JC69, tips.data(), peel.data(), 8) == PHY_OK, "the unspoilt arguments");
    ++plans;
  }
  std::printf("part_plan_check: %ld plans, %d failures\n", plans, g_bad);
  return g_bad ? 1 : 0;
}
