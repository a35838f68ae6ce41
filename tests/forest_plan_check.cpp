// Drives the device-free forest planner (phylostan_amd/csrc/forest_plan.h)
// under a host sanitizer (tests/test_forest_cpu.py builds it with
// -fsanitize=address,undefined).  With a file argument it also plans the
// peels of that file: "S T" then T x (S-1) x 3 ints, unrooted.
#include <cstdio>
#include <cstring>

#include "forest_plan.h"

static unsigned long long g_lcg = 2024;
static unsigned rnd(unsigned n) {
  g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned)(g_lcg >> 33) % n;
}

// kind 0 caterpillar, 1 balanced, 2 random; internal nodes numbered in creation order
static std::vector<int32_t> make_peel(int S, int kind, bool rooted) {
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
    if (live.size() == 2 && !rooted && b != 2 * S - 3) std::swap(a, b);
    live.erase(live.begin() + std::max(i, j));
    live.erase(live.begin() + std::min(i, j));
    if (kind == 1) live.push_back(nxt); else live.insert(live.begin(), nxt);
    if (kind == 2) std::swap(live[0], live[rnd((unsigned)live.size())]);
    peel.insert(peel.end(), {a, b, nxt});
  }
  return peel;
}

static int g_bad = 0;
static void expect(bool ok, const char* what) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s: %s\n", what, g_err.c_str());
  ++g_bad;
}
static bool refused_naming(int rc, const char* part) {
  return rc == PHY_EINVAL && g_err.find(part) != std::string::npos;
}

static std::vector<uint8_t> make_tips(int S, int P) {
  std::vector<uint8_t> tips((size_t)S * P);
  for (auto& t : tips) t = rnd(16) == 0 ? 15 : (uint8_t)(1 << rnd(4));
  return tips;
}

int main(int argc, char** argv) {
  long plans = 0;
  // T = 1: the records, mat_branch and gpos are plan_lds's / make_problem's, byte for byte
  for (int S : {3, 8, 24, 69})
    for (int kind = 0; kind < 3; ++kind)
      for (int rooted = 0; rooted < 2; ++rooted)
        for (int C : {1, 4})
          for (int variant = 0; variant < 4; ++variant) {
            const int P = 130, max_rows = variant == 3 ? 1 : 100;
            const std::vector<int32_t> peel = make_peel(S, kind, rooted != 0);
            const std::vector<uint8_t> tips = make_tips(S, P);
            const std::vector<double> w(P, 1.0);
            Prefs prefs;
            if (variant == 1) prefs.lds_budget = 16384, prefs.recompute = false;
            if (variant == 2) prefs.cols = 1, prefs.deep = 2;
            Problem pb;
            SweepPlan one;
            expect(make_problem(S, P, C, rooted, PHY_HKY, tips.data(), w.data(), peel.data(), max_rows, pb) == PHY_OK,
                   "make_problem");
            expect(plan_lds(pb, prefs, 256, one) == PHY_OK, "plan_lds");
            ForestPlan fp;
            expect(forest_plan(S, P, C, rooted, PHY_HKY, tips.data(), w.data(), 1, peel.data(), max_rows, prefs, 256, fp) ==
                       PHY_OK,
                   "forest_plan T = 1");
            ++plans;
            expect(fp.records == one.records && fp.mat_branch == pb.mat_branch && fp.gpos == pb.gpos, "T = 1 tables");
            expect(fp.plan.K == one.K && fp.plan.lat == one.lat && fp.plan.cap_m == one.cap_m && fp.plan.ndl == one.ndl &&
                       fp.plan.lds == one.lds && fp.nchunks[0] == one.nchunks && fp.nrec[0] == one.nrec &&
                       fp.rec_stride == (int)one.records.size(),
                   "T = 1 plan");
          }
  // a caterpillar (depth 0) beside a balanced tree and random ones: one cap, per-tree chunk counts and depths
  for (int S : {8, 24, 69})
    for (int rooted = 0; rooted < 2; ++rooted) {
      const int P = 70, C = 4, T = 5;
      std::vector<int32_t> peels;
      for (int t = 0; t < T; ++t) {
        const std::vector<int32_t> p = make_peel(S, t < 2 ? t : 2, rooted != 0);
        peels.insert(peels.end(), p.begin(), p.end());
      }
      const std::vector<uint8_t> tips = make_tips(S, P);
      const std::vector<double> w(P, 1.0);
      for (int budget : {0, 16384}) {
        Prefs prefs;
        prefs.lds_budget = budget;
        ForestPlan fp;
        expect(forest_plan(S, P, C, rooted, PHY_GTR, tips.data(), w.data(), T, peels.data(), 64, prefs, 256, fp) == PHY_OK,
               "forest_plan mixed");
        ++plans;
        expect(fp.min_depth == 0 && fp.ndeep[0] == 0 && fp.max_depth > 0 && fp.pb.ndeep == fp.max_depth, "depths");
        expect((int)fp.records.size() == T * fp.rec_stride && (int)fp.mat_branch.size() == T * fp.pb.B &&
                   (int)fp.gpos.size() == T * fp.pb.B,
               "table sizes");
        // every tree's records are what its own chunk plan at the common cap gives
        for (int t = 0; t < T; ++t) {
          std::vector<int> prog, mb;
          int ns = 0, nd = 0, nch = 0, nrec = 0;
          expect(build_program(S, &peels[(size_t)t * 3 * (S - 1)], rooted, prog, mb, ns, nd) == PHY_OK, "build_program");
          expect(assign_chunks(prog, S - 1, (int)mb.size(), fp.plan.cap_m, prefs.recompute, nch, nrec) == PHY_OK, "chunks");
          const std::vector<int> recs = fp.plan.K == 2 ? batched_records(prog, 2, C, fp.pb.R) : pack_program(prog);
          expect(nch == fp.nchunks[t] && nd == fp.ndeep[t] &&
                     std::equal(recs.begin(), recs.end(), fp.records.begin() + (size_t)t * fp.rec_stride) &&
                     std::equal(mb.begin(), mb.end(), fp.mat_branch.begin() + (size_t)t * fp.pb.B),
                 "per-tree tables");
          for (int m = 0; m < fp.pb.B; ++m) expect(fp.gpos[(size_t)t * fp.pb.B + mb[m]] == m, "gpos");
        }
        if (budget && S >= 24) expect(fp.max_chunks >= 2, "chunked under a small budget");
      }
    }
  // refusals, each naming its tree where one is at fault
  {
    const int S = 8, P = 20, C = 2;
    const std::vector<uint8_t> tips = make_tips(S, P);
    const std::vector<double> w(P, 1.0);
    std::vector<int32_t> peels;
    for (int t = 0; t < 4; ++t) {
      const std::vector<int32_t> p = make_peel(S, 2, false);
      peels.insert(peels.end(), p.begin(), p.end());
    }
    const Prefs prefs;
    ForestPlan fp;
    auto plan = [&](int s, int p, int c, int kind, const uint8_t* tp, const double* wp, int T, const int32_t* pl, int mr) {
      return forest_plan(s, p, c, 0, kind, tp, wp, T, pl, mr, prefs, 256, fp);
    };
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 0, peels.data(), 8), "T >= 1"), "T = 0");
    expect(refused_naming(plan(2, P, C, PHY_JC69, tips.data(), w.data(), 4, peels.data(), 8), "S >= 3"), "S");
    expect(refused_naming(plan(S, 0, C, PHY_JC69, tips.data(), w.data(), 4, peels.data(), 8), "P >= 1"), "P");
    expect(refused_naming(plan(S, P, 17, PHY_JC69, tips.data(), w.data(), 4, peels.data(), 8), "C must"), "C");
    expect(refused_naming(plan(S, P, C, 7, tips.data(), w.data(), 4, peels.data(), 8), "unknown model"), "model");
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, peels.data(), 0), "max_rows"), "max_rows");
    expect(refused_naming(plan(S, P, C, PHY_JC69, nullptr, w.data(), 4, peels.data(), 8), "NULL"), "NULL tips");
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, nullptr, 8), "NULL"), "NULL peels");
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 1 << 22, peels.data(), 8), "256 MiB"), "tables");
    std::vector<uint8_t> badtips = tips;
    badtips[5] = 16;
    expect(refused_naming(plan(S, P, C, PHY_JC69, badtips.data(), w.data(), 4, peels.data(), 8), "tip code"), "tip code");
    const size_t L = (size_t)3 * (S - 1);
    std::vector<int32_t> bad = peels;
    bad[2 * L + 1] = 99;  // tree 2: a child out of range
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, bad.data(), 8), "tree 2: peel row 0"), "range");
    bad = peels;
    bad[3 * L + 3] = bad[3 * L + 0];  // tree 3: a node used as a child twice
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, bad.data(), 8), "tree 3: "), "child twice");
    bad = peels;
    std::swap(bad[1 * L + L - 3], bad[1 * L + L - 2]);  // tree 1: the last row's children swapped
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, bad.data(), 8), "tree 1: unrooted peel"),
           "last-row rule");
    expect(plan(S, P, C, PHY_JC69, tips.data(), w.data(), 4, peels.data(), 8) == PHY_OK, "the unspoilt forest");
    ++plans;
  }
  // the peels of a file (the DS1 topologies)
  if (argc > 1) {
    FILE* f = std::fopen(argv[1], "r");
    int S = 0, T = 0;
    if (!f || std::fscanf(f, "%d %d", &S, &T) != 2 || S < 3 || T < 1) {
      std::fprintf(stderr, "cannot read %s\n", argv[1]);
      return 2;
    }
    std::vector<int32_t> peels((size_t)T * 3 * (S - 1));
    for (auto& v : peels)
      if (std::fscanf(f, "%d", &v) != 1) return 2;
    std::fclose(f);
    const int P = 300;
    const std::vector<uint8_t> tips = make_tips(S, P);
    const std::vector<double> w(P, 1.0);
    for (int max_rows : {1, T, 100 * T}) {
      ForestPlan fp;
      expect(forest_plan(S, P, 1, 0, PHY_JC69, tips.data(), w.data(), T, peels.data(), max_rows, Prefs(), 256, fp) == PHY_OK,
             "file forest");
      expect(fp.T == T && (int)fp.records.size() == T * fp.rec_stride, "file forest tables");
      ++plans;
      std::printf("file forest: T %d max_rows %d K %d cap_m %d chunks %d..%d depth %d..%d fin %d qf %d\n", T, max_rows,
                  fp.plan.K, fp.plan.cap_m, fp.min_chunks, fp.max_chunks, fp.min_depth, fp.max_depth, fp.fin, fp.qf);
    }
  }
  std::printf("forest_plan_check: %ld plans, %d failures\n", plans, g_bad);
  return g_bad ? 1 : 0;
}
