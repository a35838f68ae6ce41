// Drives the device-free planner of the sequence-summary engine
// (phylostan_amd/csrc/seqsum_plan.h) under a host sanitizer
// (tests/test_seqsum_cpu.py builds it with -fsanitize=address,undefined).
#include <cstdio>
#include <cstring>

#include "seqsum_plan.h"

// kind 0 caterpillar, 1 balanced; internal nodes numbered in creation order
static std::vector<int32_t> make_peel(int S, int kind, bool rooted) {
  std::vector<int> live(S);
  for (int i = 0; i < S; ++i) live[i] = i;
  std::vector<int32_t> peel;
  for (int nxt = S; live.size() > 1; ++nxt) {
    size_t i = 0, j = 1;
    if (kind == 0 && nxt > S) i = live.size() - 1, j = 0;
    int a = live[i], b = live[j];
    if (live.size() == 2 && !rooted && b != 2 * S - 3) std::swap(a, b);
    live.erase(live.begin() + std::max(i, j));
    live.erase(live.begin() + std::min(i, j));
    if (kind == 1) live.push_back(nxt); else live.insert(live.begin(), nxt);
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
static bool refused_naming(int rc, const char* part) { return rc == PHY_EINVAL && g_err.find(part) != std::string::npos; }

static std::vector<uint8_t> make_tips(int S, int P) {
  std::vector<uint8_t> tips((size_t)S * P);
  unsigned long long lcg = 77;
  for (auto& t : tips) {
    lcg = lcg * 6364136223846793005ULL + 1442695040888963407ULL;
    const unsigned r = (unsigned)(lcg >> 33);
    t = r % 16 == 0 ? 15 : (uint8_t)(1 << (r % 4));
  }
  return tips;
}

// the schedule: every internal node once, children before parents, the root last, the peel's child order kept
static void check_schedule(const SeqsumPlan& sp, int S, const std::vector<int32_t>& peel, bool rooted) {
  const int N = 2 * S - 1;
  std::vector<int> done(N, 0);
  for (int t = 0; t < S; ++t) done[t] = 1;
  expect((int)sp.steps.size() == (S - 1) * SEQ_STEP_INTS, "steps size");
  for (int s = 0; s < S - 1; ++s) {
    const int a = sp.steps[(size_t)s * SEQ_STEP_INTS], b = sp.steps[(size_t)s * SEQ_STEP_INTS + 1],
              v = sp.steps[(size_t)s * SEQ_STEP_INTS + 2];
    expect(v >= S && v < N && a >= 0 && a < N && b >= 0 && b < N, "step ids in range");
    if (!(v >= S && v < N && a >= 0 && a < N && b >= 0 && b < N)) return;
    expect(done[a] == 1 && done[b] == 1 && done[v] == 0, "children before parents, each node once");
    done[v] = 1;
    bool found = false;
    for (int r = 0; r < S - 1; ++r)
      if (peel[3 * r + 2] == v) found = peel[3 * r] == a && peel[3 * r + 1] == b;
    expect(found, "a step is its peel row");
  }
  expect(sp.steps[(size_t)(S - 2) * SEQ_STEP_INTS + 2] == sp.root && sp.root == 2 * S - 2, "the root is last");
  expect(sp.merged == (rooted ? -1 : 2 * S - 3), "merged node");
  expect(sp.pb.B == (rooted ? 2 * S - 2 : 2 * S - 3), "branches");
}

int main() {
  long plans = 0;
  for (int S : {3, 4, 9, 16, 69})
    for (int kind = 0; kind < 2; ++kind)
      for (int rooted = 0; rooted < 2; ++rooted)
        for (int P : {1, 64, 65, 129})
          for (int C : {1, 16})
            for (int max_draws : {1, 100}) {
              const std::vector<int32_t> peel = make_peel(S, kind, rooted != 0);
              const std::vector<uint8_t> tips = make_tips(S, P);
              const std::vector<double> w(P, 1.0);
              SeqsumPlan sp;
              expect(seqsum_plan(S, P, C, rooted, PHY_GTR, tips.data(), w.data(), peel.data(), max_draws, sp) == PHY_OK,
                     "seqsum_plan");
              ++plans;
              check_schedule(sp, S, peel, rooted != 0);
              const long long row = 1 + (4LL * (S - 1) + C + 1) * P;
              expect(sp.row_len == row && sp.off_cat == 1 + 4LL * (S - 1) * P && sp.off_rate == sp.off_cat + (long long)C * P,
                     "row layout");
              expect(sp.nblk == (P + 63) / 64 && sp.nblk * 64 <= sp.pb.Ppad && sp.pb.Ppad % 128 == 0, "column blocks");
              expect(sp.node_stride == 4LL * C * sp.pb.Ppad && sp.ws_draw == 2LL * (S - 1) * sp.node_stride, "workspace");
              expect(sp.draws_per_launch >= 1 && sp.draws_per_launch <= max_draws, "draws per launch in range");
              expect(sp.draws_per_launch == max_draws || (long long)(sp.draws_per_launch + 1) * sp.draw_bytes >
                                                            (long long)SEQ_BUDGET_BYTES,
                     "draws per launch fill the budget");
              expect(sp.lds == (size_t)C * 64 * 8 * 9 && sp.lds <= LDS_CAP, "LDS");
              // the last workspace element a launch touches is inside the allocation
              const long long last = (long long)(sp.draws_per_launch - 1) * sp.ws_draw + (long long)(S - 1) * sp.node_stride +
                                     (long long)(S - 2) * sp.node_stride + ((long long)(C - 1) * 4 + 3) * sp.pb.Ppad +
                                     (long long)sp.nblk * 64 - 1;
              expect(last < (long long)sp.draws_per_launch * sp.ws_draw, "workspace bounds");
            }
  // the synthetic shape: sizes past 2^31 bytes, one draw per launch
  {
    const int S = 128, P = 528111, C = 4;
    const std::vector<int32_t> peel = make_peel(S, 1, true);
    const std::vector<uint8_t> tips = make_tips(S, P);
    const std::vector<double> w(P, 1.0);
    SeqsumPlan sp;
    expect(seqsum_plan(S, P, C, 1, PHY_HKY, tips.data(), w.data(), peel.data(), 100, sp) == PHY_OK, "synthetic");
    ++plans;
    const long long Ppad = 528128;
    expect(sp.pb.Ppad == Ppad, "synthetic Ppad");
    expect(sp.ws_draw * 8 == 2LL * 127 * 4 * 4 * Ppad * 8 && sp.ws_draw * 8 == 17170497536LL, "synthetic workspace bytes");
    expect(sp.ws_draw * 8 > (1LL << 32), "synthetic workspace needs 64 bits");
    expect(sp.row_len == 1 + (4LL * 127 + 5) * P && sp.row_len == 270920944LL, "synthetic row");
    expect(sp.draws_per_launch == 1, "synthetic: one draw per launch");
    expect(sp.nblk == 8252, "synthetic blocks");
  }
  // refusals
  {
    const int S = 8, P = 20, C = 2;
    const std::vector<uint8_t> tips = make_tips(S, P);
    const std::vector<double> w(P, 1.0);
    const std::vector<int32_t> peel = make_peel(S, 1, false);
    SeqsumPlan sp;
    auto plan = [&](int s, int p, int c, int kind, const uint8_t* tp, const double* wp, const int32_t* pl, int md) {
      return seqsum_plan(s, p, c, 0, kind, tp, wp, pl, md, sp);
    };
    expect(refused_naming(plan(2, P, C, PHY_JC69, tips.data(), w.data(), peel.data(), 8), "S >= 3"), "S");
    expect(refused_naming(plan(S, 0, C, PHY_JC69, tips.data(), w.data(), peel.data(), 8), "P >= 1"), "P");
    expect(refused_naming(plan(S, P, 17, PHY_JC69, tips.data(), w.data(), peel.data(), 8), "C must"), "C");
    expect(refused_naming(plan(S, P, C, 7, tips.data(), w.data(), peel.data(), 8), "unknown model"), "model");
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), peel.data(), 0), "max_draws"), "max_draws");
    expect(refused_naming(plan(S, P, C, PHY_JC69, nullptr, w.data(), peel.data(), 8), "NULL"), "NULL tips");
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), nullptr, 8), "NULL"), "NULL peel");
    std::vector<uint8_t> badtips = tips;
    badtips[5] = 16;
    expect(refused_naming(plan(S, P, C, PHY_JC69, badtips.data(), w.data(), peel.data(), 8), "tip code"), "tip code");
    std::vector<int32_t> bad = peel;
    bad[1] = 99;  // a child out of range
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), bad.data(), 8), "peel row 0"), "range");
    bad = peel;
    bad[3] = bad[0];  // a node used as a child twice
    expect(plan(S, P, C, PHY_JC69, tips.data(), w.data(), bad.data(), 8) == PHY_EINVAL, "child twice");
    bad = peel;
    std::swap(bad[bad.size() - 3], bad[bad.size() - 2]);  // the last row's children swapped
    expect(refused_naming(plan(S, P, C, PHY_JC69, tips.data(), w.data(), bad.data(), 8), "unrooted peel"), "last-row rule");
    expect(plan(S, P, C, PHY_JC69, tips.data(), w.data(), peel.data(), 8) == PHY_OK, "the unspoilt tree");
    ++plans;
  }
  std::printf("seqsum_plan_check: %ld plans, %d failures\n", plans, g_bad);
  return g_bad ? 1 : 0;
}
