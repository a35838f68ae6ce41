// Drives the device-free planner (phylostan_amd/csrc/sweep_plan.h) over
// generated trees under a host sanitizer (tests/test_plan_host.py builds it
// with -fsanitize=address,undefined).  Every call must return PHY_OK or, where
// the header documents one, a refusal (PHY_EINVAL with a message).
#include <cstdio>

#include "sweep_plan.h"

static unsigned long long g_lcg = 12345;
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
    if (kind == 0 && nxt > S) i = live.size() - 1, j = 0;  // the last internal node and the next tip
    if (kind == 2) {
      i = rnd((unsigned)live.size());
      j = rnd((unsigned)live.size() - 1);
      if (j >= i) ++j;
    }
    int a = live[i], b = live[j];
    if (live.size() == 2 && !rooted && b != 2 * S - 3) std::swap(a, b);  // child 2 of the root: node 2S-3
    live.erase(live.begin() + std::max(i, j));
    live.erase(live.begin() + std::min(i, j));
    if (kind == 1) live.push_back(nxt); else live.insert(live.begin(), nxt);
    if (kind == 2) std::swap(live[0], live[rnd((unsigned)live.size())]);
    peel.insert(peel.end(), {a, b, nxt});
  }
  return peel;
}

static int g_bad = 0;
static void expect(bool ok, const char* what, int S, int P, int C) {
  if (ok) return;
  std::fprintf(stderr, "FAIL %s (S %d P %d C %d): %s\n", what, S, P, C, g_err.c_str());
  ++g_bad;
}
static bool refused(int rc) { return rc == PHY_EINVAL && !g_err.empty(); }

// The quad sweeps' LDS layout (QuadLds: region sizes in order; the kernels step their pointers by them).
// Each region holds what its kernel puts there (so stepping by the sizes overlaps nothing), the offsets ascend,
// every double region starts 8-byte aligned, the records (offset 0) and the nibble block 16-byte aligned, and
// the total is the one the closed forms gave before the layout existed.  A failure names the region.
static void check_layout(const char* what, const QuadLds& l, const size_t (&need)[6], size_t want, int S, int C) {
  static const char* const name[6] = {"records", "tip vectors", "root exchange", "tail", "flags", "nibbles"};
  const size_t size[6] = {l.recs * 8, l.tvec * 8, l.xch * 8, l.tail * 8, l.flags, l.nib};
  size_t off = 0;
  for (int i = 0; i < 6; ++i) {
    const size_t align = (i == 0 || i == 5) ? 16 : i < 4 ? 8 : 4;
    if (size[i] < need[i] || off % align != 0 || off + size[i] < off) {
      std::fprintf(stderr, "FAIL %s (S %d C %d): region %d (%s) at byte %zu, %zu bytes, needs %zu, alignment %zu\n", what, S,
                   C, i, name[i], off, size[i], need[i], align);
      ++g_bad;
    }
    off += size[i];
  }
  if (off != want || l.bytes() != want) {
    std::fprintf(stderr, "FAIL %s (S %d C %d): total %zu / %zu, the parent's %zu\n", what, S, C, off, l.bytes(), want);
    ++g_bad;
  }
}
static void check_quad_layouts() {
  // S, C, nmat, R, ndeep, nslot, then quad_lds_bytes(S, C, nmat, R, ndeep) and qmw_lds_bytes(S, C, nmat, R, nslot)
  // as computed at the commit before the layouts
  static const size_t rows[][8] = {
      {3, 1, 4, 5, 0, 0, 1312, 1328},
      {3, 4, 4, 9, 2, 1, 9760, 7744},
      {3, 16, 4, 5, 1, 3, 21024, 37616},
      {12, 4, 22, 9, 0, 0, 26464, 26480},
      {12, 4, 22, 9, 3, 6, 32608, 38864},
      {12, 5, 22, 5, 2, 5, 23968, 31776},
      {12, 16, 22, 9, 3, 0, 128608, 104048},
      {12, 1, 22, 5, 4, 7, 6304, 7888},
      {69, 4, 136, 5, 0, 9, 88624, 107216},
      {69, 4, 136, 5, 5, 22, 98864, 134048},
      {69, 5, 136, 9, 6, 13, 212912, 231120},
      {69, 1, 136, 9, 7, 2, 43952, 41424},
      {128, 1, 254, 5, 6, 31, 45376, 58320},
      {128, 4, 254, 5, 0, 17, 164608, 199712},
      {128, 5, 254, 5, 3, 4, 213056, 215712},
      {17, 5, 32, 9, 4, 3, 57616, 55136},
  };
  for (const auto& r : rows) {
    const int S = (int)r[0], C = (int)r[1], nmat = (int)r[2], R = (int)r[3], ndeep = (int)r[4], nslot = (int)r[5];
    const size_t recs = (size_t)C * nmat * R * 4 * 8, tv = 64 * 8, xch = (size_t)C * 16 * 8, nib = (size_t)S * 8;
    const size_t qneed[6] = {recs, tv, xch, (size_t)C * ndeep * 64 * 8, 0, nib};
    check_layout("QuadLds one wave", QuadLds(S, C, nmat, R, ndeep, false), qneed, r[6], S, C);
    const size_t mneed[6] = {recs, tv, xch, (size_t)C * nslot * 64 * 8, (size_t)C * nslot * 4 + 4, nib};  // + error word
    check_layout("QuadLds multi-wave", QuadLds(S, C, nmat, R, nslot, true), mneed, r[7], S, C);
    if (quad_lds_bytes(S, C, nmat, R, ndeep) != r[6] || qmw_lds_bytes(S, C, nmat, R, nslot) != r[7]) {
      std::fprintf(stderr, "FAIL quad_lds_bytes / qmw_lds_bytes (S %d C %d)\n", S, C);
      ++g_bad;
    }
  }
}

int main() {
  check_quad_layouts();
  long plans = 0, launches = 0;
  for (int S : {3, 4, 5, 12, 69, 200, 700})
    for (int kind = 0; kind < 3; ++kind)
      for (int rooted = 0; rooted < 2; ++rooted) {
        const std::vector<int32_t> peel = make_peel(S, kind, rooted != 0);
        std::vector<int> prog, matbr;
        int nslots = 0, ndeep = 0;
        expect(build_program(S, peel.data(), rooted, prog, matbr, nslots, ndeep) == PHY_OK, "build_program", S, 0, 0);
        for (int cap : {3, 9, 3 * S})
          for (int rec = 0; rec < 2; ++rec) {
            std::vector<int> p = prog;
            int nch = 0, nrec = 0;
            expect(assign_chunks(p, S - 1, (int)matbr.size(), cap, rec != 0, nch, nrec) == PHY_OK, "assign_chunks", S, 0, cap);
            expect(batched_records(p, 2, 4, 5).size() == p.size() && pack_program(p).size() * 2 == p.size(), "records", S, 0, cap);
          }
        for (int P : {1, 63, 64, 65, 129, 300}) {
          std::vector<uint8_t> tips((size_t)S * P);
          for (auto& t : tips) t = rnd(16) == 0 ? 15 : (uint8_t)(1 << (2 * rnd(2)));  // two letters, a few gaps
          const std::vector<double> w(P, 1.0);
          for (int C : {1, 4, 8, 16}) {
            Problem pb;
            const int max_draws = (S + P + C) % 3 == 0 ? 1 : (S + P + C) % 3 == 1 ? 100 : 8192;
            int rc = make_problem(S, P, C, rooted, PHY_HKY, tips.data(), w.data(), peel.data(), max_draws, pb);
            expect(rc == PHY_OK || refused(rc), "make_problem", S, P, C);
            if (rc) continue;
            expect(pack_tips(pb).size() == (size_t)S * pb.Ppad / 2, "pack_tips", S, P, C);
            for (int mode : {0, 1, -1}) {
              CladePlan cp;
              expect(select_clades(pb, mode, cp) == PHY_OK, "select_clades", S, P, C);
              for (int cols = 0; cols <= 2; ++cols)
                for (int deep = (cols + mode + 1) % 2; deep <= 2; deep += 2) {  // half of the (cols, deep) pairs per mode
                  Prefs prefs;
                  prefs.cols = cols;
                  prefs.deep = deep;
                  prefs.cc_mode = mode;
                  prefs.lds_budget = (cols + deep) % 2 ? 40000 : 0;
                  prefs.recompute = (mode + deep) % 2 == 0;
                  prefs.rescale = cols == 1 && deep == 1;
                  SweepPlan plan;
                  rc = plan_lds(pb, prefs, 256, plan);
                  expect(rc == PHY_OK || refused(rc), "plan_lds", S, P, C);
                  if (rc) continue;
                  ++plans;
                  std::vector<int> recs;
                  expect(plan_clade_records(pb, prefs, cp, plan, recs) == PHY_OK, "clade_records", S, P, C);
                  if (cp.ncl) {
                    expect(!clade_table(cp, S, C).empty(), "clade_table", S, P, C);
                    expect(pack_tips(pb, &cp).size() == (size_t)S * (pb.Ppad + CC_COLS) / 2, "pack_tips cc", S, P, C);
                  }
                  if (cols == 0 && deep == 0) {
                    const QuadPlan q = plan_quad(pb, plan);  // quad_program, quad_mw_plan
                    expect(!plan.quad_ok || !q.prog.empty(), "plan_quad", S, P, C);
                  }
                  for (int n : {1, 32, 33, max_draws}) {
                    if (n > max_draws) continue;
                    const LaunchChoice ch = choose_launch(pb, prefs, plan, n, n <= 32);
                    expect(ch.gx >= 1 && (long)ch.gx * n <= std::max<long>(plan.wg_need, 4L * 256), "choose_launch", S, P, n);
                    ++launches;
                  }
                }
            }
          }
        }
      }
  std::printf("plan_host_check: %ld plans, %ld launch choices, %d failures\n", plans, launches, g_bad);
  return g_bad ? 1 : 0;
}
