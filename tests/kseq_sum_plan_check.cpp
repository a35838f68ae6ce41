// kseq_sum_plan_check.cpp -- the plan of the K-state engine's posterior summaries (csrc/kseq_sum_plan.h) on the
// host alone: built by g++ with the address and undefined-behaviour sanitizers (tests/test_kseq_sum_cpu.py), no
// HIP include path.
//
// For every shape it plans, it walks every index the kernels of kseq_sum.inc and the summaries' form of the way
// down form -- the (draw, component, label) tables and the blab kernel's LDS, the labels by rate index, the
// items' count slots by (label, branch), the posterior shares in the CC blocks of every internal node, the
// counts kernel's reads and rows, the fold kernel's decomposition of a node_post entry and its reads of the
// items' workspace -- over every chunk of a full call, and checks that offset plus length lies inside the buffer
// the plan sizes.  It provokes the label refusals and the size refusal.  Prints "<n> failures" last.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "kseq_sum_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                               \
  do {                                                 \
    if (!(cond)) {                                     \
      ++failures;                                      \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                        \
      std::printf("\n");                               \
    }                                                  \
  } while (0)

struct Data {
  int S, P, K, M, C, rooted;
  std::vector<uint64_t> masks;
  std::vector<double> w;
  std::vector<int32_t> peel;
};

// caterpillar or a queue-joined (balanced) tree; the last row is (child1, 2S-3, 2S-2), valid rooted and unrooted
static Data make(int S, int P, int K, int M, int C, int rooted, bool caterpillar, unsigned seed) {
  Data d{S, P, K, M, C, rooted, {}, {}, {}};
  std::mt19937_64 rng(seed);
  const uint64_t full = K == 64 ? ~(uint64_t)0 : (((uint64_t)1 << K) - 1);
  d.masks.resize((size_t)S * P);
  for (auto& m : d.masks) m = rng() % 10 == 0 ? full : (uint64_t)1 << (rng() % K);
  d.w.assign(P, 1.0);
  std::vector<int> live;
  for (int t = 0; t < S; ++t) live.push_back(t);
  int next = S;
  while (live.size() > 1) {
    int a = live[0], b = live[1];
    live.erase(live.begin(), live.begin() + 2);
    if (caterpillar)
      live.insert(live.begin(), next);
    else
      live.push_back(next);
    if (live.size() == 1 && a == 2 * S - 3) std::swap(a, b);
    d.peel.push_back(a), d.peel.push_back(b), d.peel.push_back(next);
    ++next;
  }
  return d;
}

// geo_phases.inc's geo_rate_index: the strict lower triangle column by column
static int rate_index(int K, int i, int j) {
  const int row = i > j ? i : j, col = i > j ? j : i;
  return col * (K - 1) - col * (col - 1) / 2 + (row - col - 1);
}

static void walk(const char* name, const KseqPlan& pl, const KseqSumPlan& sp) {
  const int S = pl.S, K = pl.K, KT = pl.KT, M = pl.M, C = pl.C, G = pl.G, B = pl.B, P = pl.P, nt = pl.ntiles, N = pl.N;
  const int NL = sp.NL, R = pl.R, n = pl.max_draws;
  CHECK(NL >= 1 && NL <= KSEQ_SUM_LMAX, "%s: NL", name);
  CHECK(sp.blab_workgroups >= 1 && sp.fold_workgroups >= 1 && sp.count_workgroups >= 1, "%s: grids", name);
  CHECK(sp.blab_threads == pl.draw_threads && sp.blab_threads <= 512, "%s: blab threads", name);
  CHECK(sp.lds_blab <= KSEQ_LDS_CAP && pl.lds_down <= KSEQ_LDS_CAP, "%s: LDS", name);
  // ---- the blab kernel: its (draw, component, label) decomposition, the table it writes, its LDS, the labels
  size_t top_blab = 0;
  for (int it0 = 0; it0 < n * M * NL; ++it0) {
    const int dm = it0 / NL, lab = it0 - dm * NL, draw = dm / M, m = dm - draw * M;
    CHECK(draw < n && m < M && lab < NL, "%s: blab item %d", name, it0);
    top_blab = std::max(top_blab, kseq_sum_blab_at(draw, m, lab, M, NL, KT) + (size_t)(KT - 1) * KT + (KT - 1) + 1);
    CHECK(kseq_rec_at(draw, m, M, K) + kseq_rec_isq(K) + K <= pl.n_rec, "%s: record of blab item %d", name, it0);
  }
  CHECK(top_blab <= sp.n_blab, "%s: blab %zu/%zu", name, top_blab, sp.n_blab);
  const int KP = kseq_sum_blab_kp(K);
  CHECK((2 * (size_t)K * KP + (size_t)(K - 1) * KP + (K - 1) + 1) * sizeof(double) <= sp.lds_blab, "%s: blab LDS", name);
  int top_rate = 0;
  for (int i = 0; i < K; ++i)
    for (int j = 0; j < K; ++j)
      if (i != j) top_rate = std::max(top_rate, rate_index(K, i, j));
  CHECK(top_rate == R - 1 && (size_t)(NL - 1) * R + top_rate < sp.n_labels, "%s: label index", name);
  CHECK(kseq_mix_par_comp(K, M - 1) + top_rate < kseq_mix_par_rs(K, M), "%s: rate index", name);
  // ---- per chunk: the summaries' way down, the counts kernel and the fold kernel
  const size_t blk = kseq_blk(KT), cc = kseq_ws_cc(N, KT);
  size_t top_slot = 0, top_ws = 0, top_read = 0, top_np = 0, top_bc = 0, top_tab = 0;
  for (int d0 = 0; d0 < n; d0 += pl.chunk_draws) {
    const int nd = std::min(pl.chunk_draws, n - d0);
    if (d0 > 0 && nd == pl.chunk_draws && d0 + nd < n) continue;  // a middle chunk is the first again
    const int per_draw = G * nt;
    for (long long item = 0; item < (long long)nd * per_draw; ++item) {
      const int dl = (int)(item / per_draw), rem = (int)(item - (long long)dl * per_draw), g = rem / nt,
                tile = rem - g * nt;
      const size_t at = kseq_item(dl, g, tile, G, nt);
      // the tables of the item's (draw, component): lane entries (k, l) of every label
      top_tab = std::max(top_tab, kseq_sum_blab_at(d0 + dl, g / C, 0, M, NL, KT) + (size_t)(NL - 1) * KT * KT +
                                      (size_t)(KT - 1) * KT + (KT - 1) + 1);
      for (int lab = 0; lab < NL; ++lab)
        for (int ch : {0, B - 1}) {
          CHECK(kseq_sum_slot_at(lab, ch, B) < sp.slot_doubles, "%s: slot entry", name);
          top_slot = std::max(top_slot, at * sp.slot_doubles + kseq_sum_slot_at(lab, ch, B) + 1);
        }
      // the shares: the CC block of every internal node, the root's and the merged child's included
      for (int node : {S, 2 * S - 3, 2 * S - 2}) {
        const size_t e = cc + (size_t)node * blk + (size_t)(KT - 1) * KSEQ_PT + (KSEQ_PT - 1);
        CHECK(e < kseq_ws_sf(N, KT) && e < pl.ws_doubles, "%s: share of node %d", name, node);
        top_ws = std::max(top_ws, at * pl.ws_doubles + e + 1);
      }
      // 1 / L_i again: the chunk's [G][PP] arrays and the tile's weights
      CHECK(kseq_lc_at(dl, G - 1, G, pl.PP) + (size_t)tile * KSEQ_PT + KSEQ_PT <= pl.n_lc, "%s: lc", name);
      CHECK((size_t)tile * KSEQ_PT + KSEQ_PT <= pl.tile_w.size(), "%s: tile_w", name);
    }
    for (int dl : {0, nd - 1}) {  // the counts kernel
      const size_t first = kseq_item(dl, 0, 0, G, nt) * sp.slot_doubles;
      top_read = std::max(top_read, first + (size_t)(G * nt - 1) * sp.slot_doubles + (size_t)NL * B);
      top_bc = std::max(top_bc, (size_t)(d0 + dl) * sp.bc_row + (size_t)NL * B);
      CHECK((size_t)(d0 + dl) < sp.n_loglik, "%s: loglik", name);
    }
    // the fold kernel: every entry of a row (these shapes are small)
    const size_t KPn = (size_t)K * P;
    for (size_t e = 0; e < sp.np_row; ++e) {
      const int v = (int)(e / KPn), j = (int)((e - v * KPn) / P), i = (int)(e - v * KPn - (size_t)j * P);
      CHECK(v < S - 1 && j < K && i < P && ((size_t)v * K + j) * P + i == e, "%s: fold entry %zu", name, e);
      const int tile = i / KSEQ_PT, col = i - tile * KSEQ_PT;
      const size_t in = cc + (size_t)(S + v) * blk + (size_t)j * KSEQ_PT + col;
      CHECK(tile < nt && in < kseq_ws_sf(N, KT), "%s: fold read %zu", name, e);
      top_ws = std::max(top_ws, kseq_item(nd - 1, G - 1, tile, G, nt) * pl.ws_doubles + in + 1);
      top_np = std::max(top_np, (size_t)(nd - 1) * sp.np_row + e + 1);
    }
  }
  CHECK(top_slot <= sp.n_sslots && top_read <= sp.n_sslots, "%s: slots %zu %zu/%zu", name, top_slot, top_read,
        sp.n_sslots);
  CHECK(top_ws <= pl.n_ws, "%s: workspace %zu/%zu", name, top_ws, pl.n_ws);
  CHECK(top_np <= sp.n_npost && sp.np_row == sp.n_npsum, "%s: node_post %zu/%zu", name, top_np, sp.n_npost);
  CHECK(top_bc <= sp.n_bcounts, "%s: bcounts %zu/%zu", name, top_bc, sp.n_bcounts);
  CHECK(top_tab <= sp.n_blab, "%s: tables read %zu/%zu", name, top_tab, sp.n_blab);
}

static void planned(const char* name, const Data& d, int NL, int max_draws, int cu = 256) {
  KseqPlan pl;
  KseqSumPlan sp;
  std::vector<double> labels((size_t)NL * kseq_rate_count(d.K), 0.5);
  int rc = kseq_mix_plan(d.S, d.P, d.K, d.M, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), max_draws, cu,
                         pl, "phy_kseq_sum_create: ");
  if (!rc) rc = kseq_sum_plan(pl, NL, labels.data(), cu, sp);
  CHECK(rc == PHY_OK, "%s: refused: %s", name, g_err.c_str());
  if (!rc) walk(name, pl, sp);
}

static void refused(const char* what, int rc, const char* needle) {
  CHECK(rc == PHY_EINVAL, "%s: not refused (rc %d)", what, rc);
  CHECK(g_err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", what, g_err.c_str(), needle);
}

int main() {
  // the shapes of kseq_sum_truth: S, K, P, M, C, rooted, caterpillar, NL
  const int shapes[10][8] = {{3, 2, 1, 1, 1, 0, 0, 1},  {7, 5, 15, 1, 4, 1, 0, 2},  {7, 5, 17, 3, 1, 0, 1, 4},
                             {7, 17, 17, 2, 4, 0, 0, 2}, {7, 17, 1, 3, 1, 1, 1, 1},  {3, 33, 15, 1, 1, 1, 0, 4},
                             {7, 61, 17, 3, 1, 1, 0, 2}, {3, 64, 17, 1, 4, 0, 0, 1}, {7, 61, 17, 1, 1, 0, 0, 2},
                             {40, 20, 3, 1, 2, 0, 1, 2}};
  for (int i = 0; i < 10; ++i) {
    const int* s = shapes[i];
    char name[64];
    std::snprintf(name, sizeof name, "shape%d", i);
    const Data d = make(s[0], s[2], s[1], s[3], s[4], s[5], s[6] != 0, 100 + i);
    for (int md : {1, 2, 5, 8}) planned(name, d, s[7], md);
    planned(name, d, s[7], 3, 1);
  }
  for (int P : {1, 15, 16, 17})
    for (int NL : {1, 2, 4}) {
      char name[32];
      std::snprintf(name, sizeof name, "P%d_L%d", P, NL);
      planned(name, make(5, P, 61, 2, 2, 0, false, 50 + P), NL, 3);
    }
  planned("chunks400", make(400, 1, 17, 2, 1, 0, true, 20), 2, 70);
  {  // fluA codon: the per-draw tables and the posterior rows
    const Data flu = make(69, 40, 61, 3, 1, 1, false, 7);
    planned("fluA_codon_narrow", flu, 2, 32);
  }
  // ---- refusals
  const Data d = make(7, 17, 20, 2, 2, 0, false, 3);
  KseqPlan pl;
  KseqSumPlan sp;
  CHECK(kseq_mix_plan(d.S, d.P, d.K, d.M, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), 4, 256, pl) == PHY_OK,
        "base plan");
  std::vector<double> lab((size_t)4 * pl.R, 1.0);
  refused("n_labels low", kseq_sum_plan(pl, 0, lab.data(), 256, sp), "phy_kseq_sum_create: n_labels = 0, supported 1..4");
  refused("n_labels high", kseq_sum_plan(pl, 5, lab.data(), 256, sp), "n_labels = 5");
  refused("labels NULL", kseq_sum_plan(pl, 2, nullptr, 256, sp), "labels is NULL");
  lab[(size_t)pl.R + 3] = -1.0;
  refused("label negative", kseq_sum_plan(pl, 2, lab.data(), 256, sp), "labels[1][3] is negative or not finite");
  lab[(size_t)pl.R + 3] = std::nan("");
  refused("label nan", kseq_sum_plan(pl, 2, lab.data(), 256, sp), "labels[1][3]");
  lab[(size_t)pl.R + 3] = 0.0;  // a zero label is fine
  CHECK(kseq_sum_plan(pl, 2, lab.data(), 256, sp) == PHY_OK, "zero label refused");
  {  // a node_post row past 2^31 - 1 doubles (no shape the workspace budget admits reaches it: the fields alone)
    KseqPlan big = pl;
    big.S = 1000, big.P = 110000;  // K = 20, the labels' width: 999 * 20 * 110000 > 2^31
    refused("row size", kseq_sum_plan(big, 1, lab.data(), 256, sp), "exceeds 2^31 - 1");
    big.P = 107000;  // 999 * 20 * 107000 < 2^31
    CHECK(kseq_sum_plan(big, 1, lab.data(), 256, sp) == PHY_OK && sp.np_row == (size_t)999 * 20 * 107000, "row size ok");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
