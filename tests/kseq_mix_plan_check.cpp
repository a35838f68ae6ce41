// kseq_mix_plan_check.cpp -- the mixture plan of the K-state sequence engine (csrc/kseq_plan.h: kseq_mix_plan) on
// the host alone: built by g++ with the address and undefined-behaviour sanitizers
// (tests/test_kseq_mix_plan_cpu.py), no HIP include path.
//
// For every shape it plans, it walks every index the kernels of kseq_engine.inc form with the component index --
// the (draw, component) records, the (draw, g, tile) items with g = m C + c over G = M C, the component's run of
// slots the combine phase reads, the [G][PP] arrays, class_post, the params' and the row's blocks -- over every
// chunk of a full call, and checks that offset plus length lies inside the buffer the plan sizes.  It checks the
// mixture plan at M = 1 against kseq_plan's numbers, and provokes the mixture's refusals.
// Prints "<n> failures" last; the line "fluA_codon_mix ..." carries the plan's numbers for the Python test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "kseq_plan.h"

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
  for (auto& m : d.masks) {
    const unsigned u = (unsigned)(rng() % 10);
    m = u == 0 ? full : ((uint64_t)1 << (rng() % K)) | (u == 1 ? (uint64_t)1 << (rng() % K) : 0);
  }
  d.w.resize(P);
  for (auto& x : d.w) x = (double)(1 + rng() % 4);
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

static int plan(const Data& d, int max_draws, int cu, KseqPlan& pl) {
  return kseq_mix_plan(d.S, d.P, d.K, d.M, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), max_draws, cu,
                       pl);
}

// every index the component index adds or changes, against the sizes of the plan
static void walk(const char* name, const KseqPlan& pl) {
  const int K = pl.K, M = pl.M, C = pl.C, G = pl.G, B = pl.B, P = pl.P, PP = pl.PP, nt = pl.ntiles, R = pl.R;
  CHECK(M >= 1 && M <= KSEQ_MMAX && G == M * C && G <= KSEQ_CMAX, "%s: M, G", name);
  CHECK(pl.items_per_draw == G * nt, "%s: items per draw", name);
  CHECK(pl.chunk_draws >= 1 && pl.chunk_draws <= pl.max_draws, "%s: chunk", name);
  CHECK(pl.workgroups >= 1 && pl.draw_workgroups >= 1 && pl.comp_workgroups >= pl.draw_workgroups, "%s: grids", name);
  CHECK(pl.n_ws * sizeof(double) <= KSEQ_WS_BUDGET, "%s: workspace over the budget", name);
  CHECK(pl.rec_doubles == kseq_rec_doubles(K), "%s: record", name);
  // params: M blocks of rates and freqs, then rs and ps over G
  CHECK(pl.param_len == kseq_mix_param_len(K, M, C), "%s: param_len", name);
  for (int m = 0; m < M; ++m) {
    const int at = kseq_mix_par_comp(K, m);
    CHECK(at == m * (R + K) && at + kseq_par_freqs(K) + K <= kseq_mix_par_rs(K, M), "%s: params of component %d", name, m);
  }
  CHECK(kseq_mix_par_rs(K, M) + G == kseq_mix_par_ps(K, M, C) && kseq_mix_par_ps(K, M, C) + G == pl.param_len,
        "%s: rs and ps", name);
  // the row
  CHECK(pl.row_len == kseq_mix_row_len(B, K, M, C), "%s: row_len", name);
  CHECK(kseq_row_blens() + B == kseq_row_rs(B) && kseq_row_rs(B) + G == kseq_row_ps(B, G) &&
            kseq_row_ps(B, G) + G == kseq_mix_row_rates(B, K, M, C, 0),
        "%s: row head", name);
  for (int m = 0; m < M; ++m)
    CHECK(kseq_mix_row_rates(B, K, M, C, m) + R == kseq_mix_row_freqs(B, K, M, C, m) &&
              kseq_mix_row_freqs(B, K, M, C, m) + K ==
                  (m + 1 < M ? kseq_mix_row_rates(B, K, M, C, m + 1) : pl.row_len),
          "%s: row blocks of component %d", name, m);
  // per-draw buffers over a full call
  const int n = pl.max_draws;
  CHECK((size_t)n * pl.param_len <= pl.n_params && (size_t)n * B <= pl.n_blens &&
            (size_t)n * pl.row_len <= pl.n_rows_out && (size_t)n * P <= pl.n_site,
        "%s: per-draw buffers", name);
  size_t top_rec = 0, top_cp = 0;
  for (int draw : {0, n - 1})
    for (int m = 0; m < M; ++m) {
      top_rec = std::max(top_rec, kseq_rec_at(draw, m, M, K) + pl.rec_doubles);
      top_cp = std::max(top_cp, kseq_cpost_at(draw, m, M, P) + (size_t)P);
    }
  CHECK(top_rec <= pl.n_rec && top_cp <= pl.n_cpost, "%s: records %zu/%zu class_post %zu/%zu", name, top_rec, pl.n_rec,
        top_cp, pl.n_cpost);
  // the eigen kernel's and the combine kernel's (draw, component) index
  for (int dm = 0; dm < n * M; ++dm) {
    const int draw = dm / M, m = dm - draw * M;
    if (!(draw >= 0 && draw < n && m >= 0 && m < M)) CHECK(false, "%s: (draw, component) of %d", name, dm);
  }
  // per-chunk buffers over every chunk
  size_t top_ws = 0, top_slot = 0, top_lc = 0, top_d0 = 0;
  for (int d0 = 0; d0 < n; d0 += pl.chunk_draws) {
    const int nd = std::min(pl.chunk_draws, n - d0);
    if (d0 > 0 && nd == pl.chunk_draws && d0 + nd < n) continue;  // a middle chunk is the first again
    const long long items = (long long)nd * pl.items_per_draw;
    CHECK(items >= 1 && items < (1LL << 31), "%s: items of a chunk", name);
    const int per_draw = G * nt;
    for (long long item = 0; item < items; ++item) {  // the item kernels' decomposition
      const int dl = (int)(item / per_draw), rem = (int)(item - (long long)dl * per_draw), g = rem / nt,
                tile = rem - g * nt, m = g / C;
      CHECK(dl < nd && g < G && tile < nt && m < M, "%s: item %lld", name, item);
      const size_t at = kseq_item(dl, g, tile, G, nt);
      CHECK(at == (size_t)item, "%s: item index", name);
      top_ws = std::max(top_ws, at * pl.ws_doubles + pl.ws_doubles);
      top_slot = std::max(top_slot, at * pl.slot_doubles + pl.slot_doubles);
      top_lc = std::max(top_lc, kseq_lc_at(dl, g, G, PP) + (size_t)tile * KSEQ_PT + KSEQ_PT);
      top_d0 = std::max(top_d0, kseq_down0_at(dl, PP) + (size_t)tile * KSEQ_PT + KSEQ_PT);
    }
    for (int dl : {0, nd - 1})
      for (int m = 0; m < M; ++m) {  // the combine phase: component m's C * nt slots after the draw's first
        const size_t first = kseq_item(dl, 0, 0, G, nt) + (size_t)m * C * nt;
        CHECK(first == kseq_item(dl, m * C, 0, G, nt), "%s: slots of component %d", name, m);
        top_slot = std::max(top_slot, (first + (size_t)C * nt) * pl.slot_doubles);
      }
  }
  CHECK(top_ws <= pl.n_ws && top_slot <= pl.n_slots && top_lc <= pl.n_lc && top_lc <= pl.n_sh && top_d0 <= pl.n_down0,
        "%s: chunk buffers %zu/%zu %zu/%zu %zu/%zu %zu/%zu", name, top_ws, pl.n_ws, top_slot, pl.n_slots, top_lc,
        pl.n_lc, top_d0, pl.n_down0);
}

static void planned(const char* name, const Data& d, int max_draws, int cu = 256) {
  KseqPlan pl;
  const int rc = plan(d, max_draws, cu, pl);
  CHECK(rc == PHY_OK, "%s: refused: %s", name, g_err.c_str());
  if (rc) return;
  walk(name, pl);
  for (auto& x : pl.tile_masks) x ^= 1;  // write through every host array, end to end
  for (auto& x : pl.tile_w) x += 1.0;
  for (auto& x : pl.rows) x += 1;
}

// the mixture plan at M = 1 is kseq_plan's, number for number
static void same_as_plain(const char* name, const Data& d, int max_draws) {
  KseqPlan a, b;
  const int ra = kseq_plan(d.S, d.P, d.K, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), max_draws, 256, a);
  const int rb = kseq_mix_plan(d.S, d.P, d.K, 1, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), max_draws,
                               256, b);
  CHECK(ra == PHY_OK && rb == PHY_OK, "%s: M = 1 refused", name);
  CHECK(a.param_len == kseq_param_len(d.K, d.C) && a.row_len == kseq_row_len(a.B, d.K, d.C), "%s: plain lengths", name);
  CHECK(a.param_len == b.param_len && a.row_len == b.row_len && a.items_per_draw == b.items_per_draw &&
            a.chunk_draws == b.chunk_draws && a.workgroups == b.workgroups && a.draw_workgroups == b.draw_workgroups &&
            a.comp_workgroups == b.comp_workgroups && a.comp_workgroups == a.draw_workgroups && a.threads == b.threads &&
            a.lds_up == b.lds_up && a.lds_down == b.lds_down && a.lds_draw == b.lds_draw && a.n_ws == b.n_ws &&
            a.n_slots == b.n_slots && a.n_lc == b.n_lc && a.n_sh == b.n_sh && a.n_down0 == b.n_down0 &&
            a.n_rec == b.n_rec && a.n_params == b.n_params && a.n_rows_out == b.n_rows_out && a.n_site == b.n_site &&
            a.n_cpost == b.n_cpost && a.M == 1 && b.M == 1 && a.G == d.C && a.tile_masks == b.tile_masks &&
            a.tile_w == b.tile_w && a.rows == b.rows,
        "%s: M = 1 differs from kseq_plan", name);
  CHECK(kseq_mix_par_rs(d.K, 1) == kseq_par_rs(d.K) && kseq_mix_par_ps(d.K, 1, d.C) == kseq_par_ps(d.K, d.C) &&
            kseq_mix_row_rates(a.B, d.K, 1, d.C, 0) == kseq_row_rates(a.B, d.C) &&
            kseq_mix_row_freqs(a.B, d.K, 1, d.C, 0) == kseq_row_freqs(a.B, d.K, d.C) &&
            kseq_rec_at(3, 0, 1, d.K) == 3 * kseq_rec_doubles(d.K),
        "%s: M = 1 offsets", name);
}

static void refused(const char* what, int rc, const char* needle) {
  CHECK(rc == PHY_EINVAL, "%s: not refused (rc %d)", what, rc);
  CHECK(g_err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", what, g_err.c_str(), needle);
}

int main() {
  // the shapes of kseq_mix_truth.small_cases() and its caterpillar: S, K, P, M, C, rooted, caterpillar
  const int shapes[8][7] = {{3, 2, 1, 1, 1, 0, 0},  {7, 5, 15, 2, 2, 1, 0},  {7, 17, 17, 3, 1, 0, 0}, {3, 5, 17, 3, 2, 1, 0},
                            {7, 17, 1, 2, 1, 1, 1}, {3, 61, 17, 2, 2, 0, 0}, {7, 61, 15, 3, 1, 1, 0}, {24, 5, 3, 2, 1, 0, 1}};
  for (int i = 0; i < 8; ++i) {
    const int* s = shapes[i];
    char name[64];
    std::snprintf(name, sizeof name, "small%d", i);
    const Data d = make(s[0], s[2], s[1], s[3], s[4], s[5], s[6] != 0, 100 + i);
    for (int md : {1, 2, 5, 8}) planned(name, d, md);
    planned(name, d, 3, 1);
  }
  // kseq_mix_truth.edge_cases() (M = 8, G = 16; 1024 draws as the per-draw loop test plans it), the item-loop test's
  // twin, and KT = 48 under a mixture: S, K, P, M, C, rooted
  const int edges[5][6] = {{3, 5, 17, 8, 2, 1}, {3, 4, 145, 2, 2, 1}, {7, 40, 33, 2, 2, 0}, {3, 48, 65, 8, 2, 1},
                           {7, 33, 17, 1, 16, 0}};
  for (int i = 0; i < 5; ++i) {
    const int* s = edges[i];
    char name[64];
    std::snprintf(name, sizeof name, "edge%d", i);
    const Data d = make(s[0], s[2], s[1], s[3], s[4], s[5], false, 200 + i);
    for (int md : {1, 8, 64, 1024}) planned(name, d, md);
    planned(name, d, 3, 1);
    KseqPlan pl;
    CHECK(plan(d, 8, 256, pl) == PHY_OK, "%s", name);
    CHECK(pl.threads == 4 * pl.KT && pl.G == s[3] * s[4], "%s: KT %d threads %d G %d", name, pl.KT, pl.threads, pl.G);
  }
  planned("chunks400", make(400, 1, 17, 2, 1, 0, true, 20), 70);
  const Data flu = make(69, 242, 61, 3, 4, 1, false, 7);
  for (int md : {1, 32}) planned("fluA_codon_mix", flu, md);
  {
    KseqPlan pl;
    CHECK(plan(flu, 32, 256, pl) == PHY_OK, "fluA_codon_mix");
    CHECK(pl.items_per_draw == 192 && pl.chunk_draws == 1, "fluA_codon_mix: 192 items, one draw in flight");
    std::printf("fluA_codon_mix KT=%d tiles=%d items_per_draw=%d chunk_draws=%d threads=%d workgroups=%d "
                "draw_workgroups=%d lds_up=%zu lds_down=%zu lds_draw=%zu ws_doubles=%zu slot_doubles=%zu "
                "rec_doubles=%zu row_len=%d B=%d workspace_bytes=%zu\n",
                pl.KT, pl.ntiles, pl.items_per_draw, pl.chunk_draws, pl.threads, pl.workgroups, pl.draw_workgroups,
                pl.lds_up, pl.lds_down, pl.lds_draw, pl.ws_doubles, pl.slot_doubles, pl.rec_doubles, pl.row_len, pl.B,
                pl.n_ws * sizeof(double));
  }
  for (int P : {1, 15, 16, 17}) {
    char name[32];
    std::snprintf(name, sizeof name, "P%d", P);
    planned(name, make(5, P, 61, 2, 2, 0, false, 50 + P), 3);
  }
  for (int M : {1, 2, 4, 8}) {  // M * C = 16
    char name[32];
    std::snprintf(name, sizeof name, "G16_M%d", M);
    planned(name, make(5, 17, 20, M, 16 / M, 1, false, 60 + M), 3);
  }
  for (int i = 0; i < 3; ++i) {
    const int s[3][4] = {{7, 17, 17, 4}, {69, 242, 61, 4}, {3, 1, 2, 1}};
    const Data d = make(s[i][0], s[i][1], s[i][2], 1, s[i][3], i & 1, false, 70 + i);
    for (int md : {1, 32}) same_as_plain("M1", d, md);
  }
  // ---- the mixture's refusals; everything kseq_plan refuses comes through the same function
  const Data d = make(7, 17, 20, 2, 4, 0, false, 3);
  KseqPlan pl;
  auto call = [&](int S, int K, int M, int C, const uint64_t* m, int md) {
    return kseq_mix_plan(S, 17, K, M, C, 0, m, d.w.data(), d.peel.data(), md, 256, pl);
  };
  const uint64_t* MK = d.masks.data();
  refused("M low", call(7, 20, 0, 4, MK, 1), "phy_kseq_mix_create: M = 0 components, supported 1..8");
  refused("M high", call(7, 20, 9, 1, MK, 1), "M = 9 components");
  refused("C low", call(7, 20, 2, 0, MK, 1), "C = 0 categories");
  refused("G high", call(7, 20, 3, 6, MK, 1), "M * C = 18 component-categories, supported up to 16");
  refused("C high", call(7, 20, 1, 17, MK, 1), "C = 17 categories");
  refused("K", call(7, 65, 2, 4, MK, 1), "K = 65");
  refused("S", call(2, 20, 2, 4, MK, 1), "S = 2");
  refused("max_draws", call(7, 20, 2, 4, MK, 0), "max_draws");
  refused("tipmasks", call(7, 20, 2, 4, nullptr, 1), "tipmasks is NULL");
  {  // S = 2000 / P = 1300 / K = 64 / M = 4, C = 4: one draw's 1312 items of 98 MB pass the budget
    const Data big = make(2000, 1300, 64, 4, 4, 1, false, 9);
    refused("big", plan(big, 1, 256, pl), "exceeds the budget");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
