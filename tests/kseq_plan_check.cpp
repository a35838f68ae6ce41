// kseq_plan_check.cpp -- the K-state sequence engine's planner (csrc/kseq_plan.h) on the host alone: built by g++
// with the address and undefined-behaviour sanitizers (tests/test_kseq_plan_cpu.py), no HIP include path.
//
// For every shape it plans, it walks every index the kernels of kseq_engine.inc form -- through the same PHY_HD
// helpers -- over every chunk of a full call, a last short chunk included, and checks that offset plus length lies
// inside the buffer the plan sizes; it writes through every host array the plan builds; and it provokes each refusal.
// Prints "<n> failures" last; the line "fluA_codon ..." carries the plan's numbers for the Python test.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "kseq_plan.h"

static int failures = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      ++failures;                              \
      std::printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
    }                                          \
  } while (0)

struct Data {
  int S, P, K, C, rooted;
  std::vector<uint64_t> masks;
  std::vector<double> w;
  std::vector<int32_t> peel;
};

// caterpillar or a queue-joined (balanced) tree; the last row is (child1, 2S-3, 2S-2), valid rooted and unrooted
static Data make(int S, int P, int K, int C, int rooted, bool caterpillar, unsigned seed) {
  Data d{S, P, K, C, rooted, {}, {}, {}};
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
    int a, b;
    if (caterpillar) {
      a = live[0], b = live[1];
      live.erase(live.begin(), live.begin() + 2);
      live.insert(live.begin(), next);
    } else {
      a = live[0], b = live[1];
      live.erase(live.begin(), live.begin() + 2);
      live.push_back(next);
    }
    if (live.size() == 1 && a == 2 * S - 3) std::swap(a, b);
    d.peel.push_back(a), d.peel.push_back(b), d.peel.push_back(next);
    ++next;
  }
  return d;
}

static int plan(const Data& d, int max_draws, int cu, KseqPlan& pl) {
  return kseq_plan(d.S, d.P, d.K, d.C, d.rooted, d.masks.data(), d.w.data(), d.peel.data(), max_draws, cu, pl);
}

// every index of the kernels against the sizes of the plan
static void walk(const char* name, const KseqPlan& pl) {
  const int S = pl.S, K = pl.K, C = pl.C, KT = pl.KT, N = pl.N, B = pl.B, P = pl.P, PP = pl.PP, nt = pl.ntiles;
  CHECK(KT % 16 == 0 && KT >= K && KT - K < 16 && pl.NB == KT / 16 && pl.NB <= 4, "%s: KT", name);
  CHECK(nt == (P + 15) / 16 && PP == nt * 16 && pl.items_per_draw == C * nt, "%s: tiles", name);
  CHECK(pl.threads == 64 * pl.NB && pl.threads <= 256, "%s: threads", name);
  CHECK(pl.draw_threads <= GEO_MAX_THREADS && pl.site_threads <= GEO_MAX_THREADS, "%s: draw threads", name);
  CHECK(pl.chunk_draws >= 1 && pl.chunk_draws <= pl.max_draws, "%s: chunk", name);
  CHECK(pl.workgroups >= 1 && pl.draw_workgroups >= 1, "%s: grids", name);
  CHECK(pl.n_ws * sizeof(double) <= KSEQ_WS_BUDGET, "%s: workspace over the budget", name);
  // LDS
  const KseqLds L(KT);
  const size_t op = (size_t)KT * KSEQ_XS, mat = (size_t)(KT - 1) * L.VS + KT;
  CHECK(L.V() + mat <= (size_t)L.X(0), "%s: LDS V", name);
  for (int i = 0; i < 4; ++i) CHECK(L.X(i) + op <= (size_t)(i < 3 ? L.X(i + 1) : L.vecs(0)), "%s: LDS X%d", name, i);
  for (int i = 0; i < 6; ++i) CHECK(L.vecs(i) + KT <= (i < 5 ? L.vecs(i + 1) : L.red()), "%s: LDS vec", name);
  CHECK(L.red() + 4 * 16 <= L.col() && L.col() + 32 <= L.up_doubles(), "%s: LDS red", name);
  CHECK(L.RT() >= L.up_doubles() && L.RT() + mat <= (size_t)L.down_doubles(), "%s: LDS RT", name);
  CHECK((size_t)L.up_doubles() * 8 == pl.lds_up && (size_t)L.down_doubles() * 8 == pl.lds_down, "%s: LDS bytes", name);
  CHECK(pl.lds_up <= KSEQ_LDS_CAP && pl.lds_down <= KSEQ_LDS_CAP && pl.lds_draw <= KSEQ_LDS_CAP, "%s: LDS cap", name);
  CHECK((size_t)GeoLds(K).doubles() * 8 == pl.lds_draw, "%s: LDS of the draw kernels", name);
  CHECK(GeoLds(K).red() + GEO_MAX_THREADS <= GeoLds(K).doubles(), "%s: LDS red of the draw kernels", name);
  // the layouts: fields in order, none overlapping, the last inside the unit
  const size_t blk = kseq_blk(KT);
  CHECK(kseq_ws_low(N, KT) + N * blk <= kseq_ws_cc(N, KT) && kseq_ws_cc(N, KT) + N * blk <= kseq_ws_msg(N, KT) &&
            kseq_ws_msg(N, KT) + N * blk <= kseq_ws_sf(N, KT) &&
            kseq_ws_sf(N, KT) + (size_t)N * KSEQ_PT <= pl.ws_doubles,
        "%s: workspace fields", name);
  CHECK(kseq_slot_w(KT) + (size_t)KT * KT <= kseq_slot_dvec(KT) && kseq_slot_dvec(KT) + KT <= kseq_slot_rootpi(KT) &&
            kseq_slot_rootpi(KT) + KT <= kseq_slot_gb(KT) && kseq_slot_gb(KT) + B <= kseq_slot_grs(KT, B) &&
            kseq_slot_grs(KT, B) + 1 <= kseq_slot_gps(KT, B) && kseq_slot_gps(KT, B) + 1 <= pl.slot_doubles,
        "%s: slot fields", name);
  CHECK(KREC_LL < KREC_HEAD && kseq_rec_lam(K) + K <= kseq_rec_qd(K) && kseq_rec_qd(K) + K <= kseq_rec_v(K) &&
            kseq_rec_v(K) + (size_t)K * K <= kseq_rec_sq(K) && kseq_rec_sq(K) + K <= kseq_rec_isq(K) &&
            kseq_rec_isq(K) + K <= pl.rec_doubles,
        "%s: record fields", name);
  CHECK(kseq_row_blens() + B <= kseq_row_rs(B) && kseq_row_rs(B) + C <= kseq_row_ps(B, C) &&
            kseq_row_ps(B, C) + C <= kseq_row_rates(B, C) &&
            kseq_row_rates(B, C) + kseq_rate_count(K) <= kseq_row_freqs(B, K, C) &&
            kseq_row_freqs(B, K, C) + K == pl.row_len,
        "%s: row fields", name);
  CHECK(kseq_par_freqs(K) + K <= kseq_par_rs(K) && kseq_par_rs(K) + C <= kseq_par_ps(K, C) &&
            kseq_par_ps(K, C) + C == pl.param_len,
        "%s: param fields", name);
  // the host arrays
  CHECK(pl.tile_masks.size() == (size_t)nt * S * 16 && pl.tile_w.size() == (size_t)PP &&
            pl.rows.size() == (size_t)(S - 1) * KR_INTS,
        "%s: host arrays", name);
  for (int tile = 0; tile < nt; ++tile)
    CHECK(kseq_mask_at(tile, S - 1, S) + KSEQ_PT <= pl.tile_masks.size(), "%s: tile masks", name);
  for (int r = 0; r < S - 1; ++r) {
    const int32_t* w = &pl.rows[(size_t)r * KR_INTS];
    CHECK(w[KR_A] >= 0 && w[KR_A] < N - 1 && w[KR_B] >= 0 && w[KR_B] < N - 1 && w[KR_P] >= S && w[KR_P] < N,
          "%s: row %d nodes", name, r);
    // a child with a branch of its own indexes blens and the slot's G
    CHECK(w[KR_A] < B && (w[KR_FOLD] || w[KR_B] < B), "%s: row %d branches", name, r);
    CHECK(!w[KR_FOLD] || (r == S - 2 && w[KR_B] >= S), "%s: row %d fold", name, r);
  }
  // per-draw buffers over a full call, per-chunk buffers over every chunk
  const int n = pl.max_draws;
  CHECK((size_t)n * pl.param_len <= pl.n_params && (size_t)n * B <= pl.n_blens &&
            (size_t)(n - 1) * pl.rec_doubles + pl.rec_doubles <= pl.n_rec &&
            (size_t)n * pl.row_len <= pl.n_rows_out && (size_t)n * P <= pl.n_site,
        "%s: per-draw buffers", name);
  size_t top_ws = 0, top_slot = 0, top_lc = 0, top_d0 = 0;
  for (int d0 = 0; d0 < n; d0 += pl.chunk_draws) {
    const int nd = std::min(pl.chunk_draws, n - d0);
    if (d0 > 0 && nd == pl.chunk_draws && d0 + nd < n) continue;  // a middle chunk is the first again
    const long long items = (long long)nd * pl.items_per_draw;
    CHECK(items >= 1 && items < (1LL << 31), "%s: items of a chunk", name);
    for (int dl = 0; dl < nd; ++dl)
      for (int c = 0; c < C; ++c)
        for (int tile = 0; tile < nt; ++tile) {
          const size_t at = kseq_item(dl, c, tile, C, nt);
          CHECK(at < (size_t)items, "%s: item index", name);
          top_ws = std::max(top_ws, at * pl.ws_doubles + pl.ws_doubles);
          top_slot = std::max(top_slot, at * pl.slot_doubles + pl.slot_doubles);
          top_lc = std::max(top_lc, kseq_lc_at(dl, c, C, PP) + (size_t)tile * KSEQ_PT + KSEQ_PT);
          top_d0 = std::max(top_d0, kseq_down0_at(dl, PP) + (size_t)tile * KSEQ_PT + KSEQ_PT);
        }
  }
  CHECK(top_ws <= pl.n_ws && top_slot <= pl.n_slots && top_lc <= pl.n_lc && top_lc <= pl.n_sh && top_d0 <= pl.n_down0,
        "%s: chunk buffers %zu/%zu %zu/%zu %zu/%zu %zu/%zu", name, top_ws, pl.n_ws, top_slot, pl.n_slots, top_lc,
        pl.n_lc, top_d0, pl.n_down0);
}

// write through every host array, end to end (the sanitizer sees a short one)
static void scribble(KseqPlan& pl) {
  for (auto& x : pl.tile_masks) x ^= 1;
  for (auto& x : pl.tile_w) x += 1.0;
  for (auto& x : pl.rows) x += 1;
  std::memset(pl.tile_masks.data(), 0, pl.tile_masks.size() * sizeof(uint64_t));
  std::memset(pl.tile_w.data(), 0, pl.tile_w.size() * sizeof(double));
  std::memset(pl.rows.data(), 0, pl.rows.size() * sizeof(int32_t));
}

static void planned(const char* name, const Data& d, int max_draws, int cu = 256) {
  KseqPlan pl;
  const int rc = plan(d, max_draws, cu, pl);
  CHECK(rc == PHY_OK, "%s: refused: %s", name, g_err.c_str());
  if (rc) return;
  // the padding: all K bits and weight 0; the data: where the caller put it
  const uint64_t full = d.K == 64 ? ~(uint64_t)0 : (((uint64_t)1 << d.K) - 1);
  for (int i = 0; i < pl.PP; ++i) {
    const int tile = i / 16, col = i % 16;
    CHECK(pl.tile_w[i] == (i < d.P ? d.w[i] : 0.0), "%s: weight %d", name, i);
    for (int t = 0; t < d.S; ++t)
      CHECK(pl.tile_masks[kseq_mask_at(tile, t, d.S) + col] == (i < d.P ? d.masks[(size_t)t * d.P + i] : full),
            "%s: mask %d %d", name, t, i);
  }
  walk(name, pl);
  scribble(pl);
}

static void refused(const char* what, int rc, const char* needle) {
  CHECK(rc == PHY_EINVAL, "%s: not refused (rc %d)", what, rc);
  CHECK(g_err.find(needle) != std::string::npos, "%s: message '%s' lacks '%s'", what, g_err.c_str(), needle);
}

int main() {
  // the 12 shapes of kseq_truth.small_cases(): S, K, P, C, rooted, caterpillar
  const int shapes[12][6] = {{3, 2, 1, 1, 0, 0},   {7, 4, 15, 4, 1, 0},  {7, 5, 17, 1, 0, 1},  {3, 16, 65, 1, 1, 0},
                             {7, 17, 17, 4, 0, 0}, {7, 20, 65, 4, 0, 0}, {7, 20, 15, 1, 1, 1}, {3, 64, 17, 4, 1, 0},
                             {7, 64, 1, 1, 0, 0},  {7, 61, 17, 4, 1, 0}, {7, 61, 15, 1, 0, 0}, {3, 61, 65, 1, 1, 0}};
  for (int i = 0; i < 12; ++i) {
    const int* s = shapes[i];
    char name[64];
    std::snprintf(name, sizeof name, "small%d", i);
    const Data d = make(s[0], s[2], s[1], s[3], s[4], s[5] != 0, 100 + i);
    for (int md : {1, 2, 5}) planned(name, d, md);
    planned(name, d, 3, 1);
  }
  // the 10 shapes of kseq_truth.edge_cases(): KT = 48 (K = 33, 40, 48: a third row block, 192 threads), K = 32 and 49,
  // C = 16, the 300-tip caterpillar; then the 2560 items of the item-loop test
  const int edges[11][6] = {{7, 40, 33, 1, 1, 1}, {7, 20, 17, 4, 0, 0}, {7, 5, 17, 1, 1, 0},  {7, 61, 17, 1, 1, 0},
                            {300, 20, 3, 2, 0, 1}, {7, 32, 17, 1, 1, 0}, {7, 33, 17, 4, 0, 0}, {3, 48, 65, 4, 0, 0},
                            {3, 49, 17, 1, 1, 0}, {3, 4, 17, 16, 1, 0}, {3, 4, 145, 4, 1, 0}};
  for (int i = 0; i < 11; ++i) {
    const int* s = edges[i];
    char name[64];
    std::snprintf(name, sizeof name, "edge%d", i);
    const Data d = make(s[0], s[2], s[1], s[3], s[4], s[5] != 0, 200 + i);
    for (int md : {1, 2, 5, 64}) planned(name, d, md);
    planned(name, d, 3, 1);
    KseqPlan pl;
    CHECK(plan(d, 2, 256, pl) == PHY_OK, "%s", name);
    CHECK(pl.KT == 16 * ((s[1] + 15) / 16) && pl.threads == 4 * pl.KT, "%s: KT %d threads %d", name, pl.KT, pl.threads);
    if (s[1] > 32 && s[1] <= 48) CHECK(pl.NB == 3 && pl.threads == 192, "%s: three row blocks", name);
  }
  planned("caterpillar400", make(400, 3, 20, 1, 0, true, 20), 4);
  const Data flu = make(69, 242, 61, 4, 1, false, 7);
  for (int md : {1, 32, 1000}) planned("fluA_codon", flu, md);
  {
    KseqPlan pl;
    CHECK(plan(flu, 32, 256, pl) == PHY_OK, "fluA_codon");
    CHECK(pl.items_per_draw == 64 && pl.chunk_draws >= 1, "fluA_codon: one draw's 64 items resident");
    std::printf("fluA_codon KT=%d tiles=%d items_per_draw=%d chunk_draws=%d threads=%d workgroups=%d "
                "draw_workgroups=%d lds_up=%zu lds_down=%zu lds_draw=%zu ws_doubles=%zu slot_doubles=%zu "
                "rec_doubles=%zu row_len=%d B=%d workspace_bytes=%zu\n",
                pl.KT, pl.ntiles, pl.items_per_draw, pl.chunk_draws, pl.threads, pl.workgroups, pl.draw_workgroups,
                pl.lds_up, pl.lds_down, pl.lds_draw, pl.ws_doubles, pl.slot_doubles, pl.rec_doubles, pl.row_len, pl.B,
                pl.n_ws * sizeof(double));
  }
  for (int P : {1, 15, 16, 17}) {
    char name[32];
    std::snprintf(name, sizeof name, "P%d", P);
    planned(name, make(5, P, 61, 2, 0, false, 50 + P), 3);
  }
  {  // S = 2000 / P = 5000 / K = 64 / C = 16: one draw's 5008 items of 98 MB pass the budget: refused, not truncated
    const Data big = make(2000, 5000, 64, 16, 1, false, 9);
    KseqPlan pl;
    refused("big", plan(big, 1, 256, pl), "exceeds the budget");
    // the same tree at a size that fits runs the walk
    planned("big_fits", make(2000, 16, 64, 1, 1, false, 9), 2);
  }
  // ---- the refusals
  const Data d = make(7, 17, 20, 4, 0, false, 3);
  KseqPlan pl;
  auto call = [&](int S, int P, int K, int C, int rooted, const uint64_t* m, const double* w, const int32_t* peel,
                  int md) { return kseq_plan(S, P, K, C, rooted, m, w, peel, md, 256, pl); };
  const uint64_t* M = d.masks.data();
  const double* W = d.w.data();
  const int32_t* PE = d.peel.data();
  refused("S", call(2, 17, 20, 4, 0, M, W, PE, 1), "S = 2");
  refused("P", call(7, 0, 20, 4, 0, M, W, PE, 1), "P = 0");
  refused("K low", call(7, 17, 1, 4, 0, M, W, PE, 1), "K = 1");
  refused("K high", call(7, 17, 65, 4, 0, M, W, PE, 1), "K = 65");
  refused("C low", call(7, 17, 20, 0, 0, M, W, PE, 1), "C = 0");
  refused("C high", call(7, 17, 20, 17, 0, M, W, PE, 1), "C = 17");
  refused("max_draws", call(7, 17, 20, 4, 0, M, W, PE, 0), "max_draws");
  refused("tipmasks", call(7, 17, 20, 4, 0, nullptr, W, PE, 1), "tipmasks is NULL");
  refused("weights", call(7, 17, 20, 4, 0, M, nullptr, PE, 1), "weights is NULL");
  refused("peel", call(7, 17, 20, 4, 0, M, W, nullptr, 1), "peel is NULL");
  {
    auto m = d.masks;
    m[5] = 0;
    refused("empty mask", call(7, 17, 20, 4, 0, m.data(), W, PE, 1), "tipmasks[0][5] has no bit set");
    m[5] = (uint64_t)1 << 20;
    refused("high bit", call(7, 17, 20, 4, 0, m.data(), W, PE, 1), "tipmasks[0][5] has a bit >= K set");
    auto w = d.w;
    w[3] = -1.0;
    refused("negative weight", call(7, 17, 20, 4, 0, M, w.data(), PE, 1), "weights[3]");
    w[3] = std::nan("");
    refused("nan weight", call(7, 17, 20, 4, 0, M, w.data(), PE, 1), "weights[3]");
    w[3] = INFINITY;
    refused("inf weight", call(7, 17, 20, 4, 0, M, w.data(), PE, 1), "weights[3]");
  }
  {
    auto p = d.peel;
    p[3 * 1 + 0] = 99;
    refused("peel range", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "peel row 1: node id out of range");
    p = d.peel;
    p[3 * 1 + 1] = p[3 * 1 + 0];
    refused("peel same", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "peel row 1: the two children are the same");
    p = d.peel;
    p[3 * 0 + 0] = 9;  // an internal node not yet made
    refused("peel early", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "peel row 0: a child is used before");
    p = d.peel;
    p[3 * 2 + 0] = p[3 * 0 + 0];
    refused("peel reuse", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "peel row 2: a child already has a parent");
    p = d.peel;
    p[3 * 1 + 2] = p[3 * 0 + 2];
    refused("peel twice", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "peel row 1: the parent is computed twice");
    p = d.peel;
    std::swap(p[3 * 5 + 0], p[3 * 5 + 1]);  // (2S-3, child1, 2S-2)
    refused("unrooted last", call(7, 17, 20, 4, 0, M, W, p.data(), 1), "the last peel row must be (child1, 2S-3, 2S-2)");
    CHECK(call(7, 17, 20, 4, 1, M, W, p.data(), 1) == PHY_OK, "rooted takes either order: %s", g_err.c_str());
    CHECK(pl.B == 12 && pl.rows[5 * KR_INTS + KR_FOLD] == 0, "rooted: B and no fold");
    p = d.peel;
    p[3 * 5 + 2] = 11, p[3 * 4 + 2] = 12;  // the root made early
    p[3 * 5 + 1] = 12;
    refused("rooted last", call(7, 17, 20, 4, 1, M, W, p.data(), 1), "node 2S-2 belongs to the last row");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
