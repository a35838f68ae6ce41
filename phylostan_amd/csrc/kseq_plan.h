// kseq_plan.h -- the host planner of the K-state sequence likelihood engine
// (kseq_engine.inc): an alignment of P patterns under a mixture over sites of
// M reversible models of 2 <= K <= 64 states, each with C rate categories,
// tips as uint64 masks.  phy_kseq_* is M = 1 (kseq_plan), phy_kseq_mix_* any
// 1 <= M <= 8 with M C <= 16 (kseq_mix_plan); the component-category index
// g = m C + c runs over G = M C wherever one model has its category.  It makes
// every refusal of the create calls and builds every host array the device
// reads: the tip masks and weights per pattern tile, the schedule rows, and
// every length and offset of the record, the item workspace, the slot and the
// per-chunk arrays.  The engine file allocates what the plan sizes and copies
// what the plan built; it computes no size or offset of its own, and the
// kernels take theirs from the PHY_HD helpers below.
//
// Plain C++17: no HIP header, no device code, no device memory.  phylo_hip.hip
// includes it after geo_plan.h; tests/kseq_plan_check.cpp compiles it with a
// host compiler alone, under the address and undefined-behaviour sanitizers.
#ifndef PHYLO_KSEQ_PLAN_H
#define PHYLO_KSEQ_PLAN_H

#include <cmath>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <string>
#include <vector>

#include "sweep_plan.h"
#include "geo_plan.h"  // GeoLds: the per-draw kernels run the geo phases on its layout

namespace {

constexpr int KSEQ_KMIN = 2;
constexpr int KSEQ_KMAX = 64;
constexpr int KSEQ_CMAX = 16;            // categories of one model, and component-categories M C of a mixture
constexpr int KSEQ_MMAX = 8;             // components of a mixture
constexpr int KSEQ_PT = 16;             // patterns per tile: the N of the 16x16x4 fp64 MFMA
constexpr int KSEQ_XS = KSEQ_PT + 1;    // LDS row stride of a KT x 16 operand: odd, a column walk is conflict-free
constexpr int KSEQ_DRAW_THREADS = 512;  // the per-draw kernels at K > 16 (256 below), as the geo engines
constexpr int KSEQ_SITE_THREADS = 256;
// bytes of item workspace in flight (all items of a chunk are resident: the way down reads what the way up left).
// fluA codon (S = 69, P = 242, K = 61, C = 4): 64 items of 3.4 MB, 216 MB a draw: 4 draws per chunk.
constexpr size_t KSEQ_WS_BUDGET = (size_t)1 << 30;
constexpr size_t KSEQ_LDS_CAP = 160 * 1024;
// schedule rows: 4 ints each, in peel order (an item walks the tree row by row)
enum { KR_A = 0, KR_B, KR_P, KR_FOLD, KR_INTS };
// the record of a (draw, component), [n][M][rec_doubles]; the draw's verdict fields KREC_BAD and KREC_LL are read
// in component 0's alone.  In doubles: ok, sweeps, s, the site phase's verdict (1: bad draw), log L, pad;
// then lam[K], qd[K], V[K][K], sqrt(pi)[K], 1/sqrt(pi)[K]
enum { KREC_OK = 0, KREC_SWEEPS, KREC_S, KREC_BAD, KREC_LL, KREC_HEAD = 8 };

// a * b, or false when the product leaves size_t
inline bool kseq_mul(size_t a, size_t b, size_t& out) {
  if (a != 0 && b > std::numeric_limits<size_t>::max() / a) return false;
  out = a * b;
  return true;
}

PHY_HD inline int kseq_kt(int K) { return 16 * ((K + 15) / 16); }
PHY_HD inline int kseq_ntiles(int P) { return (P + KSEQ_PT - 1) / KSEQ_PT; }
PHY_HD inline int kseq_rate_count(int K) { return K * (K - 1) / 2; }
PHY_HD inline int kseq_num_branches(int S, int rooted) { return rooted ? 2 * S - 2 : 2 * S - 3; }
PHY_HD inline int kseq_param_len(int K, int C) { return kseq_rate_count(K) + K + 2 * C; }  // rates freqs rs ps
// the row: log L, d/dblens B, d/drs C, d/dps C, d/drates R, d/dfreqs K
PHY_HD inline int kseq_row_len(int B, int K, int C) { return 1 + B + 2 * C + kseq_rate_count(K) + K; }
PHY_HD inline int kseq_row_blens() { return 1; }
PHY_HD inline int kseq_row_rs(int B) { return 1 + B; }
PHY_HD inline int kseq_row_ps(int B, int C) { return 1 + B + C; }
PHY_HD inline int kseq_row_rates(int B, int C) { return 1 + B + 2 * C; }
PHY_HD inline int kseq_row_freqs(int B, int K, int C) { return 1 + B + 2 * C + kseq_rate_count(K); }
// params
PHY_HD inline int kseq_par_freqs(int K) { return kseq_rate_count(K); }
PHY_HD inline int kseq_par_rs(int K) { return kseq_rate_count(K) + K; }
PHY_HD inline int kseq_par_ps(int K, int C) { return kseq_rate_count(K) + K + C; }

// the mixture: params [rates_0 R][freqs_0 K] .. [rates_{M-1}][freqs_{M-1}][rs M C][ps M C], the row [log L]
// [d/dblens B][d/drs M C][d/dps M C][d/drates_0 R][d/dfreqs_0 K] ..; at M = 1 every one is its namesake above
PHY_HD inline int kseq_mix_param_len(int K, int M, int C) { return M * (kseq_rate_count(K) + K) + 2 * M * C; }
PHY_HD inline int kseq_mix_par_comp(int K, int m) { return m * (kseq_rate_count(K) + K); }  // rates_m; freqs_m R on
PHY_HD inline int kseq_mix_par_rs(int K, int M) { return M * (kseq_rate_count(K) + K); }
PHY_HD inline int kseq_mix_par_ps(int K, int M, int C) { return M * (kseq_rate_count(K) + K) + M * C; }
PHY_HD inline int kseq_mix_row_len(int B, int K, int M, int C) {
  return 1 + B + 2 * M * C + M * (kseq_rate_count(K) + K);
}
PHY_HD inline int kseq_mix_row_rates(int B, int K, int M, int C, int m) {
  return 1 + B + 2 * M * C + m * (kseq_rate_count(K) + K);
}
PHY_HD inline int kseq_mix_row_freqs(int B, int K, int M, int C, int m) {
  return kseq_mix_row_rates(B, K, M, C, m) + kseq_rate_count(K);
}

// the record
PHY_HD inline size_t kseq_rec_lam(int) { return KREC_HEAD; }
PHY_HD inline size_t kseq_rec_qd(int K) { return (size_t)KREC_HEAD + K; }
PHY_HD inline size_t kseq_rec_v(int K) { return (size_t)KREC_HEAD + 2 * (size_t)K; }
PHY_HD inline size_t kseq_rec_sq(int K) { return kseq_rec_v(K) + (size_t)K * K; }
PHY_HD inline size_t kseq_rec_isq(int K) { return kseq_rec_sq(K) + K; }
PHY_HD inline size_t kseq_rec_doubles(int K) { return kseq_rec_isq(K) + K; }
PHY_HD inline size_t kseq_rec_at(int draw, int m, int M, int K) { return ((size_t)draw * M + m) * kseq_rec_doubles(K); }
PHY_HD inline size_t kseq_cpost_at(int draw, int m, int M, int P) { return ((size_t)draw * M + m) * (size_t)P; }

// the item workspace, in doubles: per node a KT x 16 block ([state][pattern]) of the scaled lower partial (the way
// down overwrites an internal node's with its upward vector), of c and of msg, then the node's 16 column factors
PHY_HD inline size_t kseq_blk(int KT) { return (size_t)KT * KSEQ_PT; }
PHY_HD inline size_t kseq_ws_low(int, int) { return 0; }
PHY_HD inline size_t kseq_ws_cc(int N, int KT) { return (size_t)N * kseq_blk(KT); }
PHY_HD inline size_t kseq_ws_msg(int N, int KT) { return 2 * (size_t)N * kseq_blk(KT); }
PHY_HD inline size_t kseq_ws_sf(int N, int KT) { return 3 * (size_t)N * kseq_blk(KT); }
PHY_HD inline size_t kseq_ws_doubles(int N, int KT) { return kseq_ws_sf(N, KT) + (size_t)N * KSEQ_PT; }

// the (draw, component-category, tile) slot, in doubles: W[KT][KT], colt - rowt [KT], rootpi [KT], G per branch [B],
// the item's share of d/drs_c and of d/dps_c, padded to an even count
PHY_HD inline size_t kseq_slot_w(int) { return 0; }
PHY_HD inline size_t kseq_slot_dvec(int KT) { return (size_t)KT * KT; }
PHY_HD inline size_t kseq_slot_rootpi(int KT) { return (size_t)KT * KT + KT; }
PHY_HD inline size_t kseq_slot_gb(int KT) { return (size_t)KT * KT + 2 * (size_t)KT; }
PHY_HD inline size_t kseq_slot_grs(int KT, int B) { return kseq_slot_gb(KT) + B; }
PHY_HD inline size_t kseq_slot_gps(int KT, int B) { return kseq_slot_grs(KT, B) + 1; }
PHY_HD inline size_t kseq_slot_doubles(int KT, int B) { return (kseq_slot_gps(KT, B) + 1 + 1) & ~(size_t)1; }

// The LDS of the item kernels, in doubles from the 16-byte aligned dynamic base.  V and the 1 / (lam_k - lam_l)
// table are KT x KT with rows VS = KT + 1 doubles apart (odd); the operands are KT x 16 with rows KSEQ_XS apart.
struct KseqLds {
  int KT, VS, mat, op;
  PHY_HD explicit KseqLds(int kt) : KT(kt), VS(kt + 1), mat((kt * (kt + 1) + 1) & ~1), op((kt * KSEQ_XS + 1) & ~1) {}
  PHY_HD int V() const { return 0; }
  PHY_HD int X(int i) const { return mat + i * op; }            // operands 0, 1 (both kernels), 2, 3 (the way down)
  PHY_HD int vecs(int i) const { return mat + 4 * op + i * KT; }  // lam, sqrt(pi), 1/sqrt(pi), pi, e, expm1
  PHY_HD int red() const { return vecs(6); }                    // [4 waves][16 columns]
  PHY_HD int col() const { return red() + 64; }                 // [2][16] per-column values
  PHY_HD int up_doubles() const { return col() + 32; }
  PHY_HD int RT() const { return up_doubles(); }                // the way down alone: 1 / (lam_k - lam_l)
  PHY_HD int down_doubles() const { return RT() + mat; }
};

struct KseqPlan {
  int S = 0, P = 0, K = 0, C = 0, rooted = 0, B = 0, N = 0, R = 0;
  int M = 1, G = 0;                 // components, component-categories M C
  int KT = 0, NB = 0;               // padded states, 16-row blocks (= waves of an item's workgroup)
  int ntiles = 0, PP = 0;           // pattern tiles, padded patterns
  int items_per_draw = 0;           // G * ntiles
  int max_draws = 0, chunk_draws = 0;
  int threads = 0;                  // item kernels: 64 * NB
  int draw_threads = 0;             // eigen and combine kernels
  int site_threads = 0;
  int workgroups = 0;               // grid cap of the item kernels
  int draw_workgroups = 0;          // grid cap of the per-draw kernels
  int comp_workgroups = 0;          // grid cap of the per-(draw, component) kernels: the eigensolve and the combine
  int param_len = 0, row_len = 0;
  size_t lds_up = 0, lds_down = 0, lds_draw = 0;  // bytes
  size_t rec_doubles = 0, ws_doubles = 0, slot_doubles = 0;
  // device buffers, in elements
  size_t n_params = 0, n_blens = 0, n_rec = 0, n_rows_out = 0, n_site = 0;  // [max_draws][.]
  size_t n_ws = 0, n_slots = 0;                                            // [chunk_draws][items_per_draw][.]
  size_t n_lc = 0, n_sh = 0, n_down0 = 0;  // [chunk_draws][G][PP] twice, [chunk_draws][PP]
  size_t n_cpost = 0;                      // [max_draws][M][P]
  std::vector<uint64_t> tile_masks;  // [ntiles][S][16], padding columns all K bits
  std::vector<double> tile_w;        // [ntiles][16], padding columns 0
  std::vector<int32_t> rows;         // [S-1][KR_INTS]
};

// offsets of the per-chunk arrays (dl: the draw within its chunk; a mixture passes g and G for c and C)
PHY_HD inline size_t kseq_lc_at(int dl, int c, int C, int PP) { return ((size_t)dl * C + c) * (size_t)PP; }
PHY_HD inline size_t kseq_down0_at(int dl, int PP) { return (size_t)dl * PP; }
PHY_HD inline size_t kseq_item(int dl, int c, int tile, int C, int ntiles) {
  return ((size_t)dl * C + c) * (size_t)ntiles + tile;
}
PHY_HD inline size_t kseq_mask_at(int tile, int node, int S) { return ((size_t)tile * S + node) * KSEQ_PT; }

// peel[(S-1)*3]: rows (child1, child2, parent) in post-order.  Rooted: the last row's parent is the root 2S-2 and
// every non-root node has a branch, B = 2S-2.  Unrooted: the last row is (child1, 2S-3, 2S-2) and node 2S-3's
// branch is merged into child1's, B = 2S-3.
// who: the call the messages name.
int kseq_mix_plan(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                  const int32_t* peel, int max_draws, int cu_count, KseqPlan& out,
                  const std::string& who = "phy_kseq_mix_create: ") {
  if (S < 3) return fail(PHY_EINVAL, who + "S = " + std::to_string(S) + " tips, need S >= 3");
  if (S > (1 << 20)) return fail(PHY_EINVAL, who + "S too large");
  if (P < 1) return fail(PHY_EINVAL, who + "P = " + std::to_string(P) + " patterns, need P >= 1");
  if (P > (1 << 28)) return fail(PHY_EINVAL, who + "P too large");
  if (K < KSEQ_KMIN || K > KSEQ_KMAX)
    return fail(PHY_EINVAL, who + "K = " + std::to_string(K) + " states, supported 2..64");
  if (M < 1 || M > KSEQ_MMAX)
    return fail(PHY_EINVAL, who + "M = " + std::to_string(M) + " components, supported 1..8");
  if (C < 1 || C > KSEQ_CMAX)
    return fail(PHY_EINVAL, who + "C = " + std::to_string(C) + " categories, supported 1..16");
  if (M * C > KSEQ_CMAX)
    return fail(PHY_EINVAL, who + "M * C = " + std::to_string(M * C) + " component-categories, supported up to 16");
  if (max_draws < 1) return fail(PHY_EINVAL, who + "max_draws must be >= 1");
  if (!tipmasks) return fail(PHY_EINVAL, who + "tipmasks is NULL");
  if (!weights) return fail(PHY_EINVAL, who + "weights is NULL");
  if (!peel) return fail(PHY_EINVAL, who + "peel is NULL");
  rooted = rooted ? 1 : 0;
  const int N = 2 * S - 1, root = 2 * S - 2, merged = 2 * S - 3;
  {
    std::vector<char> made(N, 0), used(N, 0);
    for (int t = 0; t < S; ++t) made[t] = 1;
    for (int r = 0; r < S - 1; ++r) {
      const int a = peel[3 * r], b = peel[3 * r + 1], p = peel[3 * r + 2];
      const std::string row = who + "peel row " + std::to_string(r);
      if (a < 0 || a >= N || b < 0 || b >= N || p < S || p >= N)
        return fail(PHY_EINVAL, row + ": node id out of range");
      if (a == b) return fail(PHY_EINVAL, row + ": the two children are the same node");
      if (!made[a] || !made[b]) return fail(PHY_EINVAL, row + ": a child is used before it is computed");
      if (used[a] || used[b]) return fail(PHY_EINVAL, row + ": a child already has a parent");
      if (made[p]) return fail(PHY_EINVAL, row + ": the parent is computed twice");
      const bool last = r == S - 2;
      if (rooted) {
        if (last && p != root) return fail(PHY_EINVAL, row + ": the last peel row's parent must be 2S-2");
        if (!last && p == root) return fail(PHY_EINVAL, row + ": node 2S-2 belongs to the last row");
      } else {
        if (last && (p != root || b != merged))
          return fail(PHY_EINVAL, row + ": the last peel row must be (child1, 2S-3, 2S-2)");
        if (!last && (p == root || a == merged || b == merged))
          return fail(PHY_EINVAL, row + ": nodes 2S-3 and 2S-2 belong to the last row");
      }
      used[a] = used[b] = 1;
      made[p] = 1;
    }
  }
  const uint64_t full = K == 64 ? ~(uint64_t)0 : (((uint64_t)1 << K) - 1);
  for (size_t i = 0; i < (size_t)S * P; ++i) {
    const uint64_t m = tipmasks[i];
    const std::string at = who + "tipmasks[" + std::to_string(i / P) + "][" + std::to_string(i % P) + "]";
    if (m == 0) return fail(PHY_EINVAL, at + " has no bit set");
    if (m & ~full) return fail(PHY_EINVAL, at + " has a bit >= K set");
  }
  for (int i = 0; i < P; ++i)
    if (!(weights[i] >= 0.0) || !std::isfinite(weights[i]))
      return fail(PHY_EINVAL, who + "weights[" + std::to_string(i) + "] is negative or not finite");

  out = KseqPlan();
  out.S = S, out.P = P, out.K = K, out.C = C, out.rooted = rooted, out.N = N;
  out.M = M, out.G = M * C;
  out.B = kseq_num_branches(S, rooted), out.R = kseq_rate_count(K);
  out.KT = kseq_kt(K), out.NB = out.KT / 16;
  out.ntiles = kseq_ntiles(P), out.PP = out.ntiles * KSEQ_PT;
  out.items_per_draw = out.G * out.ntiles;  // <= 16 * 2^24
  out.max_draws = max_draws;
  out.threads = 64 * out.NB;
  out.draw_threads = K <= 16 ? 256 : KSEQ_DRAW_THREADS;
  out.site_threads = KSEQ_SITE_THREADS;
  out.param_len = kseq_mix_param_len(K, M, C);
  out.row_len = kseq_mix_row_len(out.B, K, M, C);
  const KseqLds L(out.KT);
  out.lds_up = (size_t)L.up_doubles() * sizeof(double);
  out.lds_down = (size_t)L.down_doubles() * sizeof(double);
  out.lds_draw = (size_t)GeoLds(K).doubles() * sizeof(double);
  if (out.lds_up > KSEQ_LDS_CAP || out.lds_down > KSEQ_LDS_CAP || out.lds_draw > KSEQ_LDS_CAP)
    return fail(PHY_EINVAL, who + "LDS plan exceeds 160 KiB");
  out.rec_doubles = kseq_rec_doubles(K);
  out.ws_doubles = kseq_ws_doubles(N, out.KT);
  out.slot_doubles = kseq_slot_doubles(out.KT, out.B);
  // one draw's items against the budget
  size_t ws_draw = 0, ws_draw_bytes = 0;
  const std::string big = who + "the workspace of one draw (" + std::to_string(out.items_per_draw) + " items of " +
                          std::to_string(out.ws_doubles) + " doubles) exceeds the budget of " +
                          std::to_string(KSEQ_WS_BUDGET) + " bytes";
  if (!kseq_mul((size_t)out.items_per_draw, out.ws_doubles, ws_draw) ||
      !kseq_mul(ws_draw, sizeof(double), ws_draw_bytes) || ws_draw_bytes > KSEQ_WS_BUDGET)
    return fail(PHY_EINVAL, big);
  out.chunk_draws = (int)std::min<size_t>((size_t)max_draws, std::max<size_t>(1, KSEQ_WS_BUDGET / ws_draw_bytes));
  const size_t nd = (size_t)max_draws, ch = (size_t)out.chunk_draws;
  size_t chunk_items = 0;
  bool ok = kseq_mul(ch, (size_t)out.items_per_draw, chunk_items);
  ok = ok && kseq_mul(nd, (size_t)out.param_len, out.n_params) && kseq_mul(nd, (size_t)out.B, out.n_blens) &&
       kseq_mul(nd * (size_t)M, out.rec_doubles, out.n_rec) && kseq_mul(nd * (size_t)M, (size_t)P, out.n_cpost) && kseq_mul(nd, (size_t)out.row_len, out.n_rows_out) &&
       kseq_mul(nd, (size_t)P, out.n_site) && kseq_mul(chunk_items, out.ws_doubles, out.n_ws) &&
       kseq_mul(chunk_items, out.slot_doubles, out.n_slots) && kseq_mul(ch * (size_t)out.G, (size_t)out.PP, out.n_lc) &&
       kseq_mul(ch, (size_t)out.PP, out.n_down0);
  size_t bytes = 0;
  for (size_t n : {out.n_params, out.n_blens, out.n_rec, out.n_rows_out, out.n_site, out.n_ws, out.n_slots, out.n_lc,
                   out.n_cpost})
    ok = ok && kseq_mul(n, sizeof(double), bytes);
  if (!ok) return fail(PHY_EINVAL, who + "a buffer size overflows (max_draws = " + std::to_string(max_draws) + ")");
  out.n_sh = out.n_lc;
  // resident workgroups of the item kernels: two per CU where the LDS admits them
  const size_t per_cu = out.lds_down * 2 <= KSEQ_LDS_CAP ? 2 : 1;
  out.workgroups = (int)std::min<size_t>((size_t)std::max(cu_count, 1) * per_cu, chunk_items);
  out.draw_workgroups = (int)std::min<size_t>((size_t)std::max(cu_count, 1), nd);
  out.comp_workgroups = (int)std::min<size_t>((size_t)std::max(cu_count, 1), nd * (size_t)M);

  out.tile_masks.assign((size_t)out.ntiles * S * KSEQ_PT, full);
  out.tile_w.assign((size_t)out.PP, 0.0);
  for (int i = 0; i < P; ++i) {
    const int tile = i / KSEQ_PT, col = i - tile * KSEQ_PT;
    out.tile_w[(size_t)tile * KSEQ_PT + col] = weights[i];
    for (int t = 0; t < S; ++t) out.tile_masks[kseq_mask_at(tile, t, S) + col] = tipmasks[(size_t)t * P + i];
  }
  out.rows.assign((size_t)(S - 1) * KR_INTS, 0);
  for (int r = 0; r < S - 1; ++r) {
    int32_t* w = &out.rows[(size_t)r * KR_INTS];
    w[KR_A] = peel[3 * r], w[KR_B] = peel[3 * r + 1], w[KR_P] = peel[3 * r + 2];
    w[KR_FOLD] = (!rooted && r == S - 2) ? 1 : 0;
  }
  return PHY_OK;
}

// one model: the mixture plan at M = 1
int kseq_plan(int S, int P, int K, int C, int rooted, const uint64_t* tipmasks, const double* weights,
              const int32_t* peel, int max_draws, int cu_count, KseqPlan& out) {
  return kseq_mix_plan(S, P, K, 1, C, rooted, tipmasks, weights, peel, max_draws, cu_count, out, "phy_kseq_create: ");
}

}  // namespace
#endif  // PHYLO_KSEQ_PLAN_H
