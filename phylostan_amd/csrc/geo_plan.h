// geo_plan.h -- the host planner of the K-state discrete-trait engine
// (geo_engine.inc): it validates S, K and the peel (phy_geo_create's
// refusals) and produces the level schedule, the LDS layout and the per-draw
// workspace the kernel runs on.
//
// Plain C++17: no HIP header, no device code, no device memory.  phylo_hip.hip
// includes it after sweep_plan.h (whose fail() / g_err it reports through);
// tests/geo_plan_check.cpp compiles it with a host compiler alone.
#ifndef PHYLO_GEO_PLAN_H
#define PHYLO_GEO_PLAN_H

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "sweep_plan.h"

namespace {

constexpr int GEO_KMIN = 2;
constexpr int GEO_KMAX = 64;         // three K x K fp64 matrices: 96 KiB of the CU's 160 KiB
constexpr int GEO_MAX_THREADS = 512;  // workgroup size at K > 16 (256 below)
constexpr int GEO_NVEC = 8;          // LDS K-vectors: lam, sqrt(pi), 1/sqrt(pi), pi, diag(Qu), rowt, colt, dd
constexpr int GEO_WS_ARRAYS = 8;     // per-node K-vectors in the per-workgroup global workspace (GW_* below)
constexpr size_t GEO_WS_BUDGET = (size_t)1 << 29;  // bytes of workspace over all workgroups
constexpr size_t GEO_LDS_CAP = 160 * 1024;
// rows of the level schedule: 4 ints each
enum { GR_A = 0, GR_B, GR_P, GR_LAST, GR_INTS };
// per-node K-vectors of the workspace, [array][node][K]
enum { GW_LOW = 0, GW_C, GW_MSG, GW_UT, GW_AA, GW_E, GW_UP, GW_EM };  // GW_E: exp(lam t); GW_EM: expm1(lam t)

// The LDS layout, in doubles from the 16-byte aligned dynamic base (kernel and
// planner share it).  Matrix rows are KP doubles apart: odd, so that a column
// walk (lanes i, address i * KP + k) touches 32 distinct bank pairs.
struct GeoLds {
  int K, KP, mat, vec;
  PHY_HD explicit GeoLds(int k) : K(k), KP(k | 1), mat((k * (k | 1) + 1) & ~1), vec((k + 1) & ~1) {}
  PHY_HD int A() const { return 0; }         // the symmetric A; then 1 / (lam_k - lam_l); then W V^T
  PHY_HD int V() const { return mat; }       // eigenvectors
  PHY_HD int W() const { return 2 * mat; }   // W; then sym(V W V^T)
  PHY_HD int vecs(int i) const { return 3 * mat + i * vec; }
  PHY_HD int cs() const { return vecs(GEO_NVEC); }           // rotation cosines, GEO_KMAX / 2
  PHY_HD int sn() const { return cs() + GEO_KMAX / 2; }      // sines
  PHY_HD int red() const { return sn() + GEO_KMAX / 2; }     // reduction scratch, GEO_MAX_THREADS
  PHY_HD int pq() const { return red() + GEO_MAX_THREADS; }  // rotation pairs: GEO_KMAX ints in GEO_KMAX / 2 doubles
  PHY_HD int doubles() const { return pq() + GEO_KMAX / 2; }
};

struct GeoPlan {
  int S = 0, K = 0, R = 0, B = 0, N = 0;
  int nlev = 0;                   // levels of internal nodes (the root's row is the last level, alone)
  std::vector<int32_t> rows;      // [S-1][GR_INTS], level by level
  std::vector<int32_t> lvl_off;   // [nlev + 1] first row of each level
  int widest = 0;                 // rows of the widest level
  int threads = 0;                // workgroup size
  int workgroups = 0;             // grid cap: draws beyond it are looped over
  size_t lds_bytes = 0;
  size_t ws_doubles = 0;          // workspace doubles per workgroup
};

// row lengths, in doubles; PHY_HD: the kernels take them from here too
PHY_HD inline int geo_rate_count(int K) { return K * (K - 1) / 2; }
PHY_HD inline int geo_param_len(int K) { return geo_rate_count(K) + K; }
PHY_HD inline int geo_row_len(int S, int K) { return 1 + (2 * S - 3) + geo_param_len(K); }  // log L, d/dblens, d/dparams
PHY_HD inline int geo_summary_len(int S, int K) { return (2 * S - 1) * K + K * K + (2 * S - 3); }  // marg, jumps, bjumps

// peel[(S-1)*3]: rows (child1, child2, parent) in post-order, the project's
// unrooted convention (phylo_hip.h): the last row's parent is the root 2S-2
// and its child2 is node 2S-3, whose branch is merged into child1's.
int geo_plan(int S, int K, const int32_t* peel, int max_draws, int cu_count, GeoPlan& out) {
  if (S < 3) return fail(PHY_EINVAL, "phy_geo_create: need S >= 3 tips");
  if (S > (1 << 20)) return fail(PHY_EINVAL, "phy_geo_create: S too large");
  if (K < GEO_KMIN || K > GEO_KMAX)
    return fail(PHY_EINVAL, "phy_geo_create: K = " + std::to_string(K) + " states, supported 2..64");
  if (!peel) return fail(PHY_EINVAL, "phy_geo_create: peel is NULL");
  if (max_draws < 1) return fail(PHY_EINVAL, "phy_geo_create: max_draws must be >= 1");
  const int N = 2 * S - 1, root = 2 * S - 2, merged = 2 * S - 3;
  std::vector<int> level(N, -1), used(N, 0);
  for (int t = 0; t < S; ++t) level[t] = 0;
  int nlev = 0;
  for (int r = 0; r < S - 1; ++r) {
    const int a = peel[3 * r], b = peel[3 * r + 1], p = peel[3 * r + 2];
    const std::string row = "phy_geo_create: peel row " + std::to_string(r);
    if (a < 0 || a >= N || b < 0 || b >= N || p < S || p >= N) return fail(PHY_EINVAL, row + ": node id out of range");
    if (a == b) return fail(PHY_EINVAL, row + ": the two children are the same node");
    if (level[a] < 0 || level[b] < 0) return fail(PHY_EINVAL, row + ": a child is used before it is computed");
    if (used[a] || used[b]) return fail(PHY_EINVAL, row + ": a child already has a parent");
    if (level[p] >= 0) return fail(PHY_EINVAL, row + ": the parent is computed twice");
    const bool last = r == S - 2;
    if (last && (p != root || b != merged))
      return fail(PHY_EINVAL, "phy_geo_create: the last peel row must be (child1, 2S-3, 2S-2)");
    if (!last && (p == root || a == merged || b == merged))
      return fail(PHY_EINVAL, row + ": nodes 2S-3 and 2S-2 belong to the last row");
    used[a] = used[b] = 1;
    level[p] = 1 + std::max(level[a], level[b]);
    nlev = std::max(nlev, level[p]);
  }
  out = GeoPlan();
  out.S = S, out.K = K, out.R = geo_rate_count(K), out.B = 2 * S - 3, out.N = N, out.nlev = nlev;
  out.lvl_off.assign(nlev + 1, 0);
  for (int r = 0; r < S - 1; ++r) ++out.lvl_off[level[peel[3 * r + 2]]];  // count of level l at [l], l >= 1
  for (int l = 1, at = 0; l <= nlev; ++l) {
    const int n = out.lvl_off[l];
    out.widest = std::max(out.widest, n);
    out.lvl_off[l] = at;  // slot l: start of level l (shifted down by one below)
    at += n;
  }
  std::vector<int> fill(out.lvl_off.begin(), out.lvl_off.end());
  out.rows.assign((size_t)(S - 1) * GR_INTS, 0);
  for (int r = 0; r < S - 1; ++r) {
    const int l = level[peel[3 * r + 2]];
    int32_t* w = &out.rows[(size_t)fill[l]++ * GR_INTS];
    w[GR_A] = peel[3 * r], w[GR_B] = peel[3 * r + 1], w[GR_P] = peel[3 * r + 2], w[GR_LAST] = r == S - 2;
  }
  for (int l = 0; l < nlev; ++l) out.lvl_off[l] = out.lvl_off[l + 1];
  out.lvl_off[nlev] = S - 1;
  out.threads = K <= 16 ? 256 : GEO_MAX_THREADS;
  out.lds_bytes = (size_t)GeoLds(K).doubles() * sizeof(double);
  if (out.lds_bytes > GEO_LDS_CAP) return fail(PHY_EINVAL, "phy_geo_create: LDS plan exceeds 160 KiB");
  out.ws_doubles = (size_t)GEO_WS_ARRAYS * N * K + 2 * (size_t)N;  // + each node's scale factor and shift
  // one workgroup per draw up to two per CU (the LDS admits one at K = 64), fewer when the workspace would
  // pass its budget
  size_t wgs = (size_t)std::max(cu_count, 1) * (out.lds_bytes * 2 <= GEO_LDS_CAP ? 2 : 1);
  wgs = std::min(wgs, std::max<size_t>(1, GEO_WS_BUDGET / (out.ws_doubles * sizeof(double))));
  out.workgroups = (int)std::min<size_t>(wgs, (size_t)max_draws);
  return PHY_OK;
}

// ---------------------------------------------------------------------------
// A sample of T trees on the same S tips (geo_trees.inc): the mixture
// likelihood sum_t w_t L_t.  Every tree keeps its own level schedule; the trees
// of a draw are split into G accumulation groups of consecutive trees, one
// workgroup walking a group in ascending tree order and folding what each tree
// leaves into one slot per (draw, group).  G and the split depend on T, S, K
// and the CU count alone -- never on max_draws or on a call's n_draws -- so a
// draw's sums have one order whatever batch it is in.
constexpr size_t GEO_TREES_DATA_BUDGET = (size_t)1 << 28;  // bytes of schedules, branch lengths and weights
constexpr size_t GEO_TREES_SLOT_BUDGET = (size_t)1 << 28;  // bytes of (draw, group) slots in flight
// the per-draw eigen record, in doubles: ok, sweeps, s, pad, lam[K], qd[K], V[K][K]
enum { GT_OK = 0, GT_SWEEPS, GT_S, GT_HEAD = 4 };
// a (draw, group) slot, in doubles: running max of log w_t + log L_t, sum of exp(that - max), pad, pad,
// W[K][K], colt - rowt [K], the root row [K], each the same exp-weighted sum
enum { GS_MAX = 0, GS_SUM, GS_HEAD = 4 };

struct GeoTreesPlan {
  int S = 0, K = 0, R = 0, B = 0, N = 0, T = 0;
  int G = 0;                       // accumulation groups per draw
  std::vector<int32_t> grp_off;    // [G + 1] group g walks trees grp_off[g] .. grp_off[g + 1] - 1
  std::vector<int32_t> rows;       // [T][S-1][GR_INTS] tree t's schedule, level by level
  std::vector<int32_t> lvl_off;    // tree t's [nlev_t + 1] level starts (rows of its own block) at lvl_start[t]
  std::vector<int32_t> lvl_start;  // [T + 1]
  int widest = 0, max_nlev = 0;    // over trees
  int threads = 0;
  int workgroups = 0;              // grid cap of the tree phase: (draw, group) items beyond it are looped over
  int draw_workgroups = 0;         // grid cap of the eigensolve and combine phases (one draw each)
  int chunk_draws = 0;             // draws whose slots are in flight at once (a call runs in chunks of them)
  size_t lds_bytes = 0, ws_doubles = 0, rec_doubles = 0, slot_doubles = 0, data_bytes = 0;
};

PHY_HD inline size_t geo_trees_rec_doubles(int K) { return (size_t)GT_HEAD + 2 * (size_t)K + (size_t)K * K; }
PHY_HD inline size_t geo_trees_slot_doubles(int K) { return (size_t)GS_HEAD + (size_t)K * K + 2 * (size_t)K; }
// beside each slot, for the summaries form alone: W2[K][K] and the first order [K] of the dwell times (geo_phases.inc),
// the same exp-weighted sums against the slot's running maximum
PHY_HD inline size_t geo_trees_dwell_doubles(int K) { return (size_t)K * K + (size_t)K; }
PHY_HD inline int geo_trees_row_len(int K) { return 1 + geo_param_len(K); }  // with a clock one more, d/dmu, last
PHY_HD inline int geo_trees_summary_len(int K) { return K * K + K; }

// peels[T][(S-1)*3], each tree by geo_plan's rules; a refusal names the tree.
int geo_trees_plan(int S, int K, int T, const int32_t* peels, int max_draws, int cu_count, GeoTreesPlan& out) {
  if (T < 1) return fail(PHY_EINVAL, "phy_geo_trees_create: T = " + std::to_string(T) + " trees, need T >= 1");
  if (!peels) return fail(PHY_EINVAL, "phy_geo_trees_create: peels is NULL");
  if (S >= 3 && S <= (1 << 20)) {  // before a tree is read: what the sample would hold on the device
    const size_t per_tree = (size_t)(S - 1) * GR_INTS * sizeof(int32_t) + (size_t)S * sizeof(int32_t) +
                            (size_t)(2 * S - 3) * sizeof(double) + sizeof(double);
    if ((size_t)T > GEO_TREES_DATA_BUDGET / per_tree)
      return fail(PHY_EINVAL, "phy_geo_trees_create: " + std::to_string(T) + " trees of " + std::to_string(S) +
                                  " tips need " + std::to_string(per_tree) + " bytes each, over the budget of " +
                                  std::to_string(GEO_TREES_DATA_BUDGET) + " bytes");
  }
  out = GeoTreesPlan();
  GeoPlan one;
  const size_t nrow = (size_t)(S > 1 ? S - 1 : 0);
  for (int t = 0; t < T; ++t) {
    const int rc = geo_plan(S, K, peels + (size_t)t * nrow * 3, max_draws, cu_count, one);
    if (rc) return fail(rc, "phy_geo_trees_create: tree " + std::to_string(t) + ": " + g_err);
    if (t == 0) {
      out.S = S, out.K = K, out.R = one.R, out.B = one.B, out.N = one.N, out.T = T;
      out.threads = one.threads, out.lds_bytes = one.lds_bytes, out.ws_doubles = one.ws_doubles;
      out.rows.reserve((size_t)T * one.rows.size());
      out.lvl_start.reserve((size_t)T + 1);
    }
    out.lvl_start.push_back((int32_t)out.lvl_off.size());
    out.rows.insert(out.rows.end(), one.rows.begin(), one.rows.end());
    out.lvl_off.insert(out.lvl_off.end(), one.lvl_off.begin(), one.lvl_off.end());
    out.widest = std::max(out.widest, one.widest);
    out.max_nlev = std::max(out.max_nlev, one.nlev);
  }
  out.lvl_start.push_back((int32_t)out.lvl_off.size());
  out.data_bytes = (out.rows.size() + out.lvl_off.size() + out.lvl_start.size()) * sizeof(int32_t) +
                   ((size_t)T * out.B + (size_t)T) * sizeof(double);
  out.rec_doubles = geo_trees_rec_doubles(K);
  out.slot_doubles = geo_trees_slot_doubles(K);
  // resident workgroups: up to two per CU (the LDS admits one at K = 64), fewer when the workspace would pass its
  // budget.  One draw's G groups fill them; more draws loop.
  size_t wgs = (size_t)std::max(cu_count, 1) * (out.lds_bytes * 2 <= GEO_LDS_CAP ? 2 : 1);
  wgs = std::min(wgs, std::max<size_t>(1, GEO_WS_BUDGET / (out.ws_doubles * sizeof(double))));
  out.workgroups = (int)wgs;
  out.draw_workgroups = (int)std::min<size_t>((size_t)std::max(cu_count, 1), (size_t)max_draws);
  out.G = (int)std::min<size_t>(std::min<size_t>(wgs, (size_t)GEO_MAX_THREADS), (size_t)T);  // the combine phase keeps G weights in LDS
  out.grp_off.resize((size_t)out.G + 1);
  for (int g = 0; g <= out.G; ++g) out.grp_off[g] = (int32_t)((long long)g * T / out.G);
  const size_t per_draw = (size_t)out.G * out.slot_doubles * sizeof(double);
  out.chunk_draws = (int)std::min<size_t>((size_t)max_draws, std::max<size_t>(1, GEO_TREES_SLOT_BUDGET / per_draw));
  return PHY_OK;
}

}  // namespace
#endif  // PHYLO_GEO_PLAN_H
