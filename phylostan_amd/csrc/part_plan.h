// part_plan.h -- the host planner of the partitioned engine (part_engine.inc):
// K disjoint site sets of one alignment on the same S tips and ONE tree, every
// partition with its own model vector and relative rate, evaluated row by row
// in one launch: row r = draw * K + k is partition k of its draw.
//
// Plain C++17 like sweep_plan.h, which it builds on.  The partitions are laid
// side by side in one padded alignment: partition k's P_k patterns start at
// column col0[k], a multiple of PART_ALIGN = 128 columns -- the block width of
// the two-column plan and two blocks of the one-column plan, so a block never
// holds columns of two partitions under either.  The columns between
// partitions carry mask 15 and weight 0, as the trailing padding always has:
// they contribute exactly nothing.  make_problem / plan_lds on that alignment
// give ONE plan for all rows (R and `extra` are those of the union of the tip
// masks; the row count is max_draws * K), and choose_launch's epilogue
// decisions are taken once at one workgroup per row, as forest_plan.h does.
// What differs per partition is the block range [blk_lo, blk_hi) a row walks.
// tests/part_plan_check.cpp compiles this file with a host compiler alone.
#ifndef PHYLO_PART_PLAN_H
#define PHYLO_PART_PLAN_H

#include "sweep_plan.h"

namespace {

constexpr int PART_ALIGN = 2 * WAVE;    // columns: a partition's first column is a multiple of it
constexpr int PART_MAX_ROWS = 65535;    // the grid's rows (one workgroup per row in y)

struct PartPlan {
  int K = 0, max_draws = 0;
  int Psum = 0;                    // the caller's patterns, sum of P_k
  Problem pb;                      // the padded alignment: P = col0[K-1] + P_{K-1}, max_draws = max_draws * K
  SweepPlan plan;                  // the common LDS plan
  std::vector<int> Pk, col0, off;  // [K] patterns, first padded column, first caller column
  std::vector<int> blk;            // [K][2] block range [lo, hi) at the plan's columns per lane
  std::vector<int> col_part, col_pat;  // [P] padded column -> partition and pattern in it (-1, -1 between partitions)
  int fin = 0, qf = 0, fin_qf = 0;     // the epilogue's form (choose_launch's, at one workgroup per row)
};

// Refusals are PHY_EINVAL: K < 1, a partition without patterns (the message
// names it), max_draws * K past the grid's rows, and everything make_problem
// refuses on the padded alignment.
int part_plan(int S, int K, const int32_t* Pk, int C, int rooted, int kind, const uint8_t* tipcodes,
              const double* weights, const int32_t* peel, int max_draws, const Prefs& prefs, int cu_count,
              PartPlan& pp) {
  if (K < 1) return fail(PHY_EINVAL, "partitions: need K >= 1 partitions");
  if (!Pk || !tipcodes || !weights || !peel) return fail(PHY_EINVAL, "NULL input array");
  if (S < 3) return fail(PHY_EINVAL, "need S >= 3 taxa");
  if (max_draws < 1) return fail(PHY_EINVAL, "max_draws must be >= 1");
  long long psum = 0, ptot = 0;
  for (int k = 0; k < K; ++k) {
    if (Pk[k] < 1) return fail(PHY_EINVAL, "partition " + std::to_string(k) + ": need P_k >= 1 patterns");
    ptot = (ptot + PART_ALIGN - 1) / PART_ALIGN * PART_ALIGN + Pk[k];
    psum += Pk[k];
    if (ptot > (long long)INT_MAX / 4) return fail(PHY_EINVAL, "partition " + std::to_string(k) + ": the padded alignment is too wide");
  }
  if ((long long)max_draws * K > PART_MAX_ROWS)
    return fail(PHY_EINVAL, "partitions: max_draws * K = " + std::to_string((long long)max_draws * K) +
                                " rows pass the grid's " + std::to_string(PART_MAX_ROWS) + " (K = " + std::to_string(K) + ")");
  pp = PartPlan();
  pp.K = K; pp.max_draws = max_draws; pp.Psum = (int)psum;
  pp.Pk.assign(Pk, Pk + K);
  pp.col0.assign(K, 0);
  pp.off.assign(K, 0);
  const int P = (int)ptot;
  std::vector<uint8_t> tips((size_t)S * P, (uint8_t)15);
  std::vector<double> w((size_t)P, 0.0);
  pp.col_part.assign(P, -1);
  pp.col_pat.assign(P, -1);
  int col = 0, off = 0;
  for (int k = 0; k < K; ++k) {
    col = (col + PART_ALIGN - 1) / PART_ALIGN * PART_ALIGN;
    pp.col0[k] = col; pp.off[k] = off;
    for (int t = 0; t < S; ++t)
      std::copy(tipcodes + (size_t)t * psum + off, tipcodes + (size_t)t * psum + off + Pk[k], tips.begin() + (size_t)t * P + col);
    std::copy(weights + off, weights + off + Pk[k], w.begin() + col);
    for (int i = 0; i < Pk[k]; ++i) {
      pp.col_part[col + i] = k;
      pp.col_pat[col + i] = i;
    }
    col += Pk[k]; off += Pk[k];
  }
  int rc = make_problem(S, P, C, rooted, kind, tips.data(), w.data(), peel, max_draws * K, pp.pb);
  if (rc) return rc;
  if ((rc = plan_lds(pp.pb, prefs, cu_count, pp.plan))) return rc;
  const int bw = WAVE * pp.plan.K;  // columns of a block
  pp.blk.assign((size_t)2 * K, 0);
  for (int k = 0; k < K; ++k) {
    pp.blk[2 * k] = pp.col0[k] / bw;
    pp.blk[2 * k + 1] = (pp.col0[k] + Pk[k] + bw - 1) / bw;
    if (pp.blk[2 * k + 1] > pp.plan.nblk)
      return fail(PHY_EINVAL, "partition " + std::to_string(k) + ": internal: block range past the plan's blocks");
  }
  const RowForm form = row_epilogue_form(pp.pb, prefs, pp.plan);
  pp.fin = form.fin; pp.qf = form.qf; pp.fin_qf = form.fin_qf;
  return PHY_OK;
}

}  // namespace

#endif  // PHYLO_PART_PLAN_H
