// forest_plan.h -- the host planner of the forest engine (forest_engine.inc):
// T binary trees on the same S tips and one alignment, evaluated row by row in
// one launch, every row naming its tree.
//
// Plain C++17 like sweep_plan.h, which it builds on: every peel goes through
// parse_peel / build_program, ONE LDS plan (plan_lds's logic at the largest
// deep stack of the forest and max_draws = max_rows) serves all trees, and the
// chunk plan and the device records are made per tree at that common cap_m.
// What differs per tree is the step program (records), the matrix numbering
// (mat_branch / gpos), the chunk boundaries, the rebuilt-cherry flags and the
// deep-stack depth; the tip nibbles, R, extra and every size are the data's.
//
// The kernel form is the context's, never a call's: K, latency or batched
// register budget, deep-stack placement, one workgroup per row, and whether
// the finalize and the chain rule run inside the sweep.  A row's bits depend
// on nothing but the row.  tests/forest_plan_check.cpp compiles this file with
// a host compiler alone.
#ifndef PHYLO_FOREST_PLAN_H
#define PHYLO_FOREST_PLAN_H

#include "sweep_plan.h"

namespace {

constexpr size_t FOREST_TABLE_CAP = (size_t)256 << 20;  // bytes of per-tree tables on the device

struct ForestPlan {
  int T = 0;
  Problem pb;      // the data, the sizes and tree 0's program; ndeep is the forest's largest
  SweepPlan plan;  // the common LDS plan (K, lat, nblk, cap_m, ndl, deep_lds, lds); prog / records are tree 0's
  int rec_stride = 0;                      // ints per tree in `records`
  std::vector<int> records;                // [T][rec_stride] device step records (batched K = 2, packed K = 1)
  std::vector<int> mat_branch, gpos;       // [T][nmat], [T][B]
  std::vector<int> nchunks, ndeep, nrec;   // [T]
  int fin = 0, qf = 0, fin_qf = 0;         // the epilogue's form (choose_launch's, at one workgroup per row)
  int max_chunks = 0, min_chunks = 0, max_depth = 0, min_depth = 0;
};

// Refusals are PHY_EINVAL: T < 1, tables past FOREST_TABLE_CAP, and
// everything make_problem refuses; a tree's refusal names its index.
int forest_plan(int S, int P, int C, int rooted, int kind, const uint8_t* tipcodes, const double* weights, int T,
                const int32_t* peels, int max_rows, const Prefs& prefs, int cu_count, ForestPlan& fp) {
  if (T < 1) return fail(PHY_EINVAL, "forest: need T >= 1 trees");
  if (S < 3) return fail(PHY_EINVAL, "need S >= 3 taxa");
  if (P < 1) return fail(PHY_EINVAL, "need P >= 1 patterns");
  if (C < 1 || C > 16) return fail(PHY_EINVAL, "C must be in 1..16");
  if (kind < PHY_JC69 || kind > PHY_GTR) return fail(PHY_EINVAL, "unknown model");
  if (max_rows < 1) return fail(PHY_EINVAL, "max_rows must be >= 1");
  if (!tipcodes || !weights || !peels) return fail(PHY_EINVAL, "NULL input array");
  const int B = rooted ? 2 * S - 2 : 2 * S - 3;
  const size_t peel_len = (size_t)(S - 1) * 3;
  // per tree: USTEP ints a step at most, the matrix numbering and its inverse
  if ((size_t)T * ((size_t)(S - 1) * USTEP + 2 * (size_t)B) * sizeof(int) > FOREST_TABLE_CAP)
    return fail(PHY_EINVAL, "forest: the trees' tables pass 256 MiB on the device");
  fp = ForestPlan();
  fp.T = T;
  std::vector<std::vector<int>> progs(T);
  fp.ndeep.assign(T, 0);
  fp.mat_branch.reserve((size_t)T * B);
  fp.gpos.assign((size_t)T * B, -1);
  int ndmax = 0;
  for (int t = 0; t < T; ++t) {
    std::vector<int> mb;
    int nslots = 0, nd = 0;
    const int rc = build_program(S, peels + (size_t)t * peel_len, rooted ? 1 : 0, progs[t], mb, nslots, nd);
    if (rc) return fail(rc, "tree " + std::to_string(t) + ": " + g_err);
    if ((int)mb.size() != B) return fail(PHY_EINVAL, "tree " + std::to_string(t) + ": internal: one matrix per branch expected");
    if (nd > 127) return fail(PHY_EINVAL, "tree " + std::to_string(t) + ": deep stack > 127 (the packed program's field width)");
    for (int m = 0; m < B; ++m) fp.gpos[(size_t)t * B + mb[m]] = m;
    for (int b = 0; b < B; ++b)
      if (fp.gpos[(size_t)t * B + b] < 0)
        return fail(PHY_EINVAL, "tree " + std::to_string(t) + ": internal: branch " + std::to_string(b) + " not in the program");
    fp.mat_branch.insert(fp.mat_branch.end(), mb.begin(), mb.end());
    fp.ndeep[t] = nd;
    ndmax = std::max(ndmax, nd);
  }
  int rc = make_problem(S, P, C, rooted, kind, tipcodes, weights, peels, max_rows, fp.pb);
  if (rc) return rc;
  fp.pb.ndeep = ndmax;  // regions and LDS are sized by the deepest tree
  if ((rc = plan_lds(fp.pb, prefs, cu_count, fp.plan))) return rc;
  const SweepPlan& pl = fp.plan;
  fp.rec_stride = (S - 1) * (pl.K == 2 ? USTEP : PSTEP);
  fp.records.reserve((size_t)T * fp.rec_stride);
  fp.nchunks.assign(T, 0);
  fp.nrec.assign(T, 0);
  for (int t = 0; t < T; ++t) {
    if ((rc = assign_chunks(progs[t], S - 1, B, pl.cap_m, prefs.recompute, fp.nchunks[t], fp.nrec[t])))
      return fail(rc, "tree " + std::to_string(t) + ": " + g_err);
    const std::vector<int> recs = pl.K == 2 ? batched_records(progs[t], pl.K, C, fp.pb.R) : pack_program(progs[t]);
    fp.records.insert(fp.records.end(), recs.begin(), recs.end());
  }
  fp.max_chunks = *std::max_element(fp.nchunks.begin(), fp.nchunks.end());
  fp.min_chunks = *std::min_element(fp.nchunks.begin(), fp.nchunks.end());
  fp.max_depth = ndmax;
  fp.min_depth = *std::min_element(fp.ndeep.begin(), fp.ndeep.end());
  const RowForm form = row_epilogue_form(fp.pb, prefs, pl);
  fp.fin = form.fin; fp.qf = form.qf; fp.fin_qf = form.fin_qf;
  return PHY_OK;
}

}  // namespace

#endif  // PHYLO_FOREST_PLAN_H
