// seqsum_plan.h -- the host planner of the sequence-summary engine
// (seqsum_engine.inc; include/phylo_hip_seqsum.h): one tree, one alignment,
// and per draw the marginal state posterior of every internal node at every
// pattern, every pattern's rate-category posterior and its mean rate.
//
// Plain C++17 like sweep_plan.h, which it builds on: make_problem validates
// the sizes, the data and the peel (phy_create's refusals) and fixes the tip
// record vectors (R, extra, vec_of) and Ppad.  What is planned here:
//   - the forward schedule: the internal nodes, children before parents, each
//     step's children in the peel row's order; the reverse pass walks it
//     backwards (parents before children);
//   - the row layout and the per-draw workspace, every size and offset in 64
//     bits;
//   - the draws per launch, from a fixed budget of device memory (a constant,
//     no environment knob): one draw per launch when a draw alone passes it.
// Nothing here depends on a call: a draw's bits are its own.
// tests/seqsum_plan_check.cpp compiles this file with a host compiler alone.
#ifndef PHYLO_SEQSUM_PLAN_H
#define PHYLO_SEQSUM_PLAN_H

#include "sweep_plan.h"

namespace {

constexpr int SEQ_COLS = WAVE;                            // pattern columns per workgroup: one per lane
constexpr int SEQ_STEP_INTS = 4;                          // child a, child b, node v, unused
constexpr size_t SEQ_BUDGET_BYTES = (size_t)1 << 30;      // per-launch workspace + rows the plan aims to stay within
constexpr int SEQ_MAX_LAUNCH = 32768;                     // draws per launch at most (grid y)

struct SeqsumPlan {
  Problem pb;
  int root = -1, merged = -1;       // node ids; merged: the unrooted tree's matrix-free child of the root, else -1
  int nblk = 0;                     // workgroups per draw (SEQ_COLS columns each)
  std::vector<int> steps;           // [S-1][SEQ_STEP_INTS], forward order
  long long row_len = 0;            // 1 + (4(S-1) + C + 1) P doubles
  long long off_anc = 0, off_cat = 0, off_rate = 0;  // offsets inside a row
  long long node_stride = 0;        // doubles of one node's partials in a draw's workspace: C * 4 * Ppad
  long long ws_draw = 0;            // doubles of a draw's workspace: 2 (S-1) node_stride (part, then q)
  long long draw_bytes = 0;         // device bytes a draw in flight holds: workspace, row, site terms, matrices
  int draws_per_launch = 0;
  size_t lds = 0;                   // dynamic LDS bytes of the summary kernel
};

// Refusals: everything make_problem refuses (PHY_EINVAL), and a row too long
// for the int phy_seqsum_row_len returns.
int seqsum_plan(int S, int P, int C, int rooted, int kind, const uint8_t* tipcodes, const double* weights,
                const int32_t* peel, int max_draws, SeqsumPlan& sp) {
  sp = SeqsumPlan();
  int rc = make_problem(S, P, C, rooted, kind, tipcodes, weights, peel, max_draws, sp.pb);
  if (rc) return rc;
  const Problem& pb = sp.pb;
  PeelTree t;
  if ((rc = parse_peel(S, peel, pb.rooted, t))) return rc;
  sp.root = t.root;
  sp.merged = t.merged;
  // make_problem has checked that the B branches are the nodes 0..B-1: the
  // root (and the merged node) carry no matrix and are the nodes >= B
  if (t.root < pb.B || (t.merged >= 0 && t.merged < pb.B)) return fail(PHY_EINVAL, "internal: the root is a branch");
  // post-order of the internal nodes (children before parents)
  sp.steps.reserve((size_t)(S - 1) * SEQ_STEP_INTS);
  {
    std::vector<std::pair<int, int>> st{{t.root, 0}};
    while (!st.empty()) {
      auto& [n, k] = st.back();
      if (n < S) {
        st.pop_back();
        continue;
      }
      if (k == 2) {
        const int step[SEQ_STEP_INTS] = {t.ch1[n], t.ch2[n], n, 0};
        sp.steps.insert(sp.steps.end(), step, step + SEQ_STEP_INTS);
        st.pop_back();
        continue;
      }
      const int child = (k == 0) ? t.ch1[n] : t.ch2[n];
      ++k;
      st.push_back({child, 0});
    }
  }
  if (sp.steps.size() != (size_t)(S - 1) * SEQ_STEP_INTS) return fail(PHY_EINVAL, "tree is not binary / connected");
  sp.nblk = (P + SEQ_COLS - 1) / SEQ_COLS;
  if ((long long)sp.nblk * SEQ_COLS > pb.Ppad) return fail(PHY_EINVAL, "internal: column blocks pass the padding");
  const long long LP = P, LS1 = S - 1, LC = C;
  sp.off_anc = 1;
  sp.off_cat = 1 + 4 * LS1 * LP;
  sp.off_rate = sp.off_cat + LC * LP;
  sp.row_len = sp.off_rate + LP;
  if (sp.row_len > (long long)INT_MAX) return fail(PHY_EINVAL, "summary row longer than 2^31 - 1 doubles");
  sp.node_stride = LC * 4 * (long long)pb.Ppad;
  sp.ws_draw = 2 * LS1 * sp.node_stride;
  sp.draw_bytes = 8 * (sp.ws_draw + sp.row_len + (long long)pb.Ppad + LC * pb.nmat * pb.R * 4 + EIG_LEN +
                       (10 + 2 * LC) + pb.B);
  // a launch's grid carries the draw in y: never more than SEQ_MAX_LAUNCH of them
  const long long fit = std::min((long long)SEQ_MAX_LAUNCH, (long long)SEQ_BUDGET_BYTES / sp.draw_bytes);
  sp.draws_per_launch = (int)std::max(1LL, std::min((long long)max_draws, fit));
  // the category terms of the root [C][64], then two buffers of a node's terms [C][4][64]
  sp.lds = ((size_t)C * SEQ_COLS + 2 * (size_t)C * 4 * SEQ_COLS) * sizeof(double);
  if (sp.lds > LDS_CAP) return fail(PHY_EINVAL, "internal: summary kernel's LDS passes the cap");
  return PHY_OK;
}

}  // namespace

#endif  // PHYLO_SEQSUM_PLAN_H
