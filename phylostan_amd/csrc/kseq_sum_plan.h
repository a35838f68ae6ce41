// kseq_sum_plan.h -- the host planner of the K-state engine's posterior
// summaries (kseq_sum.inc): the state posteriors of the internal nodes and the
// expected labelled substitution counts per branch.  A summary context is a
// mixture context (kseq_plan.h makes its plan and its refusals) plus 1..4
// labellings of the unordered state pairs; this file checks the labels and
// sizes every buffer the summaries add: the per-draw B_l tables, the items'
// count slots, the chunk's node posteriors, the running sum and the outputs.
// The kernels take every offset from the PHY_HD helpers below.
//
// Plain C++17, no HIP header: phylo_hip.hip includes it after kseq_plan.h;
// tests/kseq_sum_plan_check.cpp compiles it with a host compiler alone, under
// the address and undefined-behaviour sanitizers.
#ifndef PHYLO_KSEQ_SUM_PLAN_H
#define PHYLO_KSEQ_SUM_PLAN_H

#include "kseq_plan.h"

namespace {

constexpr int KSEQ_SUM_LMAX = 4;          // labellings of one context
constexpr int KSEQ_SUM_FOLD_THREADS = 256;

// B_l of a (draw, component, label): [KT][KT], zero on the padding
PHY_HD inline size_t kseq_sum_blab_doubles(int KT) { return (size_t)KT * KT; }
PHY_HD inline size_t kseq_sum_blab_at(int draw, int m, int l, int M, int NL, int KT) {
  return (((size_t)draw * M + m) * NL + l) * kseq_sum_blab_doubles(KT);
}
// the item's count slot: [NL][B], padded to an even count
PHY_HD inline size_t kseq_sum_slot_doubles(int NL, int B) { return ((size_t)NL * B + 1) & ~(size_t)1; }
PHY_HD inline size_t kseq_sum_slot_at(int l, int b, int B) { return (size_t)l * B + b; }
// a draw's node posteriors: [S-1][K][P], node v at v - S
PHY_HD inline size_t kseq_sum_np_row(int S, int K, int P) { return (size_t)(S - 1) * K * (size_t)P; }
// a draw's counts: [NL][B]
PHY_HD inline size_t kseq_sum_bc_row(int NL, int B) { return (size_t)NL * B; }
// the blab kernel's LDS, in doubles: V, A o lab and (A o lab) V, each K x K with rows K + 1 apart
PHY_HD inline int kseq_sum_blab_kp(int K) { return K + 1; }
PHY_HD inline size_t kseq_sum_blab_lds(int K) { return 3 * (size_t)K * kseq_sum_blab_kp(K); }

struct KseqSumPlan {
  int NL = 0;
  int blab_threads = 0, blab_workgroups = 0;  // one (draw, component, label) per workgroup
  int fold_workgroups = 0, count_workgroups = 0;
  size_t lds_blab = 0;                    // bytes
  size_t np_row = 0, bc_row = 0, slot_doubles = 0;
  // device buffers, in elements
  size_t n_labels = 0;                    // [NL][R]
  size_t n_blab = 0;                      // [max_draws][M][NL][KT][KT]
  size_t n_sslots = 0;                    // [chunk_draws][items_per_draw][slot_doubles]
  size_t n_npost = 0;                     // [chunk_draws][np_row]
  size_t n_npsum = 0;                     // [np_row]
  size_t n_bcounts = 0;                   // [max_draws][NL][B]
  size_t n_loglik = 0;                    // [max_draws]
};

// the labels alone: what phy_kseq_sum_create refuses of them, before any device call
int kseq_sum_check_labels(int K, int n_labels, const double* labels, const std::string& who) {
  if (n_labels < 1 || n_labels > KSEQ_SUM_LMAX)
    return fail(PHY_EINVAL, who + "n_labels = " + std::to_string(n_labels) + ", supported 1..4");
  if (!labels) return fail(PHY_EINVAL, who + "labels is NULL");
  const size_t R = (size_t)kseq_rate_count(K);
  for (size_t i = 0; i < (size_t)n_labels * R; ++i)
    if (!(labels[i] >= 0.0) || !std::isfinite(labels[i]))
      return fail(PHY_EINVAL, who + "labels[" + std::to_string(i / R) + "][" + std::to_string(i % R) +
                                  "] is negative or not finite");
  return PHY_OK;
}

// base: the mixture plan of the same arguments
int kseq_sum_plan(const KseqPlan& base, int n_labels, const double* labels, int cu_count, KseqSumPlan& out,
                  const std::string& who = "phy_kseq_sum_create: ") {
  const int rc = kseq_sum_check_labels(base.K, n_labels, labels, who);
  if (rc) return rc;
  out = KseqSumPlan();
  out.NL = n_labels;
  size_t np = 0;
  if (!kseq_mul((size_t)(base.S - 1), (size_t)base.K, np) || !kseq_mul(np, (size_t)base.P, np) ||
      np > (size_t)std::numeric_limits<int32_t>::max())
    return fail(PHY_EINVAL, who + "a node_post row of (S-1) K P doubles exceeds 2^31 - 1");
  out.np_row = np;
  out.bc_row = kseq_sum_bc_row(n_labels, base.B);
  out.slot_doubles = kseq_sum_slot_doubles(n_labels, base.B);
  out.lds_blab = kseq_sum_blab_lds(base.K) * sizeof(double);
  if (out.lds_blab > KSEQ_LDS_CAP) return fail(PHY_EINVAL, who + "LDS plan exceeds 160 KiB");
  out.blab_threads = base.draw_threads;
  const size_t nd = (size_t)base.max_draws, ch = (size_t)base.chunk_draws, cus = (size_t)std::max(cu_count, 1);
  size_t chunk_items = 0, per_draw = 0, bytes = 0;
  bool ok = kseq_mul(ch, (size_t)base.items_per_draw, chunk_items);
  ok = ok && kseq_mul((size_t)n_labels, (size_t)base.R, out.n_labels);
  ok = ok && kseq_mul((size_t)base.M * n_labels, kseq_sum_blab_doubles(base.KT), per_draw) &&
       kseq_mul(nd, per_draw, out.n_blab);
  ok = ok && kseq_mul(chunk_items, out.slot_doubles, out.n_sslots) && kseq_mul(ch, out.np_row, out.n_npost) &&
       kseq_mul(nd, out.bc_row, out.n_bcounts);
  out.n_npsum = out.np_row, out.n_loglik = nd;
  for (size_t n : {out.n_blab, out.n_sslots, out.n_npost, out.n_bcounts}) ok = ok && kseq_mul(n, sizeof(double), bytes);
  if (!ok) return fail(PHY_EINVAL, who + "a buffer size overflows (max_draws = " + std::to_string(base.max_draws) + ")");
  out.blab_workgroups = (int)std::min<size_t>(cus, nd * (size_t)base.M * n_labels);
  out.fold_workgroups =
      (int)std::min<size_t>(4 * cus, (out.np_row + KSEQ_SUM_FOLD_THREADS - 1) / KSEQ_SUM_FOLD_THREADS);
  out.count_workgroups = (int)std::min<size_t>(cus, nd);
  return PHY_OK;
}

}  // namespace
#endif  // PHYLO_KSEQ_SUM_PLAN_H
