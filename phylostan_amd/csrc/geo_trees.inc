// geo_trees.inc -- the discrete-trait likelihood over a sample of T trees on
// the same tips: the mixture L_mix = sum_t w_t L_t, its gradient with respect
// to rates_geo and freqs_geo, and the posterior summaries that do not depend on
// a topology (expected transitions, dwell times, the root's location).
// Included by phylo_hip.hip after geo_phases.inc and geo_engine.inc.  Its
// kernels run the phases of geo_phases.inc, the same functions geo_draw runs:
// what is stated here is how they are split over three kernels, the record and
// the slots between them, and the fold over trees.
//
// The reference has no counterpart: its --geo model conditions on one tree.
//
//   grad log L_mix = sum_t p_t grad log L_t,  p_t = w_t L_t / L_mix.
// Given a draw's eigensystem the gradient rows are linear in what a tree leaves
// behind -- W_t = sum_b (a_b c_b^T) o Phi, colt - rowt, and for the summaries
// the root row low(root) o up[root] -- so their p_t-weighted sums are formed
// first and sym(V W V^T) and the chain rule run once per draw.  Three phases:
//   1. geo_trees_eig_kernel: one workgroup per draw, geo_params_ok, geo_q_scale
//      and geo_jacobi, their results (ok, sweeps, s, lam, qd, V) to a per-draw
//      record;
//   2. geo_trees_tree_kernel: one workgroup per (draw, group) item.  It loads
//      the record into LDS and walks the group's trees in ascending order:
//      geo_prune, the root sum and geo_reverse on tree t's schedule and branch
//      lengths, then W_t (geo_w_entry), colt - rowt (geo_col_minus_row) and the root
//      row folded into the item's slot as sum_t exp(x_t - m) (.), x_t = log w_t +
//      log L_t, m the running maximum of x_t (the slot is rescaled by exp(m_old -
//      m_new) when it rises).  A tree whose exp(x_t - m) is 0 adds nothing and
//      skips its reverse pass; one without a finite log L_t has tree_ll = -inf
//      and no weight;
//   3. geo_trees_combine_kernel: one workgroup per draw merges the G slots in
//      ascending order (weights exp(m_g - M), M their maximum), forms log L_mix
//      = M + log Z, divides by Z, and runs geo_sym_vwvt and geo_chain_rule.
// The summaries form also folds, beside each slot (dslots), the two orders in t of the dwell times (geo_phases.inc:
// W2_t and their first-order sums), and phase 3 puts diag(V W2 V^T) plus the first order in place of G's diagonal.
// Every sum has one fixed order that depends on the context alone (geo_plan.h:
// G and the split do not depend on n_draws), so a draw's rows are bitwise the
// same alone, in any batch and on repeat.  No atomics.
//
// A trait clock (phy_geo_trees_eval_clock): a draw's rate mu > 0 scales every
// branch of every tree, P_b = exp(Q mu t_b).  Phases 2 and 3 are templates on
// CLOCK, and so are geo_prune and geo_w_entry; the plain calls instantiate CLOCK
// = false.  With CLOCK the item loads mu once, forms t_eff = mu t_tb as one fp64
// product wherever a branch length is read, and phase 3 forms
//   dlogL_mix/dmu = (1/mu) sum_k lam_k Wbar_kk
// from the p_t-weighted, Z-normalised W before W is overwritten: W_kk = sum_b
// a_bk c_bk t_eff e^{lam_k t_eff} and dlogL/dt_eff,b = sum_k a_bk lam_k e^{lam_k
// t_eff} c_bk, so sum_b t_eff,b dlogL/dt_eff,b = sum_k lam_k W_kk.  The slot
// layout does not change.  Dwell times leave as G_ii / mu, in the tree's unit.

struct GeoTreesArgs {
  const double* tips;    // [S][K]
  const int* rows;       // [T][S-1][GR_INTS]
  const int* lvl_off;    // tree t's level starts at lvl_start[t]
  const int* lvl_start;  // [T+1]
  const int* grp_off;    // [G+1]
  const double* blens;   // [T][B]
  const double* logw;    // [T]
  const double* params;  // [n][R+K]
  double* rec;           // [n][rec_doubles]
  double* slots;         // [chunk][G][slot_doubles]
  double* tree_ll;       // [n][T]
  double* out;           // [n][1+R+K], with CLOCK [n][2+R+K]
  double* summ;          // [n][K K + K], the summaries form only
  double* ws;            // [workgroups][ws_stride]
  size_t ws_stride;
  int S, K, T, G, n;
  int draw0, ndraw;  // the chunk of draws phases 2 and 3 run on
  const double* clock;  // [n] mu per draw, read by the CLOCK kernels alone; last, so that no other field moves
  double* dslots;       // [chunk][G][dwell_doubles]; NULL unless the summaries form runs: the tree phase then also
                        // folds the dwell times' two orders (W2, first)
};

// ---- phase 1: the eigensystem of one draw, to the record
__device__ bool geo_trees_eigen(const GeoTreesArgs& a, int draw, double* sh, double* rec) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, R = geo_rate_count(K);
  const GeoView v(sh, K);
  const double* rates = a.params + (size_t)draw * geo_param_len(K);
  const double* freqs = rates + R;
  if (!geo_params_ok(v, rates, freqs, 0.0)) return false;
  for (int i = tid; i < K; i += nt) {
    const double f = freqs[i];
    v.pi[i] = f;
    v.sq[i] = sqrt(f);
  }
  const double s = geo_q_scale(v, rates);
  if (!(s > 0.0) || !isfinite(s)) return false;
  int sweeps;
  const bool converged = geo_jacobi(v, rates, s, sweeps);
  if (tid == 0) rec[GT_SWEEPS] = (double)sweeps, rec[GT_S] = s;
  if (!converged) return false;
  double* rlam = rec + GT_HEAD;
  double* rqd = rlam + K;
  double* rV = rqd + K;
  for (int i = tid; i < K; i += nt) rlam[i] = v.A[i * v.KP + i], rqd[i] = v.qd[i];
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    rV[it] = v.V[i * v.KP + j];
  }
  return true;
}

__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_eig_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  const size_t reclen = geo_trees_rec_doubles(a.K);
  for (int draw = blockIdx.x; draw < a.n; draw += gridDim.x) {
    double* rec = a.rec + (size_t)draw * reclen;
    if (threadIdx.x == 0) rec[GT_SWEEPS] = -1.0, rec[GT_S] = 0.0;
    const bool ok = geo_trees_eigen(a, draw, sh, rec);
    __syncthreads();  // LDS is free for the next draw
    if (threadIdx.x == 0) rec[GT_OK] = ok ? 1.0 : 0.0;
  }
}

// ---- phase 2: one (draw, group) item
template <bool CLOCK>
__device__ void geo_trees_group(const GeoTreesArgs& a, int draw, int g, double* slot, double* dslot, double* sh,
                                double* wsb) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, S = a.S, B = 2 * S - 3;
  const GeoView v(sh, K, wsb, a.tips, S);
  const double* freqs = a.params + (size_t)draw * geo_param_len(K) + geo_rate_count(K);
  const double* rec = a.rec + (size_t)draw * geo_trees_rec_doubles(K);
  const int t0 = a.grp_off[g], t1 = a.grp_off[g + 1];
  double* tll = a.tree_ll + (size_t)draw * a.T;
  __syncthreads();  // the previous item's readers of LDS and of the workspace are done
  double mu = 1.0;  // uniform over the workgroup: one load per item
  if constexpr (CLOCK) mu = a.clock[draw];
  bool dead = rec[GT_OK] == 0.0;
  if constexpr (CLOCK) dead = dead || !(mu > 0.0) || !isfinite(mu);
  if (dead) {  // no eigensystem (or no rate): every tree of the draw is -inf, the slot is empty
    for (int t = t0 + tid; t < t1; t += nt) tll[t] = -INFINITY;
    if (tid == 0) slot[GS_MAX] = -INFINITY, slot[GS_SUM] = 0.0;
    return;
  }
  {
    const double* rlam = rec + GT_HEAD;
    const double* rV = rlam + 2 * K;
    for (int i = tid; i < K; i += nt) {
      const double r = sqrt(freqs[i]);
      v.lam[i] = rlam[i];
      v.sq[i] = r;
      v.isq[i] = 1.0 / r;
    }
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      v.V[i * v.KP + j] = rV[it];
    }
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {  // 1 / (lam_k - lam_l), 0 inside the near window
    const int k = it / K, l = it - k * K;
    v.A[k * v.KP + l] = phi_rinv(v.lam[k], v.lam[l], PHI_NEAR);
  }
  double m = -INFINITY, sumw = 0.0;  // uniform over the workgroup
  double* sW = slot + GS_HEAD;
  double* sv = sW + (size_t)K * K;
  double* sr = sv + K;
  for (int t = t0; t < t1; ++t) {
    const int* rows = a.rows + (size_t)t * (S - 1) * GR_INTS;
    const int* lvl = a.lvl_off + a.lvl_start[t];
    const int nlev = a.lvl_start[t + 1] - a.lvl_start[t] - 1;
    const double* bl = a.blens + (size_t)t * B;
    __syncthreads();  // the previous tree's fold has read the workspace; A is written
    geo_prune<CLOCK>(v, rows, lvl, nlev, bl, mu);
    const double Ls = geo_block_sum(tid < K ? v.LOW[(size_t)v.root * K + tid] : 0.0, v.red, tid, nt);
    double shifts = 0.0;
    for (int node = S + tid; node < 2 * S - 1; node += nt) shifts += v.sexp[node];
    shifts = geo_block_sum(shifts, v.red, tid, nt);  // integers: exact
    const double logL = log(Ls) - shifts * 0.693147180559945309417232121458;
    if (!(Ls > 0.0) || !isfinite(logL)) {  // no likelihood on this tree: no weight
      if (tid == 0) tll[t] = -INFINITY;
      continue;
    }
    if (tid == 0) tll[t] = logL;
    const double x = a.logw[t] + logL;
    const double mn = fmax(m, x);
    const bool first = m == -INFINITY;
    const double ro = first ? 0.0 : exp(m - mn);
    const double rn = exp(x - mn);
    if (rn == 0.0) continue;  // the term underflows against the group's maximum: exactly nothing

    geo_reverse(v, rows, lvl, nlev, Ls);
    // ---- W_t, colt - rowt and the root row, folded into the slot: each entry by one thread, always the same
    for (int it = tid; it < K * K; it += nt) {
      const int k = it / K, l = it - k * K;
      sW[it] = fma(geo_w_entry<CLOCK>(v, k, l, bl, mu), rn, first ? 0.0 : sW[it] * ro);
    }
    for (int i = tid; i < K; i += nt) {
      sv[i] = fma(geo_col_minus_row(v, i), rn, first ? 0.0 : sv[i] * ro);
      sr[i] = fma(v.LOW[(size_t)v.root * K + i] * v.UP[(size_t)v.root * K + i], rn, first ? 0.0 : sr[i] * ro);
    }
    if (dslot) {  // uniform.  The dwell times' two orders in t (geo_phases.inc), folded like W and colt - rowt
      double* sW2 = dslot;
      double* sd = sW2 + (size_t)K * K;
      __syncthreads();  // geo_col_minus_row has read MSG
      geo_dwell_f<CLOCK>(v, bl, mu);
      __syncthreads();
      for (int it = tid; it < K * K; it += nt) {
        const int k = it / K, l = it - k * K;
        sW2[it] = fma(geo_w2_entry<CLOCK>(v, k, l, bl, mu), rn, first ? 0.0 : sW2[it] * ro);
      }
      for (int i = tid; i < K; i += nt)
        sd[i] = fma(geo_dwell_first<CLOCK>(v, i, bl, mu), rn, first ? 0.0 : sd[i] * ro);
    }
    sumw = fma(sumw, ro, rn);
    m = mn;
  }
  if (tid == 0) slot[GS_MAX] = m, slot[GS_SUM] = sumw;
}

template <bool CLOCK>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_tree_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  double* wsb = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const size_t slotlen = geo_trees_slot_doubles(a.K);
  const int items = a.ndraw * a.G;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int dl = item / a.G, g = item - dl * a.G;
    geo_trees_group<CLOCK>(a, a.draw0 + dl, g, a.slots + (size_t)item * slotlen,
                           a.dslots ? a.dslots + (size_t)item * geo_trees_dwell_doubles(a.K) : nullptr, sh, wsb);
  }
}

// ---- phase 3: one draw.  false: the mixture has no finite likelihood.
template <bool SUM, bool CLOCK>
__device__ bool geo_trees_combine(const GeoTreesArgs& a, int draw, const double* slots, double* sh) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, R = geo_rate_count(K), G = a.G;
  const GeoView v(sh, K);
  const int KP = v.KP;
  double* red = v.red;  // first the G merge weights, then reduction scratch
  const double* rates = a.params + (size_t)draw * geo_param_len(K);
  const double* freqs = rates + R;
  const double* rec = a.rec + (size_t)draw * geo_trees_rec_doubles(K);
  const size_t slotlen = geo_trees_slot_doubles(K);
  double* orow = a.out + (size_t)draw * (geo_trees_row_len(K) + (CLOCK ? 1 : 0));
  if (rec[GT_OK] == 0.0) return false;
  double mu = 1.0;
  if constexpr (CLOCK) {
    mu = a.clock[draw];
    if (!(mu > 0.0) || !isfinite(mu)) return false;
  }
  double M = -INFINITY;
  for (int g = 0; g < G; ++g) M = fmax(M, slots[(size_t)g * slotlen + GS_MAX]);
  if (!(M > -INFINITY) || !isfinite(M)) return false;
  for (int g = tid; g < G; g += nt) {
    const double mg = slots[(size_t)g * slotlen + GS_MAX];
    red[g] = mg == -INFINITY ? 0.0 : exp(mg - M);
  }
  __syncthreads();
  double Z = 0.0;
  for (int g = 0; g < G; ++g)
    if (red[g] != 0.0) Z = fma(slots[(size_t)g * slotlen + GS_SUM], red[g], Z);
  const double logL = M + log(Z);
  if (!(Z > 0.0) || !isfinite(logL)) return false;
  const double s = rec[GT_S];
  {
    const double* rqd = rec + GT_HEAD + K;
    const double* rV = rqd + K;
    for (int i = tid; i < K; i += nt) {
      const double f = freqs[i], r = sqrt(f);
      v.pi[i] = f;
      v.sq[i] = r;
      v.isq[i] = 1.0 / r;
      v.qd[i] = rqd[i];
    }
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      v.V[i * KP + j] = rV[it];
    }
  }
  for (int it = tid; it < K * K + 2 * K; it += nt) {  // the G slots in ascending order, then / Z: the posterior mean
    double acc = 0.0;
    for (int g = 0; g < G; ++g) {
      const double sc = red[g];
      if (sc != 0.0) acc = fma(slots[(size_t)g * slotlen + GS_HEAD + it], sc, acc);
    }
    acc /= Z;
    if (it < K * K) {
      const int k = it / K, l = it - k * K;
      v.W[k * KP + l] = acc;
    } else if (it < K * K + K) {
      v.dvec[it - K * K] = acc;
    } else {
      v.rrow[it - K * K - K] = acc;
    }
  }
  __syncthreads();
  if constexpr (CLOCK) {  // dlogL_mix/dmu from the diagonal of W, which geo_sym_vwvt overwrites
    if (tid == 0) {
      const double* rlam = rec + GT_HEAD;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(rlam[k], v.W[k * KP + k], acc);
      orow[1 + R + K] = acc / mu;
    }
  }
  double* srow = nullptr;
  if constexpr (SUM) srow = a.summ + (size_t)draw * geo_trees_summary_len(K);
  geo_sym_vwvt(v, [&](int i, int j, double g) {
    // g = G_ij: E[i -> j transitions] = A_ij G_ij, E[time in i] = G_ii; with CLOCK the tree's lengths are
    // t_eff / mu: the time in i leaves in the tree's unit
    if constexpr (SUM) {
      if constexpr (CLOCK)
        srow[i * K + j] = i == j ? g / mu : geo_a_entry(v, rates, s, i, j) * g;
      else
        srow[i * K + j] = i == j ? g : geo_a_entry(v, rates, s, i, j) * g;
    }
  });
  if constexpr (SUM)
    for (int i = tid; i < K; i += nt) srow[(size_t)K * K + i] = v.rrow[i];
  __syncthreads();
  geo_chain_rule(v, rates, s, orow + 1, orow + 1 + R);
  if constexpr (SUM) {
    // ---- the dwell times: the slots' W2 and first-order sums merged as W was (the weights again: red has been
    // reduction scratch since), W2 over W and the first order over dvec, both spent; they replace G's diagonal
    __syncthreads();  // the chain rule has read W, dvec and red
    const size_t dlen = geo_trees_dwell_doubles(K);
    const double* dslots = a.dslots + (size_t)(draw - a.draw0) * G * dlen;
    for (int g = tid; g < G; g += nt) {
      const double mg = slots[(size_t)g * slotlen + GS_MAX];
      red[g] = mg == -INFINITY ? 0.0 : exp(mg - M);
    }
    __syncthreads();
    for (int it = tid; it < K * K + K; it += nt) {
      double acc = 0.0;
      for (int g = 0; g < G; ++g) {
        const double sc = red[g];
        if (sc != 0.0) acc = fma(dslots[(size_t)g * dlen + it], sc, acc);
      }
      acc /= Z;
      if (it < K * K) {
        const int k = it / K, l = it - k * K;
        v.W[k * KP + l] = acc;
      } else {
        v.dvec[it - K * K] = acc;
      }
    }
    __syncthreads();
    geo_w2_vt(v);
    __syncthreads();
    for (int i = tid; i < K; i += nt) {
      const double d = v.dvec[i] + geo_dwell_second(v, i);
      if constexpr (CLOCK)
        srow[(size_t)i * K + i] = d / mu;
      else
        srow[(size_t)i * K + i] = d;
    }
  }
  if (tid == 0) orow[0] = logL;
  return true;
}

template <bool SUM, bool CLOCK>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_combine_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  const size_t slotlen = geo_trees_slot_doubles(a.K);
  const int rowlen = geo_trees_row_len(a.K) + (CLOCK ? 1 : 0);
  const int slen = geo_trees_summary_len(a.K);
  for (int dl = blockIdx.x; dl < a.ndraw; dl += gridDim.x) {
    const int draw = a.draw0 + dl;
    __syncthreads();  // the previous draw's readers of LDS are done
    const bool ok = geo_trees_combine<SUM, CLOCK>(a, draw, a.slots + (size_t)dl * a.G * slotlen, sh);
    __syncthreads();
    if (!ok) {
      double* orow = a.out + (size_t)draw * rowlen;
      for (int i = threadIdx.x; i < rowlen; i += blockDim.x) orow[i] = i == 0 ? -INFINITY : 0.0;
      double* tll = a.tree_ll + (size_t)draw * a.T;
      for (int t = threadIdx.x; t < a.T; t += blockDim.x) tll[t] = -INFINITY;
      if constexpr (SUM) {
        double* srow = a.summ + (size_t)draw * slen;
        for (int i = threadIdx.x; i < slen; i += blockDim.x) srow[i] = 0.0;
      }
    }
  }
}

struct phy_geo_trees_ctx {
  GeoTreesPlan plan;
  int device = 0, max_draws = 0;
  hipStream_t stream = nullptr;
  double *d_tips = nullptr, *d_blens = nullptr, *d_logw = nullptr, *d_params = nullptr, *d_rec = nullptr;
  double *d_slots = nullptr, *d_tll = nullptr, *d_out = nullptr, *d_ws = nullptr;
  int *d_rows = nullptr, *d_lvl = nullptr, *d_lvs = nullptr, *d_grp = nullptr;
  double* d_summ = nullptr;  // [max_draws][K K + K], allocated by the first phy_geo_trees_eval_summaries
  double* d_dslots = nullptr;  // [chunk_draws][G][dwell_doubles], likewise
  double *d_clock = nullptr, *d_outc = nullptr;  // [max_draws], [max_draws][2+R+K]: the first clock call's
  bool attr_sum = false, attr_clock = false, attr_clock_sum = false;  // kernels whose LDS attribute is set
};

namespace {
void free_geo_trees(phy_geo_trees_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->device);
  for (void* p : {(void*)c->d_tips, (void*)c->d_blens, (void*)c->d_logw, (void*)c->d_params, (void*)c->d_rec,
                  (void*)c->d_slots, (void*)c->d_tll, (void*)c->d_out, (void*)c->d_ws, (void*)c->d_rows,
                  (void*)c->d_lvl, (void*)c->d_lvs, (void*)c->d_grp, (void*)c->d_summ, (void*)c->d_dslots, (void*)c->d_clock,
                  (void*)c->d_outc})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

template <bool SUM, bool CLOCK>
int geo_trees_launch(const GeoTreesPlan& pl, GeoTreesArgs& a, int n_draws, hipStream_t st) {
  hipLaunchKernelGGL(geo_trees_eig_kernel, dim3(std::min(n_draws, pl.draw_workgroups)), dim3(pl.threads),
                     pl.lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  for (int d0 = 0; d0 < n_draws; d0 += pl.chunk_draws) {  // a draw's rows do not depend on the chunk it falls in
    a.draw0 = d0, a.ndraw = std::min(pl.chunk_draws, n_draws - d0);
    const long long items = (long long)a.ndraw * pl.G;
    hipLaunchKernelGGL(geo_trees_tree_kernel<CLOCK>, dim3((int)std::min<long long>(items, pl.workgroups)),
                       dim3(pl.threads), pl.lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
    const dim3 cgrid(std::min(a.ndraw, pl.draw_workgroups));
    hipLaunchKernelGGL((geo_trees_combine_kernel<SUM, CLOCK>), cgrid, dim3(pl.threads), pl.lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PHY_OK;
}

// the three phases of n_draws draws; sum takes the combine phase's summaries form, clock != NULL the CLOCK kernels
// (rows of 2 + R + K)
int geo_trees_run(phy_geo_trees_ctx* ctx, const char* who, int n_draws, const double* params, const double* clock,
                  bool with_clock, double* out, double* tree_ll, double* summaries, bool sum) {
  if (!ctx) return fail(PHY_EINVAL, std::string(who) + ": NULL ctx");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, std::string(who) + ": n_draws out of range");
  if (!params || (sum ? !summaries : !out)) return fail(PHY_EINVAL, std::string(who) + ": NULL host buffer");
  if (with_clock && !clock) return fail(PHY_EINVAL, std::string(who) + ": clock is NULL");
  const GeoTreesPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t slen = (size_t)geo_trees_summary_len(pl.K);
  const size_t rowlen = (size_t)geo_trees_row_len(pl.K) + (with_clock ? 1 : 0);
  // a context that never asks pays for neither the buffers nor the further kernels' attributes
  if (sum && !with_clock && !ctx->attr_sum) {
    HIP_TRY(hipFuncSetAttribute((const void*)geo_trees_combine_kernel<true, false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_sum = true;
  }
  if (with_clock && !ctx->attr_clock) {
    for (const void* f : {(const void*)geo_trees_tree_kernel<true>, (const void*)geo_trees_combine_kernel<false, true>})
      HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_clock = true;
  }
  if (with_clock && sum && !ctx->attr_clock_sum) {
    HIP_TRY(hipFuncSetAttribute((const void*)geo_trees_combine_kernel<true, true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_clock_sum = true;
  }
  if (sum && !ctx->d_summ) {
    const int rc = dalloc(&ctx->d_summ, (size_t)ctx->max_draws * slen);
    if (rc) return rc;
  }
  if (sum && !ctx->d_dslots) {
    const int rc = dalloc(&ctx->d_dslots, (size_t)pl.chunk_draws * pl.G * geo_trees_dwell_doubles(pl.K));
    if (rc) return rc;
  }
  if (with_clock && !ctx->d_clock) {
    const int rc = dalloc(&ctx->d_clock, (size_t)ctx->max_draws);
    if (rc) return rc;
  }
  if (with_clock && !ctx->d_outc) {
    const int rc = dalloc(&ctx->d_outc, (size_t)ctx->max_draws * rowlen);
    if (rc) return rc;
  }
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * geo_param_len(pl.K), hipMemcpyHostToDevice, st));
  if (with_clock) HIP_TRY(hipMemcpyAsync(ctx->d_clock, clock, sizeof(double) * n, hipMemcpyHostToDevice, st));
  GeoTreesArgs a{};
  a.tips = ctx->d_tips, a.rows = ctx->d_rows, a.lvl_off = ctx->d_lvl, a.lvl_start = ctx->d_lvs, a.grp_off = ctx->d_grp;
  a.blens = ctx->d_blens, a.logw = ctx->d_logw, a.params = ctx->d_params, a.rec = ctx->d_rec, a.slots = ctx->d_slots;
  a.clock = with_clock ? ctx->d_clock : nullptr;
  a.tree_ll = ctx->d_tll, a.out = with_clock ? ctx->d_outc : ctx->d_out, a.summ = ctx->d_summ, a.ws = ctx->d_ws;
  a.ws_stride = pl.ws_doubles;
  a.S = pl.S, a.K = pl.K, a.T = pl.T, a.G = pl.G, a.n = n_draws;
  a.dslots = sum ? ctx->d_dslots : nullptr;
  const int rc = with_clock ? (sum ? geo_trees_launch<true, true>(pl, a, n_draws, st)
                                   : geo_trees_launch<false, true>(pl, a, n_draws, st))
                            : (sum ? geo_trees_launch<true, false>(pl, a, n_draws, st)
                                   : geo_trees_launch<false, false>(pl, a, n_draws, st));
  if (rc) return rc;
  if (out) HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(double) * n * rowlen, hipMemcpyDeviceToHost, st));
  if (tree_ll) HIP_TRY(hipMemcpyAsync(tree_ll, ctx->d_tll, sizeof(double) * n * pl.T, hipMemcpyDeviceToHost, st));
  if (sum) HIP_TRY(hipMemcpyAsync(summaries, ctx->d_summ, sizeof(double) * n * slen, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PHY_OK;
}
}  // namespace

extern "C" {

int phy_geo_trees_create(int S, int K, const double* tip_partials, int T, const int32_t* peels, const double* blens,
                         const double* log_weights, int max_draws, int device, phy_geo_trees_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  if (!tip_partials) return fail(PHY_EINVAL, "phy_geo_trees_create: tip_partials is NULL");
  if (!blens) return fail(PHY_EINVAL, "phy_geo_trees_create: blens is NULL");
  GeoTreesPlan made;
  int rc = geo_trees_plan(S, K, T, peels, max_draws, 1, made);  // refusals before any device call
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)S * K; ++i)
    if (!(tip_partials[i] >= 0.0 && tip_partials[i] <= 1.0))
      return fail(PHY_EINVAL, "phy_geo_trees_create: tip partials must lie in [0, 1]");
  const size_t B = (size_t)made.B;
  for (size_t i = 0; i < (size_t)T * B; ++i)
    if (!std::isfinite(blens[i]))
      return fail(PHY_EINVAL, "phy_geo_trees_create: tree " + std::to_string(i / B) + ": branch length " +
                                  std::to_string(i % B) + " is not finite");
  std::vector<double> logw((size_t)T, -std::log((double)T));
  if (log_weights)
    for (int t = 0; t < T; ++t) {
      if (!std::isfinite(log_weights[t]))
        return fail(PHY_EINVAL, "phy_geo_trees_create: tree " + std::to_string(t) + ": log weight is not finite");
      logw[t] = log_weights[t];
    }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  std::unique_ptr<phy_geo_trees_ctx, void (*)(phy_geo_trees_ctx*)> c(new phy_geo_trees_ctx(), free_geo_trees);
  HIP_TRY(hipSetDevice(device));
  c->device = device;
  c->max_draws = max_draws;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  if ((rc = geo_trees_plan(S, K, T, peels, max_draws, cus, c->plan))) return rc;
  const GeoTreesPlan& pl = c->plan;
  for (const void* f : {(const void*)geo_trees_eig_kernel, (const void*)geo_trees_tree_kernel<false>,
                        (const void*)geo_trees_combine_kernel<false, false>})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t nd = (size_t)max_draws;
  const size_t wgs = (size_t)std::min<long long>((long long)pl.chunk_draws * pl.G, pl.workgroups);
  if ((rc = dalloc(&c->d_tips, (size_t)S * K)) || (rc = dalloc(&c->d_rows, pl.rows.size())) ||
      (rc = dalloc(&c->d_lvl, pl.lvl_off.size())) || (rc = dalloc(&c->d_lvs, pl.lvl_start.size())) ||
      (rc = dalloc(&c->d_grp, pl.grp_off.size())) || (rc = dalloc(&c->d_blens, (size_t)T * B)) ||
      (rc = dalloc(&c->d_logw, (size_t)T)) || (rc = dalloc(&c->d_params, nd * geo_param_len(K))) ||
      (rc = dalloc(&c->d_rec, nd * pl.rec_doubles)) ||
      (rc = dalloc(&c->d_slots, (size_t)pl.chunk_draws * pl.G * pl.slot_doubles)) ||
      (rc = dalloc(&c->d_tll, nd * (size_t)T)) || (rc = dalloc(&c->d_out, nd * geo_trees_row_len(K))) ||
      (rc = dalloc(&c->d_ws, wgs * pl.ws_doubles)))
    return rc;
  HIP_TRY(hipMemcpy(c->d_tips, tip_partials, sizeof(double) * S * K, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_blens, blens, sizeof(double) * (size_t)T * B, hipMemcpyHostToDevice));
  if ((rc = upload(c->d_rows, pl.rows)) || (rc = upload(c->d_lvl, pl.lvl_off)) ||
      (rc = upload(c->d_lvs, pl.lvl_start)) || (rc = upload(c->d_grp, pl.grp_off)) || (rc = upload(c->d_logw, logw)))
    return rc;
  *out = c.release();
  return PHY_OK;
}

int phy_geo_trees_destroy(phy_geo_trees_ctx* ctx) {
  free_geo_trees(ctx);
  return PHY_OK;
}

int phy_geo_trees_num_trees(const phy_geo_trees_ctx* ctx) { return ctx ? ctx->plan.T : -1; }

int phy_geo_trees_output_len(const phy_geo_trees_ctx* ctx) { return ctx ? geo_trees_row_len(ctx->plan.K) : -1; }

int phy_geo_trees_summary_len(const phy_geo_trees_ctx* ctx) { return ctx ? geo_trees_summary_len(ctx->plan.K) : -1; }

int phy_geo_trees_eval(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out, double* tree_ll) {
  return geo_trees_run(ctx, "phy_geo_trees_eval", n_draws, params, nullptr, false, out, tree_ll, nullptr, false);
}

int phy_geo_trees_eval_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out,
                                 double* tree_ll, double* summaries) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_summaries", n_draws, params, nullptr, false, out, tree_ll, summaries,
                       true);
}

int phy_geo_trees_clock_output_len(const phy_geo_trees_ctx* ctx) {
  return ctx ? geo_trees_row_len(ctx->plan.K) + 1 : -1;
}

int phy_geo_trees_eval_clock(phy_geo_trees_ctx* ctx, int n_draws, const double* params, const double* clock,
                             double* out, double* tree_ll) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_clock", n_draws, params, clock, true, out, tree_ll, nullptr, false);
}

int phy_geo_trees_eval_clock_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params, const double* clock,
                                       double* out, double* tree_ll, double* summaries) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_clock_summaries", n_draws, params, clock, true, out, tree_ll,
                       summaries, true);
}

int phy_geo_trees_info(const phy_geo_trees_ctx* ctx, int* widest_level, int* max_levels, int* groups, int* threads,
                       int* lds_bytes, int* workgroups) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (widest_level) *widest_level = ctx->plan.widest;
  if (max_levels) *max_levels = ctx->plan.max_nlev;
  if (groups) *groups = ctx->plan.G;
  if (threads) *threads = ctx->plan.threads;
  if (lds_bytes) *lds_bytes = (int)ctx->plan.lds_bytes;
  if (workgroups) *workgroups = ctx->plan.workgroups;
  return PHY_OK;
}

}  // extern "C"
