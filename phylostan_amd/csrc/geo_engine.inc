// geo_engine.inc -- the K-state discrete-trait ("phylogeography") likelihood
// engine: log L and its full gradient of one site of K locations on a fixed
// tree, K from 2 to 64, fp64 throughout.  Included by phylo_hip.hip after
// geo_phases.inc, which states each device phase below once for this engine
// and for geo_trees.inc: geo_draw here is their sequence on one draw, plus what
// only it computes (the branch gradients and, with SUM, the summaries).
//
// It replaces what the reference's --geo model leaves to Stan:
// calculate_p_matrices (generate_script.py:895-950: Q = R diag(pi) normalised,
// the symmetric eigendecomposition of A = D^1/2 Q D^-1/2, one K x K matrix
// product per branch) and the pruning loop (:1085-1096), both differentiated by
// reverse-mode autodiff on every log_prob.
//
// One workgroup evaluates one draw end to end in one launch (workgroups loop
// when there are more draws than workgroups):
//   1. (geo_params_ok, geo_q_scale, geo_jacobi) A in LDS; cyclic
//      Jacobi in the round-robin ordering of the 4 x 4 solver (jacobi4):
//      floor(K/2) disjoint rotations per round, odd K with a bye, until off(A)^2
//      <= 1e-32 |A|^2; GEO_SWEEP_CAP sweeps without that is -inf.
//   2. (geo_prune) pruning in the eigenbasis, P_b never formed:
//      c = V^T (sqrt(pi) v), message = v + (V (em c)) / sqrt(pi), em = expm1(lam
//      t), level by level (geo_plan.h), with power-of-two rescaling after every
//      internal node.  P(t) v is formed as v + (P(t) - I) v because V V^T is the
//      identity to 1e-16 only: 1e-16 / (q t) of a transition probability on a
//      short branch; a zero-length branch passes v through exactly;
//   3. (geo_reverse) the reverse pass: per branch u~ (dlogL / dmessage), a = V^T
//      (u~ / sqrt(pi)), the downward message u~ + sqrt(pi) (V (em a));
//   4. (geo_w_entry, geo_col_minus_row, geo_sym_vwvt, geo_chain_rule) dlogL/dt_b =
//      sum_k a_k lam_k e^{lam_k t} c_k, W = sum_b (a_b c_b^T) o Phi(lam, t_b)
//      with the three-arm rule (phi_rinv / phi_close; the quotient of em), dlogL/dA = sym(V W V^T),
//      and the chain rule to rates_geo and freqs_geo (entries of freqs
//      independent, as grad_freqs of the 4-state rows).
//   5. (geo_draw<true>, phy_geo_eval_summaries) the posterior summaries those
//      leave behind: node marginals low o up, expected transitions A_ij G_ij
//      from G = V W V^T, transitions per branch from M = V^T A_off V, and the
//      dwell times G_ii from their two orders in t (geo_phases.inc: the product
//      keeps 1e-16 of its off-diagonal entries on the diagonal).
// The per-node K-vectors live in a per-workgroup global workspace (GW_*): at
// K = 64 the three matrices leave no LDS for 8 (2S-1) K doubles, and each is
// written once and read a few times by the same CU (its L1 / L2 hold them).

struct GeoArgs {
  const double* tips;    // [S][K]
  const int* rows;       // [S-1][GR_INTS] level order
  const int* lvl_off;    // [nlev+1]
  const double* blens;   // [n][B]
  const double* params;  // [n][R+K]
  double* out;           // [n][1+B+R+K]
  double* ws;            // [workgroups][ws_stride]
  int* sweeps;           // [n] Jacobi sweeps of each draw (-1: refused before the solve)
  size_t ws_stride;
  int S, K, nlev, n;
};

// The summaries form (phy_geo_eval_summaries) writes one more row per draw:
// marg[N][K], jumps[K][K], bjumps[B] (include/phylo_hip_geo.h).
struct GeoSumArgs : GeoArgs {
  double* summ;  // [n][N K + K K + B]
};
template <bool SUM>
using GeoArgsOf = std::conditional_t<SUM, GeoSumArgs, GeoArgs>;

// One draw.  false: the likelihood is not finite (the row is then -inf and zeros).
// SUM adds the posterior summaries from what the gradient leaves behind; every
// line of it is under if constexpr, so geo_draw<false> is the plain evaluation.
template <bool SUM>
__device__ bool geo_draw(const GeoArgsOf<SUM>& a, int draw, double* sh, double* wsb) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, S = a.S, N = 2 * S - 1, B = 2 * S - 3, R = K * (K - 1) / 2;
  const GeoView v(sh, K, wsb, a.tips, S);
  const int KP = v.KP;
  double *A = v.A, *V = v.V, *W = v.W, *lam = v.lam;
  const double* rates = a.params + (size_t)draw * (R + K);
  const double* freqs = rates + R;
  const double* bl = a.blens + (size_t)draw * B;
  double* orow = a.out + (size_t)draw * geo_row_len(S, K);
  const size_t NK = (size_t)N * K;
  double* srow = nullptr;  // this draw's summary row
  if constexpr (SUM) srow = a.summ + (size_t)draw * geo_summary_len(S, K);

  // ---- the parameters: refuse what has no likelihood (a branch length that is not finite among it)
  {
    double bad = 0.0;
    for (int i = tid; i < B; i += nt) bad += isfinite(bl[i]) ? 0.0 : 1.0;
    if (!geo_params_ok(v, rates, freqs, bad)) return false;
  }
  for (int i = tid; i < K; i += nt) {
    const double f = freqs[i], r = sqrt(f);
    v.pi[i] = f;
    v.sq[i] = r;
    v.isq[i] = 1.0 / r;
  }
  const double s = geo_q_scale(v, rates);
  if (!(s > 0.0) || !isfinite(s)) return false;
  int sweeps;
  const bool converged = geo_jacobi(v, rates, s, sweeps);
  if (a.sweeps && tid == 0) a.sweeps[draw] = sweeps;
  if (!converged) return false;
  for (int i = tid; i < K; i += nt) lam[i] = A[i * KP + i];
  __syncthreads();
  // 1 / (lam_k - lam_l), 0 inside the near window (ties included): phi_close takes those
  for (int it = tid; it < K * K; it += nt) {
    const int k = it / K, l = it - k * K;
    A[k * KP + l] = phi_rinv(lam[k], lam[l], PHI_NEAR);
  }
  __syncthreads();

  geo_prune<false>(v, a.rows, a.lvl_off, a.nlev, bl, 1.0);
  const double Ls = geo_block_sum(tid < K ? v.LOW[(size_t)v.root * K + tid] : 0.0, v.red, tid, nt);
  double shifts = 0.0;
  for (int node = S + tid; node < N; node += nt) shifts += v.sexp[node];
  shifts = geo_block_sum(shifts, v.red, tid, nt);  // integers: exact
  const double logL = log(Ls) - shifts * 0.693147180559945309417232121458;
  if (!(Ls > 0.0) || !isfinite(logL)) return false;
  geo_reverse(v, a.rows, a.lvl_off, a.nlev, Ls);
  if constexpr (SUM) {
    // ---- node marginals: low(n) o up[n] sums to 1 by multilinearity of L, the 2^shift of n cancelling (up[n] is
    // the derivative with respect to the scaled partial); the merged root child carries the root's row
    for (int it = tid; it < N * K; it += nt) {
      const int node = it / K, i = it - node * K, src = node == v.root - 1 ? v.root : node;
      srow[it] = v.low(src)[i] * v.UP[(size_t)src * K + i];
    }
  }

  // ---- branch gradients, W, and the direct D^{+-1/2} terms of P
  for (int b = tid; b < B; b += nt) {
    const double *aa = v.AA + (size_t)b * K, *e = v.EE + (size_t)b * K, *c = v.CC + (size_t)b * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = fma(aa[k] * lam[k], e[k] * c[k], acc);
    orow[1 + b] = acc;
  }
  for (int it = tid; it < K * K; it += nt) {
    const int k = it / K, l = it - k * K;
    W[k * KP + l] = geo_w_entry<false>(v, k, l, bl, 1.0);
  }
  for (int i = tid; i < K; i += nt) v.dvec[i] = geo_col_minus_row(v, i);
  __syncthreads();
  geo_sym_vwvt(v, [&](int i, int j, double g) {
    // g = G_ij, G = V W V^T = dlogL/dA entry by entry: E[i -> j transitions] = A_ij G_ij, E[time in i] = G_ii
    // (Minin & Suchard 2008; A_ij G_ij = Q_ij dlogL/dQ_ij)
    if constexpr (SUM) srow[NK + i * K + j] = i == j ? g : geo_a_entry(v, rates, s, i, j) * g;
  });
  __syncthreads();
  geo_chain_rule(v, rates, s, orow + 1 + B, orow + 1 + B + R);
  if constexpr (SUM) {
    // ---- transitions per branch: n_b = sum_kl a_bk c_bl Phi_kl(t_b) M_kl, M = V^T A_off V.  V^T A V = diag(lam),
    // so M = diag(lam) - V^T diag(A) V: one K^3 product.  A and W are both spent: 1 / (lam_k - lam_l) again over
    // A, M over W
    __syncthreads();  // the chain rule has read W
    for (int it = tid; it < K * K; it += nt) {
      const int k = it / K, l = it - k * K;
      double acc = 0.0;
      for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k] * V[i * KP + l], v.qd[i], acc);
      A[k * KP + l] = phi_rinv(lam[k], lam[l], PHI_NEAR);
      W[k * KP + l] = (k == l ? lam[k] : 0.0) - acc / s;
    }
    __syncthreads();
    double* bj = srow + NK + (size_t)K * K;
    const int wave = tid >> 6, lane = tid & 63, nwaves = nt >> 6;
    for (int b = wave; b < B; b += nwaves) {  // one wave per branch, its K^2 terms in a fixed order
      const double *aa = v.AA + (size_t)b * K, *e = v.EE + (size_t)b * K, *c = v.CC + (size_t)b * K;
      const double* em = v.EM + (size_t)b * K;
      const double t = bl[b];
      double acc = 0.0;
      for (int it = lane; it < K * K; it += 64) {
        const int k = it / K, l = it - k * K;
        const double ri = A[k * KP + l], Ek = e[k], El = e[l];
        const double phi = ri == 0.0 ? phi_close(lam[k], lam[l], t, Ek, El) : (em[k] - em[l]) * ri;
        acc = fma(aa[k] * c[l] * phi, W[k * KP + l], acc);
      }
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) bj[b] = acc;
    }
    // ---- the dwell times from their two orders in t (geo_phases.inc): F over MSG, W2 over W (M is spent once the
    // branches are done), W2 V^T over A (the table is spent once W2 is formed); they replace G's diagonal
    geo_dwell_f<false>(v, bl, 1.0);
    __syncthreads();
    for (int it = tid; it < K * K; it += nt) {
      const int k = it / K, l = it - k * K;
      W[k * KP + l] = geo_w2_entry<false>(v, k, l, bl, 1.0);
    }
    __syncthreads();
    geo_w2_vt(v);
    __syncthreads();
    for (int i = tid; i < K; i += nt)
      srow[NK + (size_t)i * K + i] = geo_dwell_first<false>(v, i, bl, 1.0) + geo_dwell_second(v, i);
  }
  if (tid == 0) orow[0] = logL;
  return true;
}

template <bool SUM>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_kernel(GeoArgsOf<SUM> a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  double* wsb = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const int rowlen = geo_row_len(a.S, a.K);
  for (int draw = blockIdx.x; draw < a.n; draw += gridDim.x) {
    if (a.sweeps && threadIdx.x == 0) a.sweeps[draw] = -1;
    const bool ok = geo_draw<SUM>(a, draw, sh, wsb);
    __syncthreads();  // the row's writers are done; LDS and the workspace are free for the next draw
    if (!ok) {
      double* orow = a.out + (size_t)draw * rowlen;
      for (int i = threadIdx.x; i < rowlen; i += blockDim.x) orow[i] = i == 0 ? -INFINITY : 0.0;
      if constexpr (SUM) {
        const int slen = geo_summary_len(a.S, a.K);
        double* srow = a.summ + (size_t)draw * slen;
        for (int i = threadIdx.x; i < slen; i += blockDim.x) srow[i] = 0.0;
      }
    }
  }
}

struct phy_geo_ctx {
  GeoPlan plan;
  int device = 0, max_draws = 0;
  hipStream_t stream = nullptr;
  double *d_tips = nullptr, *d_blens = nullptr, *d_params = nullptr, *d_out = nullptr, *d_ws = nullptr;
  int *d_rows = nullptr, *d_lvl = nullptr, *d_sweeps = nullptr;
  double* d_summ = nullptr;  // [max_draws][summary_len], allocated by the first phy_geo_eval_summaries
  int last_n = 0;
};

namespace {
void free_geo(phy_geo_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->device);
  for (void* p : {(void*)c->d_tips, (void*)c->d_blens, (void*)c->d_params, (void*)c->d_out, (void*)c->d_ws,
                  (void*)c->d_rows, (void*)c->d_lvl, (void*)c->d_sweeps, (void*)c->d_summ})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// one launch on n_draws draws; sum takes the summaries form (geo_kernel<true>, out optional)
int geo_run(phy_geo_ctx* ctx, const char* who, int n_draws, const double* blens, const double* params, double* out,
            double* summaries, bool sum) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, std::string(who) + ": n_draws out of range");
  if (!blens || !params || (sum ? !summaries : !out)) return fail(PHY_EINVAL, "NULL host buffer");
  const GeoPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t slen = (size_t)geo_summary_len(pl.S, pl.K);
  if (sum && !ctx->d_summ) {  // a context that never asks pays for neither the buffer nor the second kernel's attribute
    HIP_TRY(hipFuncSetAttribute((const void*)geo_kernel<true>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                (int)GEO_LDS_CAP));
    const int rc = dalloc(&ctx->d_summ, (size_t)ctx->max_draws * slen);
    if (rc) return rc;
  }
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_blens, blens, sizeof(double) * n * pl.B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * geo_param_len(pl.K), hipMemcpyHostToDevice, st));
  GeoSumArgs a{};
  a.tips = ctx->d_tips, a.rows = ctx->d_rows, a.lvl_off = ctx->d_lvl;
  a.blens = ctx->d_blens, a.params = ctx->d_params, a.out = ctx->d_out, a.ws = ctx->d_ws, a.sweeps = ctx->d_sweeps;
  a.ws_stride = pl.ws_doubles, a.S = pl.S, a.K = pl.K, a.nlev = pl.nlev, a.n = n_draws;
  a.summ = ctx->d_summ;
  const int grid = std::min(n_draws, pl.workgroups);
  if (sum)
    hipLaunchKernelGGL(geo_kernel<true>, dim3(grid), dim3(pl.threads), pl.lds_bytes, st, a);
  else
    hipLaunchKernelGGL(geo_kernel<false>, dim3(grid), dim3(pl.threads), pl.lds_bytes, st, static_cast<GeoArgs&>(a));
  HIP_TRY(hipGetLastError());
  if (out)
    HIP_TRY(hipMemcpyAsync(out, ctx->d_out, sizeof(double) * n * geo_row_len(pl.S, pl.K), hipMemcpyDeviceToHost, st));
  if (sum) HIP_TRY(hipMemcpyAsync(summaries, ctx->d_summ, sizeof(double) * n * slen, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->last_n = n_draws;
  return PHY_OK;
}
}  // namespace

extern "C" {

int phy_geo_create(int S, int K, const double* tip_partials, const int32_t* peel, int max_draws, int device,
                   phy_geo_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  if (!tip_partials) return fail(PHY_EINVAL, "phy_geo_create: tip_partials is NULL");
  int ndev = 0;
  GeoPlan made;
  int rc = geo_plan(S, K, peel, max_draws, 1, made);  // refusals before any device call
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)S * K; ++i)
    if (!(tip_partials[i] >= 0.0 && tip_partials[i] <= 1.0))
      return fail(PHY_EINVAL, "phy_geo_create: tip partials must lie in [0, 1]");
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  std::unique_ptr<phy_geo_ctx, void (*)(phy_geo_ctx*)> c(new phy_geo_ctx(), free_geo);
  HIP_TRY(hipSetDevice(device));
  c->device = device;
  c->max_draws = max_draws;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  if ((rc = geo_plan(S, K, peel, max_draws, cus, c->plan))) return rc;
  const GeoPlan& pl = c->plan;
  HIP_TRY(hipFuncSetAttribute((const void*)geo_kernel<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t nd = (size_t)max_draws;
  if ((rc = dalloc(&c->d_tips, (size_t)S * K)) || (rc = dalloc(&c->d_rows, pl.rows.size())) ||
      (rc = dalloc(&c->d_lvl, pl.lvl_off.size())) || (rc = dalloc(&c->d_blens, nd * pl.B)) ||
      (rc = dalloc(&c->d_params, nd * geo_param_len(K))) || (rc = dalloc(&c->d_out, nd * geo_row_len(S, K))) ||
      (rc = dalloc(&c->d_ws, (size_t)pl.workgroups * pl.ws_doubles)) || (rc = dalloc(&c->d_sweeps, nd)))
    return rc;
  HIP_TRY(hipMemcpy(c->d_tips, tip_partials, sizeof(double) * S * K, hipMemcpyHostToDevice));
  if ((rc = upload(c->d_rows, pl.rows)) || (rc = upload(c->d_lvl, pl.lvl_off))) return rc;
  *out = c.release();
  return PHY_OK;
}

int phy_geo_destroy(phy_geo_ctx* ctx) {
  free_geo(ctx);
  return PHY_OK;
}

int phy_geo_num_branches(const phy_geo_ctx* ctx) { return ctx ? ctx->plan.B : -1; }

int phy_geo_output_len(const phy_geo_ctx* ctx) { return ctx ? geo_row_len(ctx->plan.S, ctx->plan.K) : -1; }

int phy_geo_eval(phy_geo_ctx* ctx, int n_draws, const double* blens, const double* params, double* out) {
  return geo_run(ctx, "phy_geo_eval", n_draws, blens, params, out, nullptr, false);
}

int phy_geo_summary_len(const phy_geo_ctx* ctx) { return ctx ? geo_summary_len(ctx->plan.S, ctx->plan.K) : -1; }

int phy_geo_eval_summaries(phy_geo_ctx* ctx, int n_draws, const double* blens, const double* params, double* out,
                           double* summaries) {
  return geo_run(ctx, "phy_geo_eval_summaries", n_draws, blens, params, out, summaries, true);
}

int phy_geo_info(const phy_geo_ctx* ctx, int* levels, int* widest_level, int* lds_bytes, int* threads,
                 int* workgroups) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (levels) *levels = ctx->plan.nlev;
  if (widest_level) *widest_level = ctx->plan.widest;
  if (lds_bytes) *lds_bytes = (int)ctx->plan.lds_bytes;
  if (threads) *threads = ctx->plan.threads;
  if (workgroups) *workgroups = ctx->plan.workgroups;
  return PHY_OK;
}

int phy_geo_sweeps(phy_geo_ctx* ctx, int n_draws, int* sweeps) {
  if (!ctx || !sweeps) return fail(PHY_EINVAL, "NULL argument");
  if (n_draws < 1 || n_draws > ctx->last_n) return fail(PHY_ERANGE, "phy_geo_sweeps: more draws than the last phy_geo_eval");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpy(sweeps, ctx->d_sweeps, sizeof(int) * n_draws, hipMemcpyDeviceToHost));
  return PHY_OK;
}

}  // extern "C"
