// kseq_sum.inc -- posterior summaries of the K-state sequence likelihood (kseq_engine.inc): per draw the state
// posteriors of the internal nodes, node_post [S-1][K][P], and the expected number of labelled substitutions on
// each branch, bcounts [NL][B], for 1 <= NL <= 4 symmetric labellings of the state pairs (codon models:
// synonymous and nonsynonymous).  Included by phylo_hip.hip after kseq_engine.inc; phylostan_amd/kseq.py's
// kseq_sum_host is the same derivation in numpy; the planner is kseq_sum_plan.h.  All fp64, no atomics.
//
// The eigen, way-up and site phases are kseq_engine.inc's kernels on the same KseqArgs, so log L carries the
// bits of phy_kseq_mix_eval's row[0].  Per call then
//   a. kseq_sum_blab_kernel, one workgroup per (draw, component, label): B_l = V^T (A o lab_l) V from the eigen
//      record, A = D^1/2 Q D^-1/2, [KT][KT] with zero padding.  <(a c^T) o Phi(lam, t), B_l> is the column's
//      expected count on a branch: int_0^t P(s) (Q o lab) P(t - s) ds in the eigenbasis, the derivative of the
//      branch's exp((Q + eps Q o lab) t) at eps = 0, of which d/dblens is the case lab = 1 with the diagonal.
// and per chunk, after the way up and the site phase,
//   b. kseq_sum_down_kernel: kseq_down_item<true>, which leaves the items' posterior shares in their CC blocks
//      and their counts in the count slots.  It reads B_l from global memory, once per branch: the tables of one
//      (draw, component) are 64 KB at K = 61 and two labels and stay in L2, where a lane's share of four labels in
//      registers (64 doubles beside the products' operands) or a second KT x (KT + 1) table in LDS (only one
//      fits, so at most one label) would each fix NL below 4;
//   c. kseq_sum_counts_kernel, one workgroup per draw: bcounts over g ascending, tile innermost; log L;
//   d. kseq_sum_fold_kernel, one thread per entry of node_post: the shares over g in ascending order, into the
//      draw's row (eval) or, looping over the chunk's draws in draw order, onto the running sum (add).
// A refused draw gives -inf and zeros and takes no part in the sum.  Every sum has one order that depends on
// the shape alone: a draw's outputs are bitwise the same alone, in any batch, in any chunk and on repeat, and the
// running sum is the left-to-right fp64 sum of the finite draws' rows however they are split into calls.

__global__ void __launch_bounds__(GEO_MAX_THREADS)
    kseq_sum_blab_kernel(KseqArgs a, const double* labels, double* blab, int NL) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  const int tid = threadIdx.x, nt = blockDim.x, K = a.K, KT = a.KT, KP = kseq_sum_blab_kp(K), R = kseq_rate_count(K);
  double *Vs = shm, *As = shm + (size_t)K * KP, *Ts = shm + 2 * (size_t)K * KP;
  for (int it0 = blockIdx.x; it0 < a.n * a.M * NL; it0 += gridDim.x) {
    const int dm = it0 / NL, lab = it0 - dm * NL, draw = dm / a.M, m = dm - draw * a.M;
    const double* rec = a.rec + kseq_rec_at(draw, m, a.M, K);
    double* out = blab + kseq_sum_blab_at(draw, m, lab, a.M, NL, KT);
    __syncthreads();  // the previous table's readers of LDS are done
    if (rec[KREC_OK] == 0.0) {  // no eigensystem: the way down skips the draw
      for (int it = tid; it < KT * KT; it += nt) out[it] = 0.0;
      continue;
    }
    const double* rates = a.params + (size_t)draw * kseq_mix_param_len(K, a.M, a.C) + kseq_mix_par_comp(K, m);
    const double* lb = labels + (size_t)lab * R;
    const double* sq = rec + kseq_rec_sq(K);
    const double* rV = rec + kseq_rec_v(K);
    const double s = rec[KREC_S];
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      Vs[i * KP + j] = rV[it];
      double x = 0.0;
      if (i != j) {
        const int at = geo_rate_index(K, i, j);
        x = (sq[i] * sq[j]) * rates[at] / s * lb[at];  // geo_a_entry's A_ij, labelled
      }
      As[i * KP + j] = x;
    }
    __syncthreads();
    for (int it = tid; it < K * K; it += nt) {  // T = (A o lab) V
      const int i = it / K, k = it - i * K;
      double acc = 0.0;
      for (int j = 0; j < K; ++j) acc = fma(As[i * KP + j], Vs[j * KP + k], acc);
      Ts[i * KP + k] = acc;
    }
    __syncthreads();
    for (int it = tid; it < KT * KT; it += nt) {  // B = V^T T
      const int k = it / KT, l = it - k * KT;
      double acc = 0.0;
      if (k < K && l < K)
        for (int i = 0; i < K; ++i) acc = fma(Vs[i * KP + k], Ts[i * KP + l], acc);
      out[it] = acc;
    }
  }
}

__global__ void __launch_bounds__(256) kseq_sum_down_kernel(KseqArgs a, const double* blab, double* sslots, int NL) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  const size_t wslen = kseq_ws_doubles(a.N, a.KT), slotlen = kseq_sum_slot_doubles(NL, a.B);
  const int per_draw = a.G * a.ntiles, items = a.ndraw * per_draw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int dl = item / per_draw, rem = item - dl * per_draw, gc = rem / a.ntiles, tile = rem - gc * a.ntiles;
    const size_t at = kseq_item(dl, gc, tile, a.G, a.ntiles);
    kseq_down_item<true>(a, dl, gc, tile, shm, a.ws + at * wslen, sslots + at * slotlen,
                         blab + kseq_sum_blab_at(a.draw0 + dl, gc / a.C, 0, a.M, NL, a.KT), NL);
  }
}

// the draw has a likelihood: every eigensystem and the site phase's verdict (uniform)
__device__ __forceinline__ bool kseq_sum_good(const KseqArgs& a, int draw) {
  return kseq_draw_ok(a, draw) && a.rec[kseq_rec_at(draw, 0, a.M, a.K) + KREC_BAD] == 0.0;
}

__global__ void __launch_bounds__(KSEQ_SUM_FOLD_THREADS)
    kseq_sum_counts_kernel(KseqArgs a, const double* sslots, double* bcounts, double* loglik, int NL) {
  const size_t slotlen = kseq_sum_slot_doubles(NL, a.B);
  for (int dl = blockIdx.x; dl < a.ndraw; dl += gridDim.x) {
    const int draw = a.draw0 + dl;
    const bool good = kseq_sum_good(a, draw);
    double* out = bcounts + (size_t)draw * kseq_sum_bc_row(NL, a.B);
    const double* slots0 = sslots + kseq_item(dl, 0, 0, a.G, a.ntiles) * slotlen;
    for (int it = threadIdx.x; it < NL * a.B; it += blockDim.x) {  // it = lab B + b, the slot's own order
      double acc = 0.0;
      if (good)
        for (int c = 0; c < a.G; ++c)
          for (int tl = 0; tl < a.ntiles; ++tl) acc += slots0[(size_t)(c * a.ntiles + tl) * slotlen + it];
      out[it] = acc;
    }
    if (threadIdx.x == 0) loglik[draw] = good ? a.rec[kseq_rec_at(draw, 0, a.M, a.K) + KREC_LL] : -INFINITY;
  }
}

// npost: the chunk's rows [ndraw][np_row], or nullptr; npsum: the running sum [np_row], or nullptr
__global__ void __launch_bounds__(KSEQ_SUM_FOLD_THREADS) kseq_sum_fold_kernel(KseqArgs a, double* npost, double* npsum) {
  const size_t wslen = kseq_ws_doubles(a.N, a.KT), blk = kseq_blk(a.KT), cc = kseq_ws_cc(a.N, a.KT);
  const size_t row = kseq_sum_np_row(a.S, a.K, a.P), KP = (size_t)a.K * a.P;
  for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < row; e += (size_t)gridDim.x * blockDim.x) {
    const int v = (int)(e / KP), j = (int)((e - v * KP) / a.P), i = (int)(e - v * KP - (size_t)j * a.P);
    const int tile = i / KSEQ_PT, col = i - tile * KSEQ_PT;
    const size_t in = cc + (size_t)(a.S + v) * blk + (size_t)j * KSEQ_PT + col;
    double sum = npsum ? npsum[e] : 0.0;
    for (int dl = 0; dl < a.ndraw; ++dl) {
      const bool good = kseq_sum_good(a, a.draw0 + dl);
      double x = 0.0;
      if (good)
        for (int g = 0; g < a.G; ++g) x += a.ws[kseq_item(dl, g, tile, a.G, a.ntiles) * wslen + in];
      if (npost) npost[(size_t)dl * row + e] = x;
      if (good) sum += x;
    }
    if (npsum) npsum[e] = sum;
  }
}

struct phy_kseq_sum_ctx {
  phy_kseq_ctx* base = nullptr;
  KseqSumPlan sp;
  double *d_labels = nullptr, *d_blab = nullptr, *d_sslots = nullptr, *d_npost = nullptr, *d_npsum = nullptr;
  double *d_bcounts = nullptr, *d_loglik = nullptr;
  long long n_finite = 0;
};

namespace {
void free_kseq_sum(phy_kseq_sum_ctx* c) {
  if (!c) return;
  if (c->base) {
    DeviceGuard on(c->base->device);
    for (void* p : {(void*)c->d_labels, (void*)c->d_blab, (void*)c->d_sslots, (void*)c->d_npost, (void*)c->d_npsum,
                    (void*)c->d_bcounts, (void*)c->d_loglik})
      if (p) (void)hipFree(p);
  }
  free_kseq(c->base);
  delete c;
}

// n <= max_draws draws on the stream.  node_post: the host's [n][np_row] (eval) or nullptr; sum: onto the running sum.
int kseq_sum_launch(phy_kseq_sum_ctx* c, int n_draws, const double* blens, const double* params, double* loglik,
                    double* bcounts, double* node_post, bool sum) {
  phy_kseq_ctx* ctx = c->base;
  const KseqPlan& pl = ctx->plan;
  const KseqSumPlan& sp = c->sp;
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_blens, blens, sizeof(double) * n * pl.B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * pl.param_len, hipMemcpyHostToDevice, st));
  KseqArgs a{};
  a.masks = ctx->d_masks, a.tile_w = ctx->d_tile_w, a.rows = ctx->d_rows, a.blens = ctx->d_blens;
  a.params = ctx->d_params, a.rec = ctx->d_rec, a.ws = ctx->d_ws, a.slots = ctx->d_slots, a.lc = ctx->d_lc;
  a.sh = ctx->d_sh, a.down0 = ctx->d_down0, a.out = ctx->d_out, a.site = ctx->d_site;
  a.cpost = nullptr;
  a.S = pl.S, a.P = pl.P, a.K = pl.K, a.M = pl.M, a.C = pl.C, a.G = pl.G, a.B = pl.B, a.N = pl.N, a.KT = pl.KT;
  a.NB = pl.NB, a.ntiles = pl.ntiles, a.PP = pl.PP, a.n = n_draws;
  hipLaunchKernelGGL(kseq_eig_kernel, dim3(std::min(n_draws * pl.M, pl.comp_workgroups)), dim3(pl.draw_threads),
                     pl.lds_draw, st, a);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(kseq_sum_blab_kernel, dim3(std::min(n_draws * pl.M * sp.NL, sp.blab_workgroups)),
                     dim3(sp.blab_threads), sp.lds_blab, st, a, (const double*)c->d_labels, c->d_blab, sp.NL);
  HIP_TRY(hipGetLastError());
  const bool rows = node_post != nullptr;
  for (int d0 = 0; d0 < n_draws; d0 += pl.chunk_draws) {
    a.draw0 = d0, a.ndraw = std::min(pl.chunk_draws, n_draws - d0);
    const long long items = (long long)a.ndraw * pl.items_per_draw;
    const dim3 igrid((int)std::min<long long>(items, pl.workgroups)), dgrid(std::min(a.ndraw, pl.draw_workgroups));
    hipLaunchKernelGGL(kseq_up_kernel, igrid, dim3(pl.threads), pl.lds_up, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_site_kernel, dgrid, dim3(pl.site_threads), pl.lds_draw, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_sum_down_kernel, igrid, dim3(pl.threads), pl.lds_down, st, a, (const double*)c->d_blab,
                       c->d_sslots, sp.NL);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_sum_counts_kernel, dim3(std::min(a.ndraw, sp.count_workgroups)),
                       dim3(KSEQ_SUM_FOLD_THREADS), 0, st, a, (const double*)c->d_sslots, c->d_bcounts, c->d_loglik,
                       sp.NL);
    HIP_TRY(hipGetLastError());
    if (rows || sum) {
      hipLaunchKernelGGL(kseq_sum_fold_kernel, dim3(sp.fold_workgroups), dim3(KSEQ_SUM_FOLD_THREADS), 0, st, a,
                         rows ? c->d_npost : nullptr, sum ? c->d_npsum : nullptr);
      HIP_TRY(hipGetLastError());
    }
    if (rows)
      HIP_TRY(hipMemcpyAsync(node_post + (size_t)d0 * sp.np_row, c->d_npost, sizeof(double) * a.ndraw * sp.np_row,
                             hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipMemcpyAsync(loglik, c->d_loglik, sizeof(double) * n, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(bcounts, c->d_bcounts, sizeof(double) * n * sp.bc_row, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PHY_OK;
}

int kseq_sum_args(const char* who, const phy_kseq_sum_ctx* ctx, int n_draws, const void* blens, const void* params,
                  const void* loglik, const void* bcounts) {
  if (!ctx) return fail(PHY_EINVAL, std::string(who) + ": NULL ctx");
  if (!blens || !params || !loglik || !bcounts) return fail(PHY_EINVAL, std::string(who) + ": NULL host buffer");
  if (n_draws < 1 || n_draws > ctx->base->plan.max_draws)
    return fail(PHY_ERANGE, std::string(who) + ": n_draws out of range (1..max_draws)");
  return PHY_OK;
}
}  // namespace

extern "C" {

int phy_kseq_sum_create(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks,
                        const double* weights, const int32_t* peel, int n_labels, const double* labels,
                        int max_draws, int device, phy_kseq_sum_ctx** out) {
  const std::string who = "phy_kseq_sum_create: ";
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, who + "out is NULL");
  *out = nullptr;
  if (!labels || n_labels < 1) {  // kseq_create takes (0, NULL) for no summaries: refuse those here
    KseqPlan probe;
    int rc = kseq_mix_plan(S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, 1, probe, who);
    if (!rc) rc = kseq_sum_check_labels(K, n_labels, labels, who);
    return rc ? rc : fail(PHY_EINVAL, who + "labels");
  }
  std::unique_ptr<phy_kseq_sum_ctx, void (*)(phy_kseq_sum_ctx*)> c(new phy_kseq_sum_ctx(), free_kseq_sum);
  int rc = kseq_create(who, S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, device, &c->base, n_labels,
                       labels);
  if (rc) return rc;
  const KseqPlan& pl = c->base->plan;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  if ((rc = kseq_sum_plan(pl, n_labels, labels, cus, c->sp, who))) return rc;
  const KseqSumPlan& sp = c->sp;
  for (const void* f : {(const void*)kseq_sum_blab_kernel, (const void*)kseq_sum_down_kernel})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KSEQ_LDS_CAP));
  if ((rc = dalloc(&c->d_labels, sp.n_labels)) || (rc = dalloc(&c->d_blab, sp.n_blab)) ||
      (rc = dalloc(&c->d_sslots, sp.n_sslots)) || (rc = dalloc(&c->d_npost, sp.n_npost)) ||
      (rc = dalloc(&c->d_npsum, sp.n_npsum)) || (rc = dalloc(&c->d_bcounts, sp.n_bcounts)) ||
      (rc = dalloc(&c->d_loglik, sp.n_loglik)))
    return rc;
  HIP_TRY(hipMemcpyAsync(c->d_labels, labels, sizeof(double) * sp.n_labels, hipMemcpyHostToDevice, c->base->stream));
  HIP_TRY(hipMemsetAsync(c->d_npsum, 0, sizeof(double) * sp.n_npsum, c->base->stream));
  HIP_TRY(hipStreamSynchronize(c->base->stream));
  *out = c.release();
  return PHY_OK;
}

int phy_kseq_sum_destroy(phy_kseq_sum_ctx* ctx) {
  free_kseq_sum(ctx);
  return PHY_OK;
}

int phy_kseq_sum_num_branches(const phy_kseq_sum_ctx* ctx) { return ctx ? ctx->base->plan.B : -1; }

int phy_kseq_sum_eval(phy_kseq_sum_ctx* ctx, int n_draws, const double* blens, const double* params, double* loglik,
                      double* bcounts, double* node_post) {
  const int rc = kseq_sum_args("phy_kseq_sum_eval", ctx, n_draws, blens, params, loglik, bcounts);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->base->device));
  return kseq_sum_launch(ctx, n_draws, blens, params, loglik, bcounts, node_post, false);
}

int phy_kseq_sum_reset(phy_kseq_sum_ctx* ctx) {
  if (!ctx) return fail(PHY_EINVAL, "phy_kseq_sum_reset: NULL ctx");
  HIP_TRY(hipSetDevice(ctx->base->device));
  HIP_TRY(hipMemsetAsync(ctx->d_npsum, 0, sizeof(double) * ctx->sp.n_npsum, ctx->base->stream));
  HIP_TRY(hipStreamSynchronize(ctx->base->stream));
  ctx->n_finite = 0;
  return PHY_OK;
}

int phy_kseq_sum_add(phy_kseq_sum_ctx* ctx, int n_draws, const double* blens, const double* params, double* loglik,
                     double* bcounts) {
  int rc = kseq_sum_args("phy_kseq_sum_add", ctx, n_draws, blens, params, loglik, bcounts);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(ctx->base->device));
  if ((rc = kseq_sum_launch(ctx, n_draws, blens, params, loglik, bcounts, nullptr, true))) return rc;
  for (int d = 0; d < n_draws; ++d)
    if (std::isfinite(loglik[d])) ++ctx->n_finite;
  return PHY_OK;
}

int phy_kseq_sum_read(phy_kseq_sum_ctx* ctx, double* node_post_sum, int* n_finite) {
  if (!ctx) return fail(PHY_EINVAL, "phy_kseq_sum_read: NULL ctx");
  if (!node_post_sum) return fail(PHY_EINVAL, "phy_kseq_sum_read: NULL host buffer");
  HIP_TRY(hipSetDevice(ctx->base->device));
  HIP_TRY(hipMemcpyAsync(node_post_sum, ctx->d_npsum, sizeof(double) * ctx->sp.n_npsum, hipMemcpyDeviceToHost,
                         ctx->base->stream));
  HIP_TRY(hipStreamSynchronize(ctx->base->stream));
  if (n_finite) *n_finite = (int)ctx->n_finite;
  return PHY_OK;
}

}  // extern "C"
