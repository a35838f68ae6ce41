// part_engine.inc -- the partitioned form of the unrescaled pattern sweep
// (include/phylo_hip_part.h; planned by part_plan.h): K disjoint site sets of
// one alignment on one tree, each with its own model vector and relative rate
// mu_k, the branch lengths shared:
//
//   log L(t, mu, theta) = sum_k log L_k(mu_k t; theta_k).
//
// Included at the end of phylo_hip.hip, after row_engine.inc, whose RowSweep
// holds the device, the stream, the buffers and the launch chain of "one
// workgroup per row".  Row r = d * K + k of the launch is partition k of draw
// d: it carries theta_k of the draw and the branch lengths mu_k t
// (part_scale_kernel).  eig_kernel, pmat_kernel, the finalize and qgrad_kernel
// run unchanged on the n * K rows; sweep_kernel runs in its PT form, ONE
// workgroup per row walking the row's partition's blocks of the padded
// alignment.  part_combine_kernel then folds a draw's K rows into the draw's
// output row in a fixed order (partition_combine_host in
// phylostan_amd/partition.py restates it).  The partitions' own: their plan,
// the block ranges (d_blk), the draws' t and mu, the two kernels here, the
// rows and the folded output, the pinned staging of a call and the gather of
// site_ll.  The form is the context's, never a call's: a row's bits are its
// own.

struct phy_part_ctx {
  PartPlan pp;
  Prefs prefs;
  RowSweep rs;
  int max_draws = 0, rowlen = 0, outlen = 0;
  int* d_blk = nullptr;
  double *d_t = nullptr, *d_mu = nullptr, *d_rows = nullptr, *d_out = nullptr;
  // pinned staging of a whole call (contexts whose max_draws keeps it small)
  double *h_in = nullptr, *h_out = nullptr;
  std::vector<double> site_tmp;  // the rows' site log-likelihoods in padded columns, before the gather
};

namespace {

constexpr int PART_THREADS = 256;

// bl[d][k][b] = mu[d][k] * t[d][b]: one rounded product.
__global__ void __launch_bounds__(PART_THREADS) part_scale_kernel(const double* __restrict__ t,
                                                                   const double* __restrict__ mu,
                                                                   double* __restrict__ bl, int B, int K, int n) {
#pragma clang fp contract(off)
  const size_t i = (size_t)blockIdx.x * PART_THREADS + threadIdx.x;
  if (i >= (size_t)n * K * B) return;
  const size_t row = i / B;  // d * K + k
  const int b = (int)(i - row * B);
  const size_t d = row / K;
  bl[i] = mu[row] * t[d * B + b];
}

// One workgroup per draw folds its K rows [log L][g_b][tail] into
// [log L][d/dt B] then per partition [d/dmu_k][tail_k]:
//   log L   = (((L_0 + L_1) + L_2) + ...)
//   d/dt_b  = (((mu_0 g_0b) + (mu_1 g_1b)) + ...)           rounded products, left to right over k
//   d/dmu_k = ((((t_0 g_k0) + (t_1 g_k1)) + (t_2 g_k2)) + ...)  rounded products, left to right over b
// No atomics, no contraction.  A draw with a partition whose log L is not finite: -inf and zeros.
__global__ void __launch_bounds__(PART_THREADS) part_combine_kernel(const double* __restrict__ rows,
                                                                     const double* __restrict__ t,
                                                                     const double* __restrict__ mu,
                                                                     double* __restrict__ out, int B, int K, int tail,
                                                                     int rowlen, int outlen) {
#pragma clang fp contract(off)
  const int d = blockIdx.x;
  const double* r0 = rows + (size_t)d * K * rowlen;
  const double* td = t + (size_t)d * B;
  const double* mud = mu + (size_t)d * K;
  double* o = out + (size_t)d * outlen;
  bool ok = true;
  for (int k = 0; k < K; ++k) ok = ok && isfinite(r0[(size_t)k * rowlen]);
  if (!ok) {
    for (int j = threadIdx.x; j < outlen; j += PART_THREADS) o[j] = j == 0 ? -INFINITY : 0.0;
    return;
  }
  for (int j = threadIdx.x; j < outlen; j += PART_THREADS) {
    double v;
    if (j == 0) {
      v = r0[0];
      for (int k = 1; k < K; ++k) v = v + r0[(size_t)k * rowlen];
    } else if (j <= B) {
      const int b = j - 1;
      v = mud[0] * r0[1 + b];
      for (int k = 1; k < K; ++k) v = v + mud[k] * r0[(size_t)k * rowlen + 1 + b];
    } else {
      const int q = j - 1 - B, k = q / (1 + tail), e = q - k * (1 + tail);
      const double* rk = r0 + (size_t)k * rowlen;
      if (e == 0) {
        v = td[0] * rk[1];
        for (int b = 1; b < B; ++b) v = v + td[b] * rk[1 + b];
      } else {
        v = rk[1 + B + e - 1];
      }
    }
    o[j] = v;
  }
}

void free_part(phy_part_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->rs.device);
  row_sweep_free(c->rs);
  void* ptrs[] = {c->d_blk, c->d_t, c->d_mu, c->d_rows, c->d_out};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (c->h_in) (void)hipHostFree(c->h_in);
  if (c->h_out) (void)hipHostFree(c->h_out);
  delete c;
}

// The launches of n draws on st: the scaled branch lengths, the row engine's chain on the n * K rows, the fold.
int part_launch(phy_part_ctx* c, int n, hipStream_t st, double* d_site) {
  const PartPlan& pp = c->pp;
  const int C = pp.pb.C, B = pp.pb.B, K = pp.K, nr = n * K;
  {
    const size_t items = (size_t)nr * B;
    hipLaunchKernelGGL(part_scale_kernel, dim3((unsigned)((items + PART_THREADS - 1) / PART_THREADS)), dim3(PART_THREADS),
                       0, st, c->d_t, c->d_mu, c->rs.d_blens, B, K, n);
    HIP_TRY(hipGetLastError());
  }
  const int rc = row_sweep_launch(c->rs, RowForm{pp.fin, pp.qf, pp.fin_qf}, nr, RowExtras{false, c->d_blk, K}, c->d_rows,
                                  d_site, st);
  if (rc) return rc;
  hipLaunchKernelGGL(part_combine_kernel, dim3(n), dim3(PART_THREADS), 0, st, c->d_rows, c->d_t, c->d_mu, c->d_out, B, K,
                     2 * C + 14, c->rowlen, c->outlen);
  HIP_TRY(hipGetLastError());
  return PHY_OK;
}

}  // namespace

extern "C" {

int phy_part_create(int S, int K, const int32_t* P_k, int C, int rooted, int model, const uint8_t* tipcodes,
                    const double* weights, const int32_t* peel, int max_draws, int device, phy_part_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  std::unique_ptr<phy_part_ctx, void (*)(phy_part_ctx*)> c(new phy_part_ctx(), free_part);
  c->prefs = prefs_from_env();
  int rc = plan_for_device(device, [&](int cus) {
    return part_plan(S, K, P_k, C, rooted, model, tipcodes, weights, peel, max_draws, c->prefs, cus, c->pp);
  });
  if (rc) return rc;
  const PartPlan& pp = c->pp;
  const Problem& pb = pp.pb;
  const void* kernel = row_kernel_for<false, true>(pp.plan.K, pp.plan.lat, pp.plan.deep_lds);
  if (!kernel) return fail(PHY_EINVAL, "internal: no partition kernel for the plan");
  c->max_draws = max_draws;
  c->rowlen = PHY_OUT_G(pb.B, C);
  c->outlen = 1 + pb.B + K * (1 + 2 * C + 14);
  const size_t D = (size_t)max_draws, M = D * K, ml = 10 + 2 * (size_t)C;
  if ((rc = row_sweep_create(c->rs, pb, pp.plan, kernel, pp.plan.records, pb.mat_branch, M, c->rowlen, device)) ||
      (rc = dalloc(&c->d_blk, pp.blk.size())) || (rc = dalloc(&c->d_t, D * pb.B)) || (rc = dalloc(&c->d_mu, M)) ||
      (rc = dalloc(&c->d_rows, M * c->rowlen)) || (rc = dalloc(&c->d_out, D * c->outlen)) ||
      (rc = upload(c->d_blk, pp.blk)))
    return rc;
  if ((D * (pb.B + c->outlen) + M * (1 + ml + c->rowlen)) * sizeof(double) <= ROW_PIN_BYTES) {
    HIP_TRY(hipHostMalloc((void**)&c->h_in, sizeof(double) * (D * pb.B + M * (1 + ml)), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&c->h_out, sizeof(double) * (D * c->outlen + M * c->rowlen), hipHostMallocDefault));
  }
  *out = c.release();
  return PHY_OK;
}

int phy_part_destroy(phy_part_ctx* ctx) {
  free_part(ctx);
  return PHY_OK;
}

int phy_part_num_partitions(const phy_part_ctx* ctx) { return ctx ? ctx->pp.K : -1; }
int phy_part_num_branches(const phy_part_ctx* ctx) { return ctx ? ctx->pp.pb.B : -1; }
int phy_part_row_len(const phy_part_ctx* ctx) { return ctx ? ctx->rowlen : -1; }
int phy_part_output_len(const phy_part_ctx* ctx) { return ctx ? ctx->outlen : -1; }

namespace {
void part_facts(const PartPlan& pp, int* facts) {
  const int fv[PHY_PART_FACTS] = {pp.plan.K, pp.plan.lat ? 1 : 0, pp.plan.nblk, pp.pb.P, pp.pb.Ppad, pp.pb.R,
                                  (int)(pp.pb.extra & 0xffffffffull), (int)(pp.pb.extra >> 32), pp.plan.cap_m, pp.plan.nchunks,
                                  pp.plan.ndl, pp.plan.deep_lds ? 1 : 0, (int)pp.plan.lds, pp.fin, pp.qf, pp.fin_qf};
  std::copy(fv, fv + PHY_PART_FACTS, facts);
}
}  // namespace

int phy_part_info(const phy_part_ctx* ctx, int* facts, int* blocks) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (facts) part_facts(ctx->pp, facts);
  if (blocks) std::copy(ctx->pp.blk.begin(), ctx->pp.blk.end(), blocks);
  return PHY_OK;
}

int phy_part_plan(int S, int K, const int32_t* P_k, int C, int rooted, int model, const uint8_t* tipcodes,
                  const double* weights, const int32_t* peel, int max_draws, int cu_count, int* facts, int* blocks,
                  int* col_part, int* col_pat) {
  g_err.clear();
  PartPlan pp;
  const int rc = part_plan(S, K, P_k, C, rooted, model, tipcodes, weights, peel, max_draws, prefs_from_env(),
                           cu_count > 0 ? cu_count : SweepPlan().cu_count, pp);
  if (rc) return rc;
  if (facts) part_facts(pp, facts);
  if (blocks) std::copy(pp.blk.begin(), pp.blk.end(), blocks);
  if (col_part) std::copy(pp.col_part.begin(), pp.col_part.end(), col_part);
  if (col_pat) std::copy(pp.col_pat.begin(), pp.col_pat.end(), col_pat);
  return PHY_OK;
}

int phy_part_eval(phy_part_ctx* ctx, int n_draws, const double* blens, const double* mu, const double* model,
                  double* out, double* part_rows, double* site_ll) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (!blens || !mu || !model || !out) return fail(PHY_EINVAL, "NULL host buffer");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, "n_draws out of range (1..max_draws)");
  HIP_TRY(hipSetDevice(ctx->rs.device));
  hipStream_t st = ctx->rs.stream;
  const PartPlan& pp = ctx->pp;
  const Problem& pb = pp.pb;
  const size_t n = (size_t)n_draws, K = (size_t)pp.K, ml = 10 + 2 * (size_t)pb.C;
  const size_t nb = n * pb.B, nu = n * K, nm = nu * ml, no = n * ctx->outlen, nrw = nu * ctx->rowlen;
  const bool pin = ctx->h_in != nullptr;
  const double *sb = blens, *su = mu, *sm = model;
  if (pin) {
    std::memcpy(ctx->h_in, blens, sizeof(double) * nb);
    std::memcpy(ctx->h_in + nb, mu, sizeof(double) * nu);
    std::memcpy(ctx->h_in + nb + nu, model, sizeof(double) * nm);
    sb = ctx->h_in; su = ctx->h_in + nb; sm = ctx->h_in + nb + nu;
  }
  HIP_TRY(hipMemcpyAsync(ctx->d_t, sb, sizeof(double) * nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_mu, su, sizeof(double) * nu, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->rs.d_model, sm, sizeof(double) * nm, hipMemcpyHostToDevice, st));
  int rc = part_launch(ctx, n_draws, st, site_ll ? ctx->rs.d_site : nullptr);
  if (rc) return rc;
  double* dst = pin ? ctx->h_out : out;
  HIP_TRY(hipMemcpyAsync(dst, ctx->d_out, sizeof(double) * no, hipMemcpyDeviceToHost, st));
  if (part_rows)
    HIP_TRY(hipMemcpyAsync(pin ? ctx->h_out + no : part_rows, ctx->d_rows, sizeof(double) * nrw, hipMemcpyDeviceToHost, st));
  if (site_ll) {
    ctx->site_tmp.resize(nu * pb.P);
    HIP_TRY(hipMemcpyAsync(ctx->site_tmp.data(), ctx->rs.d_site, sizeof(double) * nu * pb.P, hipMemcpyDeviceToHost, st));
  }
  HIP_TRY(hipStreamSynchronize(st));
  if (pin) {
    std::memcpy(out, ctx->h_out, sizeof(double) * no);
    if (part_rows) std::memcpy(part_rows, ctx->h_out + no, sizeof(double) * nrw);
  }
  // a rejected partition row: -inf and a zero gradient, as phy_eval's rows (the fold has already refused its draw)
  if (part_rows) reject_rows(part_rows, nu, ctx->rowlen);
  // the caller's unpadded pattern order: row d * K + k wrote its partition's columns of the padded alignment
  if (site_ll)
    for (size_t d = 0; d < n; ++d)
      for (size_t k = 0; k < K; ++k)
        std::memcpy(site_ll + d * pp.Psum + pp.off[k], ctx->site_tmp.data() + (d * K + k) * pb.P + pp.col0[k],
                    sizeof(double) * pp.Pk[k]);
  return PHY_OK;
}

}  // extern "C"
