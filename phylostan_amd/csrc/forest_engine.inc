// forest_engine.inc -- the forest form of the unrescaled pattern sweep
// (include/phylo_hip_forest.h; planned by forest_plan.h): T trees on one
// alignment in one context, every row of a call naming its tree.
//
// Included at the end of phylo_hip.hip.  The kernels are the pattern sweep's
// own, instantiated with their forest flag: pmat_kernel<false, true> numbers
// a row's matrices by its tree's mat_branch, sweep_kernel<., ., ., false,
// false, true> offsets prog and mat_branch by the row's tree once, as a
// scalar, and walks that tree's records.  The form is fixed by the context:
// the plan's K / register budget / deep-stack placement, ONE workgroup per row
// (so the sweep writes the row's dL/dP in branch order itself and no epilogue
// kernel reads a per-tree table), eig_kernel for every call size, and the
// finalize and chain rule inside the sweep or after it as the plan's LDS
// decides.  Nothing depends on a call's n_rows: a row's bits are its own.

struct phy_forest_ctx {
  ForestPlan fp;
  Prefs prefs;
  int device = 0, max_rows = 0, outlen = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_tips = nullptr;
  double* d_w = nullptr;
  int *d_prog = nullptr, *d_matbr = nullptr, *d_tree = nullptr;
  double *d_pmat = nullptr, *d_eig = nullptr, *d_inner = nullptr, *d_model = nullptr, *d_blens = nullptr;
  double *d_out = nullptr, *d_site = nullptr, *d_grows = nullptr, *d_gslot = nullptr, *d_sslot = nullptr;
  double2 *d_scratch = nullptr, *d_dstk = nullptr;
  // pinned staging of a whole call (contexts whose max_rows keeps it small)
  double *h_in = nullptr, *h_out = nullptr;
  int32_t* h_tree = nullptr;
};

namespace {

constexpr size_t FOREST_PIN_BYTES = (size_t)64 << 20;

const SweepKernel FOREST_KERNELS[] = {
    {2, false, true, false, false, (const void*)sweep_kernel<512, 2, true, false, false, true>},
    {2, false, false, false, false, (const void*)sweep_kernel<512, 2, false, false, false, true>},
    {1, true, true, false, false, (const void*)sweep_kernel<512, 1, true, false, false, true>},
    {1, true, false, false, false, (const void*)sweep_kernel<512, 1, false, false, false, true>},
    {1, false, true, false, false, (const void*)sweep_kernel<1024, 1, true, false, false, true>},
    {1, false, false, false, false, (const void*)sweep_kernel<1024, 1, false, false, false, true>},
};
const void* forest_kernel_for(int K, bool lat, bool dl) {
  for (const SweepKernel& k : FOREST_KERNELS)
    if (k.K == K && k.lat == (lat && K == 1) && k.dl == dl) return k.fn;
  return nullptr;
}

void free_forest(phy_forest_ctx* c) {
  if (!c) return;
  int dev_old = 0;
  (void)hipGetDevice(&dev_old);
  (void)hipSetDevice(c->device);
  void* ptrs[] = {c->d_tips, c->d_w,   c->d_prog, c->d_matbr, c->d_tree,  c->d_pmat,  c->d_eig,     c->d_inner, c->d_model,
                  c->d_blens, c->d_out, c->d_site, c->d_grows, c->d_gslot, c->d_sslot, c->d_scratch, c->d_dstk};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  void* pins[] = {c->h_in, c->h_out, c->h_tree};
  for (void* p : pins)
    if (p) (void)hipHostFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  (void)hipSetDevice(dev_old);
  delete c;
}

// The launches of n rows on st: eigensystems, matrix records, the sweep (one workgroup per row), its epilogue.
int forest_launch(phy_forest_ctx* c, int n, hipStream_t st, double* d_site) {
  const ForestPlan& fp = c->fp;
  const Problem& pb = fp.pb;
  const SweepPlan& pl = fp.plan;
  const int C = pb.C, B = pb.B;
  PmatArgs pa{c->d_model, c->d_blens, c->d_matbr, c->d_eig, c->d_pmat, C, B, pb.kind, pb.nmat, n, pb.R, pb.extra, 0};
  pa.tree_of_row = c->d_tree;
  hipLaunchKernelGGL(eig_kernel, dim3((n + 63) / 64), dim3(64), 0, st, pa);
  HIP_TRY(hipGetLastError());
  const dim3 pgrid((C * pb.nmat + PMAT_WAVE_RECS - 1) / PMAT_WAVE_RECS, n);
  hipLaunchKernelGGL((pmat_kernel<false, true>), pgrid, dim3(64), (size_t)PMAT_WAVE_RECS * pb.R * 4 * sizeof(double), st,
                     pa);
  HIP_TRY(hipGetLastError());
  SweepArgs a{};
  a.tips = c->d_tips; a.weights = c->d_w; a.pmat = c->d_pmat; a.mat_branch = c->d_matbr; a.eig = c->d_eig;
  a.model = c->d_model; a.blens = c->d_blens; a.site_ll = d_site; a.out = c->d_out;
  a.grows = c->d_grows; a.grows_stride = (long long)16 * C * B; a.outlen = c->outlen;
  a.scratch = c->d_scratch; a.dstk = c->d_dstk; a.gslot = c->d_gslot; a.sslot = c->d_sslot; a.inner = c->d_inner;
  a.S = pb.S; a.P = pb.P; a.Ppad = pb.Ppad; a.C = C; a.B = B; a.R = pb.R; a.extra = pb.extra; a.kind = pb.kind;
  a.nsteps = pb.nsteps; a.nslots = pb.nslots; a.ndeep = pb.ndeep; a.nmat = pb.nmat; a.nblk = pl.nblk;
  a.ndl = pl.ndl; a.cap_m = pl.cap_m;
  a.g_direct = 1; a.fin = fp.fin; a.qfused = fp.qf;
  a.tree_of_row = c->d_tree; a.fo_stride = fp.rec_stride;
  {
    const int* prog = c->d_prog;
    void* kargs[] = {(void*)&a, (void*)&prog};
    HIP_TRY(hipLaunchKernel(forest_kernel_for(pl.K, pl.lat, pl.deep_lds), dim3(1, n), dim3(C * WAVE), kargs, pl.lds, st));
  }
  HIP_TRY(hipGetLastError());
  LaunchChoice ch;
  ch.gx = 1; ch.g_direct = 1; ch.fin = fp.fin; ch.qf = fp.qf; ch.fin_qf = fp.fin_qf; ch.gsum_in = 0;
  FinArgs f{};
  f.gslot = c->d_gslot; f.sslot = c->d_sslot; f.pmat = c->d_pmat; f.inner = c->d_inner; f.eig = c->d_eig;
  f.gpos = nullptr;  // read only when a row spans workgroups
  f.blens = c->d_blens; f.model = c->d_model; f.out = c->d_out; f.grows = c->d_grows;
  f.grows_stride = (long long)16 * C * B; f.outlen = c->outlen;
  f.C = C; f.B = B; f.nmat = pb.nmat; f.R = pb.R; f.kind = pb.kind;
  f.gx = 1; f.g_direct = 1; f.gsum_in = 0; f.qf = fp.fin_qf;
  int rc = launch_finalize(ch, f, n, st);
  if (rc) return rc;
  if (!fp.qf && !fp.fin_qf) {
    hipLaunchKernelGGL(qgrad_kernel, dim3(n), dim3(QG_THREADS), 0, st, f);
    HIP_TRY(hipGetLastError());
  }
  return PHY_OK;
}

}  // namespace

extern "C" {

int phy_forest_create(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                      int T, const int32_t* peels, int max_rows, int device, phy_forest_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  std::unique_ptr<phy_forest_ctx, void (*)(phy_forest_ctx*)> c(new phy_forest_ctx(), free_forest);
  c->prefs = prefs_from_env();
  // planned before the device is touched (the refusals need none), again if its CU count is not the assumed one
  int cus = SweepPlan().cu_count;
  int rc = forest_plan(S, P, C, rooted, model, tipcodes, weights, T, peels, max_rows, c->prefs, cus, c->fp);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && v > 0 && v != cus) {
      cus = v;
      if ((rc = forest_plan(S, P, C, rooted, model, tipcodes, weights, T, peels, max_rows, c->prefs, cus, c->fp))) return rc;
    }
  }
  const ForestPlan& fp = c->fp;
  const Problem& pb = fp.pb;
  if (!forest_kernel_for(fp.plan.K, fp.plan.lat, fp.plan.deep_lds)) return fail(PHY_EINVAL, "internal: no forest kernel for the plan");
  hipError_t he = hipSetDevice(device);
  if (he != hipSuccess) return fail(PHY_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
  c->device = device;
  c->max_rows = max_rows;
  c->outlen = PHY_OUT_G(pb.B, C);
  for (const SweepKernel& k : FOREST_KERNELS)
    (void)hipFuncSetAttribute(k.fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
  (void)hipFuncSetAttribute((const void*)finalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t M = (size_t)max_rows, ncolwg = (size_t)C * WAVE, ml = 10 + 2 * (size_t)C;
  if ((rc = dalloc(&c->d_tips, (size_t)S * pb.Ppad / 2)) || (rc = dalloc(&c->d_w, (size_t)pb.Ppad)) ||
      (rc = dalloc(&c->d_prog, fp.records.size())) || (rc = dalloc(&c->d_matbr, fp.mat_branch.size())) ||
      (rc = dalloc(&c->d_tree, M)) || (rc = dalloc(&c->d_pmat, M * C * pb.nmat * pb.R * 4)) ||
      (rc = dalloc(&c->d_eig, M * EIG_LEN)) || (rc = dalloc(&c->d_inner, M * C * pb.B)) ||
      (rc = dalloc(&c->d_model, M * ml)) || (rc = dalloc(&c->d_blens, M * pb.B)) ||
      (rc = dalloc(&c->d_out, M * c->outlen)) || (rc = dalloc(&c->d_site, M * P)) ||
      (rc = dalloc(&c->d_grows, M * 16 * C * pb.B)) || (rc = dalloc(&c->d_gslot, M * C * pb.nmat * 16)) ||
      (rc = dalloc(&c->d_sslot, M * C * 8)) ||
      (rc = dalloc(&c->d_scratch, M * std::max(pb.nslots, 1) * 2 * 2 * ncolwg)) ||
      (rc = dalloc(&c->d_dstk, M * std::max(pb.ndeep, 1) * 2 * 2 * ncolwg)))
    return rc;
  {
    std::vector<double> w(pb.Ppad, 0.0);
    std::copy(pb.w.begin(), pb.w.end(), w.begin());
    if ((rc = upload(c->d_tips, pack_tips(pb))) || (rc = upload(c->d_w, w)) || (rc = upload(c->d_prog, fp.records)) ||
        (rc = upload(c->d_matbr, fp.mat_branch)))
      return rc;
  }
  if (M * (pb.B + ml + c->outlen) * sizeof(double) <= FOREST_PIN_BYTES) {
    HIP_TRY(hipHostMalloc((void**)&c->h_in, sizeof(double) * M * (pb.B + ml), hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&c->h_out, sizeof(double) * M * c->outlen, hipHostMallocDefault));
    HIP_TRY(hipHostMalloc((void**)&c->h_tree, sizeof(int32_t) * M, hipHostMallocDefault));
  }
  *out = c.release();
  return PHY_OK;
}

int phy_forest_destroy(phy_forest_ctx* ctx) {
  free_forest(ctx);
  return PHY_OK;
}

int phy_forest_num_trees(const phy_forest_ctx* ctx) { return ctx ? ctx->fp.T : -1; }
int phy_forest_num_branches(const phy_forest_ctx* ctx) { return ctx ? ctx->fp.pb.B : -1; }
int phy_forest_output_len(const phy_forest_ctx* ctx) { return ctx ? ctx->outlen : -1; }

int phy_forest_info(const phy_forest_ctx* ctx, int* cols, int* cap_m, int* max_chunks, int* min_chunks, int* max_depth,
                    int* min_depth, int* deep_in_lds, int* lds_bytes) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  const ForestPlan& fp = ctx->fp;
  if (cols) *cols = fp.plan.K;
  if (cap_m) *cap_m = fp.plan.cap_m;
  if (max_chunks) *max_chunks = fp.max_chunks;
  if (min_chunks) *min_chunks = fp.min_chunks;
  if (max_depth) *max_depth = fp.max_depth;
  if (min_depth) *min_depth = fp.min_depth;
  if (deep_in_lds) *deep_in_lds = fp.plan.ndl;
  if (lds_bytes) *lds_bytes = (int)fp.plan.lds;
  return PHY_OK;
}

int phy_forest_plan(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights, int T,
                    const int32_t* peels, int max_rows, int cu_count, int* facts, int* chunks, int* depths) {
  g_err.clear();
  ForestPlan fp;
  const int rc = forest_plan(S, P, C, rooted, model, tipcodes, weights, T, peels, max_rows, prefs_from_env(),
                             cu_count > 0 ? cu_count : SweepPlan().cu_count, fp);
  if (rc) return rc;
  if (facts) {
    const int fv[12] = {fp.plan.K, fp.plan.cap_m, fp.max_chunks, fp.min_chunks, fp.max_depth, fp.min_depth, fp.plan.ndl,
                        (int)fp.plan.lds, fp.plan.lat ? 1 : 0, fp.fin, fp.qf, fp.fin_qf};
    std::copy(fv, fv + 12, facts);
  }
  if (chunks) std::copy(fp.nchunks.begin(), fp.nchunks.end(), chunks);
  if (depths) std::copy(fp.ndeep.begin(), fp.ndeep.end(), depths);
  return PHY_OK;
}

int phy_forest_eval(phy_forest_ctx* ctx, int n_rows, const int32_t* tree_of_row, const double* blens,
                    const double* model, double* out, double* site_ll) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (!tree_of_row || !blens || !model || !out) return fail(PHY_EINVAL, "NULL host buffer");
  if (n_rows < 1 || n_rows > ctx->max_rows) return fail(PHY_ERANGE, "n_rows out of range (1..max_rows)");
  const int T = ctx->fp.T;
  for (int r = 0; r < n_rows; ++r)
    if (tree_of_row[r] < 0 || tree_of_row[r] >= T)
      return fail(PHY_ERANGE, "row " + std::to_string(r) + ": tree " + std::to_string(tree_of_row[r]) +
                                  " outside 0.." + std::to_string(T - 1));
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const Problem& pb = ctx->fp.pb;
  const size_t n = (size_t)n_rows, ml = 10 + 2 * (size_t)pb.C, nb = n * pb.B, nm = n * ml, no = n * ctx->outlen;
  const bool pin = ctx->h_in != nullptr;
  const double *sb = blens, *sm = model;
  const int32_t* stree = tree_of_row;
  if (pin) {
    std::memcpy(ctx->h_in, blens, sizeof(double) * nb);
    std::memcpy(ctx->h_in + nb, model, sizeof(double) * nm);
    std::memcpy(ctx->h_tree, tree_of_row, sizeof(int32_t) * n);
    sb = ctx->h_in; sm = ctx->h_in + nb; stree = ctx->h_tree;
  }
  HIP_TRY(hipMemcpyAsync(ctx->d_tree, stree, sizeof(int32_t) * n, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_blens, sb, sizeof(double) * nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_model, sm, sizeof(double) * nm, hipMemcpyHostToDevice, st));
  int rc = forest_launch(ctx, n_rows, st, site_ll ? ctx->d_site : nullptr);
  if (rc) return rc;
  double* dst = pin ? ctx->h_out : out;
  HIP_TRY(hipMemcpyAsync(dst, ctx->d_out, sizeof(double) * no, hipMemcpyDeviceToHost, st));
  if (site_ll)
    HIP_TRY(hipMemcpyAsync(site_ll, ctx->d_site, sizeof(double) * n * pb.P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (pin) std::memcpy(out, ctx->h_out, sizeof(double) * no);
  // a rejected row: -inf and a zero gradient
  for (size_t r = 0; r < n; ++r) {
    double* row = out + r * ctx->outlen;
    if (std::isfinite(row[0])) continue;
    row[0] = -INFINITY;
    std::fill(row + 1, row + ctx->outlen, 0.0);
  }
  return PHY_OK;
}

}  // extern "C"
