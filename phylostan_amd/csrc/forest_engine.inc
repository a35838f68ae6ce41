// forest_engine.inc -- the forest form of the unrescaled pattern sweep
// (include/phylo_hip_forest.h; planned by forest_plan.h): T trees on one
// alignment in one context, every row of a call naming its tree.
//
// Included at the end of phylo_hip.hip, after row_engine.inc, whose RowSweep
// holds the device, the stream, the buffers and the launch chain of "one
// workgroup per row".  The forest's own: its plan (the [T] records and
// mat_branch tables), the kernels' forest flag -- pmat_kernel<false, true>
// numbers a row's matrices by its tree's mat_branch, sweep_kernel<., ., .,
// false, false, true> offsets prog and mat_branch by the row's tree once, as a
// scalar, and walks that tree's records -- the rows' trees (d_tree), the
// output rows and the pinned staging of a call.  The form is fixed by the
// context: the plan's K / register budget / deep-stack placement, ONE
// workgroup per row (so the sweep writes the row's dL/dP in branch order
// itself and no epilogue kernel reads a per-tree table), eig_kernel for every
// call size, and the finalize and chain rule inside the sweep or after it as
// the plan's LDS decides.  Nothing depends on a call's n_rows: a row's bits
// are its own.

struct phy_forest_ctx {
  ForestPlan fp;
  Prefs prefs;
  RowSweep rs;
  int max_rows = 0, outlen = 0;
  int* d_tree = nullptr;
  double* d_out = nullptr;
  // pinned staging of a whole call (contexts whose max_rows keeps it small)
  double *h_in = nullptr, *h_out = nullptr;
  int32_t* h_tree = nullptr;
};

namespace {

void free_forest(phy_forest_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->rs.device);
  row_sweep_free(c->rs);
  if (c->d_tree) (void)hipFree(c->d_tree);
  if (c->d_out) (void)hipFree(c->d_out);
  void* pins[] = {c->h_in, c->h_out, c->h_tree};
  for (void* p : pins)
    if (p) (void)hipHostFree(p);
  delete c;
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
  int rc = plan_for_device(device, [&](int cus) {
    return forest_plan(S, P, C, rooted, model, tipcodes, weights, T, peels, max_rows, c->prefs, cus, c->fp);
  });
  if (rc) return rc;
  const ForestPlan& fp = c->fp;
  const Problem& pb = fp.pb;
  const void* kernel = row_kernel_for<true, false>(fp.plan.K, fp.plan.lat, fp.plan.deep_lds);
  if (!kernel) return fail(PHY_EINVAL, "internal: no forest kernel for the plan");
  c->max_rows = max_rows;
  c->outlen = PHY_OUT_G(pb.B, C);
  const size_t M = (size_t)max_rows, ml = 10 + 2 * (size_t)C;
  if ((rc = row_sweep_create(c->rs, pb, fp.plan, kernel, fp.records, fp.mat_branch, M, c->outlen, device)) ||
      (rc = dalloc(&c->d_tree, M)) || (rc = dalloc(&c->d_out, M * c->outlen)))
    return rc;
  if (M * (pb.B + ml + c->outlen) * sizeof(double) <= ROW_PIN_BYTES) {
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
  const RowSweep& rs = ctx->rs;
  HIP_TRY(hipSetDevice(rs.device));
  hipStream_t st = rs.stream;
  const ForestPlan& fp = ctx->fp;
  const Problem& pb = fp.pb;
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
  HIP_TRY(hipMemcpyAsync(rs.d_blens, sb, sizeof(double) * nb, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(rs.d_model, sm, sizeof(double) * nm, hipMemcpyHostToDevice, st));
  int rc = row_sweep_launch(rs, RowForm{fp.fin, fp.qf, fp.fin_qf}, n_rows, RowExtras{true, ctx->d_tree, fp.rec_stride},
                            ctx->d_out, site_ll ? rs.d_site : nullptr, st);
  if (rc) return rc;
  double* dst = pin ? ctx->h_out : out;
  HIP_TRY(hipMemcpyAsync(dst, ctx->d_out, sizeof(double) * no, hipMemcpyDeviceToHost, st));
  if (site_ll)
    HIP_TRY(hipMemcpyAsync(site_ll, rs.d_site, sizeof(double) * n * pb.P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  if (pin) std::memcpy(out, ctx->h_out, sizeof(double) * no);
  reject_rows(out, n, ctx->outlen);
  return PHY_OK;
}

}  // extern "C"
