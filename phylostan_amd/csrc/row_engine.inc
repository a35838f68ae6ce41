// row_engine.inc -- the host path of "the unrescaled pattern sweep at ONE
// workgroup per row", shared by the engines whose rows carry something of
// their own (forest_engine.inc: a tree; part_engine.inc: a partition) and
// included in phylo_hip.hip before them.  A RowSweep owns the device, the
// stream and every buffer the launch chain reads or writes for up to M rows;
// row_sweep_launch runs the chain: eig_kernel, pmat_kernel<false, .>, the
// engine's sweep_kernel at dim3(1, rows), the finalize and qgrad_kernel as the
// planner's RowForm places them (sweep_plan.h).  The form is fixed by the
// context, never by a call.  An engine adds its plan, its kernel
// (row_kernel_for), a launch's RowExtras and the buffers only it has.

namespace {

constexpr size_t ROW_PIN_BYTES = (size_t)64 << 20;  // a context stages whole calls in pinned memory up to this

// The six (K, register budget, deep stack in LDS) instantiations of the sweep's <FO, PT> form.
template <bool FO, bool PT>
const void* row_kernel_for(int K, bool lat, bool dl) {
  const SweepKernel kernels[] = {
      {2, false, true, false, false, (const void*)sweep_kernel<512, 2, true, false, false, FO, PT>},
      {2, false, false, false, false, (const void*)sweep_kernel<512, 2, false, false, false, FO, PT>},
      {1, true, true, false, false, (const void*)sweep_kernel<512, 1, true, false, false, FO, PT>},
      {1, true, false, false, false, (const void*)sweep_kernel<512, 1, false, false, false, FO, PT>},
      {1, false, true, false, false, (const void*)sweep_kernel<1024, 1, true, false, false, FO, PT>},
      {1, false, false, false, false, (const void*)sweep_kernel<1024, 1, false, false, false, FO, PT>},
  };
  for (const SweepKernel& k : kernels)
    if (k.K == K && k.lat == (lat && K == 1) && k.dl == dl) return k.fn;
  return nullptr;
}
// Instantiated here, the forest's form before launch_matrices and the partitions' after it: the kernels' order
// in the module stays what it was when each engine named its own six.
template const void* row_kernel_for<true, false>(int, bool, bool);

// The eigensystems (one thread per row) and the matrix records of pa.n rows on st; `forest`: pa.mat_branch is
// [T][nmat] and pa.tree_of_row names every row's tree.  Sequence summaries launch theirs here too.
int launch_matrices(const PmatArgs& pa, bool forest, hipStream_t st) {
  hipLaunchKernelGGL(eig_kernel, dim3((pa.n + 63) / 64), dim3(64), 0, st, pa);
  HIP_TRY(hipGetLastError());
  const dim3 pgrid((pa.C * pa.nmat + PMAT_WAVE_RECS - 1) / PMAT_WAVE_RECS, pa.n);
  const size_t plds = (size_t)PMAT_WAVE_RECS * pa.R * 4 * sizeof(double);
  if (forest)
    hipLaunchKernelGGL((pmat_kernel<false, true>), pgrid, dim3(64), plds, st, pa);
  else
    hipLaunchKernelGGL((pmat_kernel<false, false>), pgrid, dim3(64), plds, st, pa);
  HIP_TRY(hipGetLastError());
  return PHY_OK;
}
template const void* row_kernel_for<false, true>(int, bool, bool);

struct RowSweep {
  const Problem* pb = nullptr;  // the owning context's
  const SweepPlan* plan = nullptr;
  const void* kernel = nullptr;  // the plan's of row_kernel_for
  int device = 0, row_len = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_tips = nullptr;
  double* d_w = nullptr;
  int *d_prog = nullptr, *d_matbr = nullptr;
  double *d_pmat = nullptr, *d_eig = nullptr, *d_inner = nullptr, *d_model = nullptr, *d_blens = nullptr;
  double *d_site = nullptr, *d_grows = nullptr, *d_gslot = nullptr, *d_sslot = nullptr;
  double2 *d_scratch = nullptr, *d_dstk = nullptr;
};

// What differs between the engines in a launch: the forest's tree of every row and ints per tree in the
// records (mat_branch is then [T][nmat]), or the partitions' block ranges and their number.
struct RowExtras {
  bool forest;
  const int* table;  // tree_of_row | pt_blk
  int count;         // fo_stride | pt_K
};

// Sets the device, opts the kernel and finalize_kernel into LDS_CAP, creates the stream, allocates for M rows
// of row_len doubles and uploads the alignment, the records and the matrix numbering.  pb and plan stay the
// caller's and outlive rs.
int row_sweep_create(RowSweep& rs, const Problem& pb, const SweepPlan& plan, const void* kernel,
                     const std::vector<int>& records, const std::vector<int>& mat_branch, size_t M, int row_len,
                     int device) {
  hipError_t he = hipSetDevice(device);
  if (he != hipSuccess) return fail(PHY_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
  rs.pb = &pb;
  rs.plan = &plan;
  rs.kernel = kernel;
  rs.device = device;
  rs.row_len = row_len;
  (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
  (void)hipFuncSetAttribute((const void*)finalize_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
  HIP_TRY(hipStreamCreateWithFlags(&rs.stream, hipStreamNonBlocking));
  const size_t C = pb.C, ncolwg = C * WAVE, ml = 10 + 2 * C;
  int rc;
  if ((rc = dalloc(&rs.d_tips, (size_t)pb.S * pb.Ppad / 2)) || (rc = dalloc(&rs.d_w, (size_t)pb.Ppad)) ||
      (rc = dalloc(&rs.d_prog, records.size())) || (rc = dalloc(&rs.d_matbr, mat_branch.size())) ||
      (rc = dalloc(&rs.d_pmat, M * C * pb.nmat * pb.R * 4)) || (rc = dalloc(&rs.d_eig, M * EIG_LEN)) ||
      (rc = dalloc(&rs.d_inner, M * C * pb.B)) || (rc = dalloc(&rs.d_model, M * ml)) ||
      (rc = dalloc(&rs.d_blens, M * pb.B)) || (rc = dalloc(&rs.d_site, M * pb.P)) ||
      (rc = dalloc(&rs.d_grows, M * 16 * C * pb.B)) || (rc = dalloc(&rs.d_gslot, M * C * pb.nmat * 16)) ||
      (rc = dalloc(&rs.d_sslot, M * C * 8)) ||
      (rc = dalloc(&rs.d_scratch, M * std::max(pb.nslots, 1) * 2 * 2 * ncolwg)) ||
      (rc = dalloc(&rs.d_dstk, M * std::max(pb.ndeep, 1) * 2 * 2 * ncolwg)) ||
      (rc = upload_alignment(rs.d_tips, rs.d_w, pb)) || (rc = upload(rs.d_prog, records)) ||
      (rc = upload(rs.d_matbr, mat_branch)))
    return rc;
  return PHY_OK;
}

// With rs.device current (DeviceGuard).
void row_sweep_free(RowSweep& rs) {
  void* ptrs[] = {rs.d_tips,  rs.d_w,    rs.d_prog,  rs.d_matbr, rs.d_pmat,  rs.d_eig,     rs.d_inner, rs.d_model,
                  rs.d_blens, rs.d_site, rs.d_grows, rs.d_gslot, rs.d_sslot, rs.d_scratch, rs.d_dstk};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (rs.stream) (void)hipStreamDestroy(rs.stream);
}

// The launches of n rows on st, their branch lengths and model vectors in d_blens / d_model: eigensystems,
// matrix records, the sweep (one workgroup per row), its epilogue.  Rows of row_len doubles to `out`.
int row_sweep_launch(const RowSweep& rs, const RowForm& form, int n, const RowExtras& x, double* out, double* d_site,
                     hipStream_t st) {
  const Problem& pb = *rs.pb;
  const SweepPlan& pl = *rs.plan;
  const int C = pb.C, B = pb.B;
  PmatArgs pa{rs.d_model, rs.d_blens, rs.d_matbr, rs.d_eig, rs.d_pmat, C, B, pb.kind, pb.nmat, n, pb.R, pb.extra, 0};
  if (x.forest) pa.tree_of_row = x.table;
  int rc = launch_matrices(pa, x.forest, st);
  if (rc) return rc;
  LaunchChoice ch;  // choose_launch's at one workgroup per row
  ch.gx = 1; ch.g_direct = 1; ch.fin = form.fin; ch.qf = form.qf; ch.fin_qf = form.fin_qf; ch.gsum_in = 0;
  ch.eig = rs.d_eig; ch.mat_branch = rs.d_matbr;
  ch.gpos = nullptr;  // read only when a row spans workgroups
  const SweepBufs bufs{rs.d_tips, rs.d_w, rs.d_pmat, rs.d_inner, rs.d_gslot, rs.d_sslot, rs.d_scratch, rs.d_dstk, rs.row_len};
  const CallBufs io{rs.d_blens, rs.d_model, out, d_site, rs.d_grows, (long long)16 * C * B};
  SweepArgs a = sweep_args(bufs, pb, pl, ch, io);
  if (x.forest) { a.tree_of_row = x.table; a.fo_stride = x.count; }
  else { a.pt_blk = x.table; a.pt_K = x.count; }
  {
    const int* prog = rs.d_prog;
    void* kargs[] = {(void*)&a, (void*)&prog};
    HIP_TRY(hipLaunchKernel(rs.kernel, dim3(1, n), dim3(C * WAVE), kargs, pl.lds, st));
  }
  HIP_TRY(hipGetLastError());
  const FinArgs f = fin_args(bufs, pb, ch, io);
  if ((rc = launch_finalize(ch, f, n, st))) return rc;
  if (!form.qf && !form.fin_qf) {
    hipLaunchKernelGGL(qgrad_kernel, dim3(n), dim3(QG_THREADS), 0, st, f);
    HIP_TRY(hipGetLastError());
  }
  return PHY_OK;
}

}  // namespace
