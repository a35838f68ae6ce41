// seqsum_engine.inc -- the sequence-summary engine (include/phylo_hip_seqsum.h;
// planned by seqsum_plan.h): per draw, the marginal state posterior of every
// internal node at every pattern, every pattern's rate-category posterior and
// its mean rate, and their running sum over draws, kept on the device.
//
// Included at the end of phylo_hip.hip.  The matrix records are the pattern
// sweep's (eig_kernel, pmat_kernel<false, false>), numbered by branch: matrix
// m is the edge above node m.  seqsum_kernel keeps what an evaluation throws
// away: the forward partials part[v] and the pre-order partials q[v] of every
// internal node, in a global workspace [draw][part | q][node][c][state][column]
// (coalesced along the columns).  One workgroup per (64 pattern columns,
// draw), one wave per rate category, one lane per column; a thread reads back
// only what it wrote itself, so the passes need no barrier of their own.  The
// barriers are those of the sums over categories, which go through LDS in
// category order: L_i at the root, and one per internal node in the reverse
// pass (two buffers in turn: one barrier a node).  All arithmetic is fp64
// without rescaling.  seqsum_ll_kernel sums the draw's weighted site
// log-likelihoods in a fixed shape; seqsum_acc_kernel adds the launch's finite
// draws to the accumulator, one thread per element, in draw order.

struct phy_seqsum_ctx {
  SeqsumPlan sp;
  int device = 0, max_draws = 0;
  long long n_finite = 0;
  hipStream_t stream = nullptr;
  uint8_t* d_tips = nullptr;
  int *d_steps = nullptr, *d_matbr = nullptr;
  double *d_w = nullptr, *d_pmat = nullptr, *d_eig = nullptr, *d_model = nullptr, *d_blens = nullptr;
  double *d_ws = nullptr, *d_rows = nullptr, *d_site = nullptr, *d_acc = nullptr;
};

struct SeqArgs {
  const uint8_t* tips;    // [S][Ppad / 2] record-vector nibbles (pack_tips)
  const double* weights;  // [Ppad], zero on padding
  const double* model;    // [draw][10 + 2C]
  double* ws;             // [draw][2][S-1][C][4][Ppad]
  double* rows;           // [draw][row_len]
  double* site;           // [draw][Ppad] w_i log L_i, zero on padding
  int S, P, Ppad, C, B, R;
  long long row_len, off_cat, off_rate, node_stride, ws_draw;
};

namespace {

constexpr int SEQ_LL_THREADS = 256;
constexpr int SEQ_ACC_THREADS = 256;

// y = P x from the record's four columns (rec[j * 4 + i] = P[i][j])
__device__ __forceinline__ void seq_matvec(const double* __restrict__ rec, const double x[4], double y[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double acc = rec[i] * x[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) acc = fma(rec[j * 4 + i], x[j], acc);
    y[i] = acc;
  }
}
// y = P^T x
__device__ __forceinline__ void seq_matvec_t(const double* __restrict__ rec, const double x[4], double y[4]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    double acc = rec[j * 4] * x[0];
#pragma unroll
    for (int i = 1; i < 4; ++i) acc = fma(rec[j * 4 + i], x[i], acc);
    y[j] = acc;
  }
}

__global__ void __launch_bounds__(1024) seqsum_kernel(SeqArgs a, const int* __restrict__ steps,
                                                      const double* __restrict__ pmat) {
  extern __shared__ __attribute__((aligned(16))) double seq_lds[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // the wave's category
  const int draw = blockIdx.y;
  const int col = blockIdx.x * SEQ_COLS + lane;  // < nblk * 64 <= Ppad
  const int S = a.S, C = a.C, B = a.B, P = a.P;
  const size_t Ppad = (size_t)a.Ppad;
  const int rlen = a.R * 4;
  const double* mdl = a.model + (size_t)draw * (10 + 2 * C);
  const double pi[4] = {mdl[0], mdl[1], mdl[2], mdl[3]};
  const double ps_c = mdl[10 + C + c];
  const double* __restrict__ recs = pmat + ((size_t)draw * C + c) * (size_t)B * rlen;  // this wave's records, by branch
  double* part_ws = a.ws + (size_t)draw * a.ws_draw + (size_t)c * 4 * Ppad + col;
  double* q_ws = part_ws + (size_t)(S - 1) * a.node_stride;
  double* row = a.rows + (size_t)draw * a.row_len;
  double* cat_lds = seq_lds;                             // [C][64]
  double* node_lds = seq_lds + (size_t)C * SEQ_COLS;     // [2][C][4][64]
  const bool live = col < P;

  auto load4 = [&](const double* base, int node, double x[4]) {
    const double* p = base + (size_t)(node - S) * a.node_stride;
#pragma unroll
    for (int s = 0; s < 4; ++s) x[s] = p[(size_t)s * Ppad];
  };
  auto store4 = [&](double* base, int node, const double x[4]) {
    double* p = base + (size_t)(node - S) * a.node_stride;
#pragma unroll
    for (int s = 0; s < 4; ++s) p[(size_t)s * Ppad] = x[s];
  };
  // P_ch part[ch] as the parent sees it: a tip's record vector, an internal
  // child's partial through its matrix, the merged child's partial as it is
  auto moved = [&](int ch, double m[4]) {
    if (ch < S) {
      const unsigned nib = a.tips[(size_t)ch * (Ppad / 2) + (col >> 1)];
      const unsigned vec = (col & 1) ? (nib >> 4) : (nib & 15u);  // < R (pack_tips)
      const double2* r2 = reinterpret_cast<const double2*>(recs + (size_t)ch * rlen + vec * 4);
      const double2 lo = r2[0], hi = r2[1];
      m[0] = lo.x; m[1] = lo.y; m[2] = hi.x; m[3] = hi.y;
    } else {
      double x[4];
      load4(part_ws, ch, x);
      if (ch < B) {
        seq_matvec(recs + (size_t)ch * rlen, x, m);
      } else {
#pragma unroll
        for (int s = 0; s < 4; ++s) m[s] = x[s];
      }
    }
  };

  // forward: part[v] = (P_a part[a]) o (P_b part[b])
  double pv[4] = {0.0, 0.0, 0.0, 0.0};
  for (int st = 0; st < S - 1; ++st) {
    const int ca = steps[st * SEQ_STEP_INTS], cb = steps[st * SEQ_STEP_INTS + 1], v = steps[st * SEQ_STEP_INTS + 2];
    double ma[4], mb[4];
    moved(ca, ma);
    moved(cb, mb);
#pragma unroll
    for (int s = 0; s < 4; ++s) pv[s] = ma[s] * mb[s];
    store4(part_ws, v, pv);
  }
  // root: L_ci = ps_c pi . part[root], L_i their sum in category order
  double Lc = pi[0] * pv[0];
#pragma unroll
  for (int s = 1; s < 4; ++s) Lc = fma(pi[s], pv[s], Lc);
  Lc *= ps_c;
  cat_lds[c * SEQ_COLS + lane] = Lc;
  __syncthreads();
  double L = 0.0;
  for (int cc = 0; cc < C; ++cc) L += cat_lds[cc * SEQ_COLS + lane];
  if (live) row[a.off_cat + (size_t)c * P + col] = Lc / L;
  if (c == 0) {
    double rate = 0.0;
    for (int cc = 0; cc < C; ++cc) rate = fma(mdl[10 + cc], cat_lds[cc * SEQ_COLS + lane] / L, rate);
    if (live) row[a.off_rate + col] = rate;
    a.site[(size_t)draw * Ppad + col] = live ? a.weights[col] * log(L) : 0.0;
  }
  // reverse: anc[v] from part[v] o q[v], then q of v's internal children
  int buf = 0;
  for (int st = S - 2; st >= 0; --st) {
    const int ca = steps[st * SEQ_STEP_INTS], cb = steps[st * SEQ_STEP_INTS + 1], v = steps[st * SEQ_STEP_INTS + 2];
    double qv[4];
    load4(part_ws, v, pv);
    if (st == S - 2) {
#pragma unroll
      for (int s = 0; s < 4; ++s) qv[s] = pi[s];
    } else {
      load4(q_ws, v, qv);
    }
    double* nb = node_lds + (size_t)buf * C * 4 * SEQ_COLS;
#pragma unroll
    for (int s = 0; s < 4; ++s) nb[(c * 4 + s) * SEQ_COLS + lane] = ps_c * (pv[s] * qv[s]);
    __syncthreads();
    for (int s = c; s < 4; s += C) {
      double acc = 0.0;
      for (int cc = 0; cc < C; ++cc) acc += nb[(cc * 4 + s) * SEQ_COLS + lane];
      if (live) row[1 + ((size_t)(v - S) * 4 + s) * P + col] = acc / L;
    }
    buf ^= 1;  // the next node's terms go to the other buffer: a wave is at most one barrier ahead
    if (ca >= S) {  // r_a = q[v] o (P_b part[b]);  q[a] = P_a^T r_a
      double mb[4], r[4], qa[4];
      moved(cb, mb);
#pragma unroll
      for (int s = 0; s < 4; ++s) r[s] = qv[s] * mb[s];
      if (ca < B) {
        seq_matvec_t(recs + (size_t)ca * rlen, r, qa);
        store4(q_ws, ca, qa);
      } else {
        store4(q_ws, ca, r);
      }
    }
    if (cb >= S) {
      double ma[4], r[4], qb[4];
      moved(ca, ma);
#pragma unroll
      for (int s = 0; s < 4; ++s) r[s] = qv[s] * ma[s];
      if (cb < B) {
        seq_matvec_t(recs + (size_t)cb * rlen, r, qb);
        store4(q_ws, cb, qb);
      } else {
        store4(q_ws, cb, r);
      }
    }
  }
}

// row[0] of every draw: the sum of its site terms, thread t over the columns
// t, t + 256, ..., then a tree over the threads: one shape for every call.
__global__ void __launch_bounds__(SEQ_LL_THREADS) seqsum_ll_kernel(const double* __restrict__ site, double* rows, int P,
                                                                   int Ppad, long long row_len) {
  __shared__ double sh[SEQ_LL_THREADS];
  const int draw = blockIdx.x, t = threadIdx.x;
  const double* s = site + (size_t)draw * Ppad;
  double acc = 0.0;
  for (int i = t; i < P; i += SEQ_LL_THREADS) acc += s[i];
  sh[t] = acc;
  __syncthreads();
  for (int h = SEQ_LL_THREADS / 2; h > 0; h >>= 1) {
    if (t < h) sh[t] += sh[t + h];
    __syncthreads();
  }
  if (t == 0) rows[(size_t)draw * row_len] = sh[0];
}

// acc[e] += rows[d][e] over the launch's finite draws d = 0..n-1, in order.
__global__ void __launch_bounds__(SEQ_ACC_THREADS) seqsum_acc_kernel(const double* __restrict__ rows, double* acc, int n,
                                                                     long long row_len) {
  const long long e = (long long)blockIdx.x * SEQ_ACC_THREADS + threadIdx.x;
  if (e >= row_len) return;
  double v = acc[e];
  for (int d = 0; d < n; ++d) {
    const double* r = rows + (size_t)d * row_len;
    if (isfinite(r[0])) v += r[e];
  }
  acc[e] = v;
}

void free_seqsum(phy_seqsum_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->device);
  void* ptrs[] = {c->d_tips, c->d_steps, c->d_matbr, c->d_w,  c->d_pmat, c->d_eig,
                  c->d_model, c->d_blens, c->d_ws,    c->d_rows, c->d_site, c->d_acc};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// n <= draws_per_launch draws on the stream: inputs up, eigensystems, matrix records, the two passes, row[0].
int seqsum_launch(phy_seqsum_ctx* c, int n, const double* blens, const double* model) {
  const SeqsumPlan& sp = c->sp;
  const Problem& pb = sp.pb;
  const int C = pb.C, B = pb.B;
  hipStream_t st = c->stream;
  const size_t ml = 10 + 2 * (size_t)C;
  HIP_TRY(hipMemcpyAsync(c->d_blens, blens, sizeof(double) * n * B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(c->d_model, model, sizeof(double) * n * ml, hipMemcpyHostToDevice, st));
  PmatArgs pa{c->d_model, c->d_blens, c->d_matbr, c->d_eig, c->d_pmat, C, B, pb.kind, pb.nmat, n, pb.R, pb.extra, 0};
  const int rc = launch_matrices(pa, false, st);
  if (rc) return rc;
  SeqArgs a{};
  a.tips = c->d_tips; a.weights = c->d_w; a.model = c->d_model; a.ws = c->d_ws; a.rows = c->d_rows; a.site = c->d_site;
  a.S = pb.S; a.P = pb.P; a.Ppad = pb.Ppad; a.C = C; a.B = B; a.R = pb.R;
  a.row_len = sp.row_len; a.off_cat = sp.off_cat; a.off_rate = sp.off_rate; a.node_stride = sp.node_stride;
  a.ws_draw = sp.ws_draw;
  hipLaunchKernelGGL(seqsum_kernel, dim3(sp.nblk, n), dim3(C * WAVE), sp.lds, st, a, (const int*)c->d_steps,
                     (const double*)c->d_pmat);
  HIP_TRY(hipGetLastError());
  hipLaunchKernelGGL(seqsum_ll_kernel, dim3(n), dim3(SEQ_LL_THREADS), 0, st, (const double*)c->d_site, c->d_rows, pb.P,
                     pb.Ppad, sp.row_len);
  HIP_TRY(hipGetLastError());
  return PHY_OK;
}

}  // namespace

extern "C" {

int phy_seqsum_create(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                      const int32_t* peel, int max_draws, int device, phy_seqsum_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  std::unique_ptr<phy_seqsum_ctx, void (*)(phy_seqsum_ctx*)> c(new phy_seqsum_ctx(), free_seqsum);
  int rc = seqsum_plan(S, P, C, rooted, model, tipcodes, weights, peel, max_draws, c->sp);
  if (rc) return rc;
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  hipError_t he = hipSetDevice(device);
  if (he != hipSuccess) return fail(PHY_EHIP, std::string("hipSetDevice: ") + hipGetErrorString(he));
  c->device = device;
  c->max_draws = max_draws;
  const SeqsumPlan& sp = c->sp;
  const Problem& pb = sp.pb;
  (void)hipFuncSetAttribute((const void*)seqsum_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS_CAP);
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t L = (size_t)sp.draws_per_launch, ml = 10 + 2 * (size_t)C;
  if ((rc = dalloc(&c->d_tips, (size_t)S * pb.Ppad / 2)) || (rc = dalloc(&c->d_w, (size_t)pb.Ppad)) ||
      (rc = dalloc(&c->d_steps, sp.steps.size())) || (rc = dalloc(&c->d_matbr, (size_t)pb.B)) ||
      (rc = dalloc(&c->d_pmat, L * C * pb.nmat * pb.R * 4)) || (rc = dalloc(&c->d_eig, L * EIG_LEN)) ||
      (rc = dalloc(&c->d_model, L * ml)) || (rc = dalloc(&c->d_blens, L * pb.B)) ||
      (rc = dalloc(&c->d_ws, L * (size_t)sp.ws_draw)) || (rc = dalloc(&c->d_rows, L * (size_t)sp.row_len)) ||
      (rc = dalloc(&c->d_site, L * (size_t)pb.Ppad)) || (rc = dalloc(&c->d_acc, (size_t)sp.row_len)))
    return rc;
  {
    std::vector<int> ident(pb.B);
    for (int b = 0; b < pb.B; ++b) ident[b] = b;  // matrix m is branch m
    if ((rc = upload_alignment(c->d_tips, c->d_w, pb)) || (rc = upload(c->d_steps, sp.steps)) ||
        (rc = upload(c->d_matbr, ident)))
      return rc;
  }
  // on the context's own stream, which does not wait for the null stream
  HIP_TRY(hipMemsetAsync(c->d_acc, 0, sizeof(double) * (size_t)sp.row_len, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  *out = c.release();
  return PHY_OK;
}

int phy_seqsum_destroy(phy_seqsum_ctx* ctx) {
  free_seqsum(ctx);
  return PHY_OK;
}

int phy_seqsum_num_branches(const phy_seqsum_ctx* ctx) { return ctx ? ctx->sp.pb.B : -1; }
int phy_seqsum_row_len(const phy_seqsum_ctx* ctx) { return ctx ? (int)ctx->sp.row_len : -1; }

int phy_seqsum_plan(int S, int P, int C, int rooted, int model, const uint8_t* tipcodes, const double* weights,
                    const int32_t* peel, int max_draws, long long* facts, int32_t* order) {
  g_err.clear();
  SeqsumPlan sp;
  const int rc = seqsum_plan(S, P, C, rooted, model, tipcodes, weights, peel, max_draws, sp);
  if (rc) return rc;
  if (facts) {
    const long long fv[8] = {sp.row_len, sp.pb.Ppad, sp.nblk, sp.ws_draw * 8, sp.draw_bytes, sp.draws_per_launch,
                             (long long)sp.lds, sp.pb.R};
    std::copy(fv, fv + 8, facts);
  }
  if (order)
    for (int s = 0; s < S - 1; ++s) order[s] = sp.steps[(size_t)s * SEQ_STEP_INTS + 2];
  return PHY_OK;
}

int phy_seqsum_eval(phy_seqsum_ctx* ctx, int n_draws, const double* blens, const double* model, double* rows) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (!blens || !model || !rows) return fail(PHY_EINVAL, "NULL host buffer");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, "n_draws out of range (1..max_draws)");
  HIP_TRY(hipSetDevice(ctx->device));
  const SeqsumPlan& sp = ctx->sp;
  const size_t rl = (size_t)sp.row_len, ml = 10 + 2 * (size_t)sp.pb.C, B = (size_t)sp.pb.B;
  for (int lo = 0; lo < n_draws; lo += sp.draws_per_launch) {
    const int n = std::min(sp.draws_per_launch, n_draws - lo);
    int rc = seqsum_launch(ctx, n, blens + lo * B, model + lo * ml);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(rows + lo * rl, ctx->d_rows, sizeof(double) * n * rl, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  reject_rows(rows, (size_t)n_draws, rl);
  return PHY_OK;
}

int phy_seqsum_reset(phy_seqsum_ctx* ctx) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemsetAsync(ctx->d_acc, 0, sizeof(double) * (size_t)ctx->sp.row_len, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  ctx->n_finite = 0;
  return PHY_OK;
}

int phy_seqsum_add(phy_seqsum_ctx* ctx, int n_draws, const double* blens, const double* model, double* loglik) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (!blens || !model || !loglik) return fail(PHY_EINVAL, "NULL host buffer");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, "n_draws out of range (1..max_draws)");
  HIP_TRY(hipSetDevice(ctx->device));
  const SeqsumPlan& sp = ctx->sp;
  const size_t rl = (size_t)sp.row_len, ml = 10 + 2 * (size_t)sp.pb.C, B = (size_t)sp.pb.B;
  const unsigned agrid = (unsigned)((sp.row_len + SEQ_ACC_THREADS - 1) / SEQ_ACC_THREADS);
  for (int lo = 0; lo < n_draws; lo += sp.draws_per_launch) {
    const int n = std::min(sp.draws_per_launch, n_draws - lo);
    int rc = seqsum_launch(ctx, n, blens + lo * B, model + lo * ml);
    if (rc) return rc;
    hipLaunchKernelGGL(seqsum_acc_kernel, dim3(agrid), dim3(SEQ_ACC_THREADS), 0, ctx->stream,
                       (const double*)ctx->d_rows, ctx->d_acc, n, sp.row_len);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(loglik + lo, sizeof(double), ctx->d_rows, sizeof(double) * rl, sizeof(double), (size_t)n,
                             hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(hipStreamSynchronize(ctx->stream));
  }
  for (int d = 0; d < n_draws; ++d) {
    if (std::isfinite(loglik[d])) ++ctx->n_finite;
    else loglik[d] = -INFINITY;
  }
  return PHY_OK;
}

int phy_seqsum_read(phy_seqsum_ctx* ctx, double* row, int* n_finite) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (!row) return fail(PHY_EINVAL, "NULL host buffer");
  HIP_TRY(hipSetDevice(ctx->device));
  HIP_TRY(hipMemcpyAsync(row, ctx->d_acc, sizeof(double) * (size_t)ctx->sp.row_len, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(hipStreamSynchronize(ctx->stream));
  if (n_finite) *n_finite = (int)ctx->n_finite;
  return PHY_OK;
}

}  // extern "C"
