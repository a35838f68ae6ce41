// kseq_engine.inc -- the K-state sequence likelihood on the device: an
// alignment of P patterns under a mixture over sites of M reversible models of
// 2 <= K <= 64 states (codon models are K = 61), each with C rate categories:
// L_i = sum_m sum_c ps[m][c] L_i(Q_m, t rs[m][c], pi_m).  log L with its full
// gradient, the site log-likelihoods and the components' posterior
// probabilities per pattern.  phy_kseq_* is the M = 1 case of the same kernels
// (phy_kseq_mix_* at M = 1 returns its bits); g = m C + c runs over G = M C.
// Included by phylo_hip.hip after geo_trees.inc,
// whose eigen / tree / combine structure it follows; phylostan_amd/kseq.py's
// kseq_host is the same derivation in numpy.  All fp64.
//
// Per chunk of draws (kseq_plan.h: every length and offset comes from there):
//   1. kseq_eig_kernel, one workgroup per (draw, component): geo_params_ok (rs,
//      ps and the
//      branch lengths join the refusal sum), geo_q_scale, geo_jacobi, then
//      kseq_polish (V re-orthogonalised, lam as Rayleigh quotients); the record
//      ok, sweeps, s, lam, qd, V, sqrt(pi), 1/sqrt(pi).  It runs once per call,
//      over all its draws; a draw's M eigensolves run side by side.
//   2. kseq_up_kernel, one (draw, g, tile of 16 patterns) item per
//      workgroup of KT / 16 waves: the whole tree, row by row, for the tile.
//      Per child c = V^T (sqrt(pi) o x) and msg = x + (V (em o c)) / sqrt(pi),
//      em = expm1(lam t): P(t) x as x + (P(t) - I) x, because V V^T is the
//      identity to 1e-16 only, 1e-16 / (q t) of a transition probability q t
//      on a short branch; at t = 0 the message is x.  Then the
//      product of the two messages, the per-column power-of-two rescale; the
//      scaled lower partial, c, msg and the column factors go to the item's
//      workspace, L_g and the column's total shift to the chunk's [G][PP] arrays.
//      An item reads the record and freqs of its own component m = g / C.
//      msg is stored, not recomputed on the way down: the workspace of the
//      fluA codon shape is 3.4 MB an item with it and 2.2 MB without, 4 or 6
//      draws in flight under the budget, and recomputing would add two of the
//      way down's five products per branch.
//   3. kseq_site_kernel, one workgroup per draw: shmin over the live g, rel,
//      (0 for a category that is not alive and lies more than KSEQ_DEAD_BELOW
//      bits under shmin), L_i, site log L, log L, the bad-draw verdict, w_i /
//      L_i and, when asked,
//      the components' posteriors from the ps L rel terms on that shared shift.
//   4. kseq_down_kernel, the same items in reverse row order: u~, a = V^T (u~ /
//      sqrt(pi)), G = sum a lam e c, the downward vector u~ + sqrt(pi) (V (em o
//      a)) (it overwrites the node's lower partial, which nothing reads again),
//      the two dvec terms as (up - u~) . low and u~ . (msg - low), rootpi, and
//      W += (a c^T) o Phi in registers (Phi's quotient of em_k - em_l, which
//      does not cancel where both exponentials are near 1): a wave holds
//      its 16 rows of W, 4 x KT / 16 doubles a lane.  Everything leaves in the
//      item's slot; no atomics.
//   5. kseq_combine_kernel, one workgroup per (draw, component): the
//      component's slots in ascending (category, tile) order, geo_sym_vwvt,
//      geo_chain_rule into its d/drates and d/dfreqs blocks, its root term.
//      Component 0's workgroup also folds d/dblens = sum_g r_g G_b in ascending
//      g (component, then category), tile innermost, and writes d/drs, d/dps.
// A draw any of whose M records is not ok is skipped by phases 2 to 5.
//
// The five products go through v_mfma_f64_16x16x4_f64, one wave per 16-row
// block of the output: kseq_mm_vt (V^T X), kseq_mm_v (V X) and kseq_mm_outer
// (X Y^T).  Operand maps: lane l holds A[row l & 15][k l >> 4] and B[k l >> 4]
// [col l & 15]; the result's register r is D[row (l >> 4) + 4 r][col l & 15].
// The elementwise steps between the products run on that result layout, so a
// lane multiplies its own four entries of two messages without a shuffle.
// Padded states (K .. KT - 1) are zero in V, sqrt(pi), 1/sqrt(pi) and the tips,
// hence zero in every product: they never win a column's maximum.
//
// Every sum has one order that depends on the shape alone: a draw's row and
// site_ll and class_post are bitwise the same alone, in any batch, in any chunk
// and on repeat.

typedef double kseq_v4d __attribute__((ext_vector_type(4)));

struct KseqArgs {
  const uint64_t* masks;  // [ntiles][S][16]
  const double* tile_w;   // [PP]
  const int* rows;        // [S-1][KR_INTS]
  const double* blens;    // [n][B]
  const double* params;   // [n][param_len]
  double* rec;            // [n][M][rec_doubles]
  double* ws;             // [chunk items][ws_doubles]
  double* slots;          // [chunk items][slot_doubles]
  double* lc;             // [chunk][G][PP] L_g
  double* sh;             // [chunk][G][PP] the column's shift; after the site phase rel = 2^-(shift - shmin)
  double* down0;          // [chunk][PP] w_i / L_i
  double* out;            // [n][row_len]
  double* site;           // [n][P]
  double* cpost;          // [n][M][P], or NULL when the call did not ask
  int S, P, K, M, C, G, B, N, KT, NB, ntiles, PP, n;
  int draw0, ndraw;
};

// ---- the three operand arrangements.  V: KT x KT, rows VS apart; X, Y: KT x 16, rows KSEQ_XS apart.
// D[16 w + .][.] of V^T X
__device__ __forceinline__ kseq_v4d kseq_mm_vt(const double* V, int VS, const double* X, int KT, int w, int lane) {
  const int g = lane >> 4, cl = lane & 15;
  kseq_v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int j0 = 0; j0 < KT; j0 += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(V[(j0 + g) * VS + 16 * w + cl], X[(j0 + g) * KSEQ_XS + cl], acc, 0, 0,
                                               0);
  return acc;
}
// D[16 w + .][.] of V X
__device__ __forceinline__ kseq_v4d kseq_mm_v(const double* V, int VS, const double* X, int KT, int w, int lane) {
  const int g = lane >> 4, cl = lane & 15;
  kseq_v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int k0 = 0; k0 < KT; k0 += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(V[(16 * w + cl) * VS + k0 + g], X[(k0 + g) * KSEQ_XS + cl], acc, 0, 0,
                                               0);
  return acc;
}
// the 16 x 16 block (w, lb) of X Y^T
__device__ __forceinline__ kseq_v4d kseq_mm_outer(const double* X, const double* Y, int w, int lb, int lane) {
  const int g = lane >> 4, cl = lane & 15;
  kseq_v4d acc = {0.0, 0.0, 0.0, 0.0};
  for (int p0 = 0; p0 < KSEQ_PT; p0 += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(X[(16 * w + cl) * KSEQ_XS + p0 + g],
                                               Y[(16 * lb + cl) * KSEQ_XS + p0 + g], acc, 0, 0, 0);
  return acc;
}

// One item's pointers: the LDS of KseqLds and its workspace block.
struct KseqView {
  int K, KT, VS, S, N;
  double *V, *X0, *X1, *X2, *X3, *lam, *sq, *isq, *pi, *ev, *em, *red, *col, *RT;
  double *LOW, *CC, *MSG, *SF;
  const uint64_t* masks;  // the tile's [S][16]
  __device__ __forceinline__ KseqView(double* shm, const KseqArgs& a, double* wsb, int tile)
      : K(a.K), KT(a.KT), S(a.S), N(a.N) {
    const KseqLds L(a.KT);
    VS = L.VS;
    V = shm + L.V(), X0 = shm + L.X(0), X1 = shm + L.X(1), X2 = shm + L.X(2), X3 = shm + L.X(3);
    lam = shm + L.vecs(0), sq = shm + L.vecs(1), isq = shm + L.vecs(2), pi = shm + L.vecs(3), ev = shm + L.vecs(4);
    em = shm + L.vecs(5);
    red = shm + L.red(), col = shm + L.col(), RT = shm + L.RT();
    LOW = wsb + kseq_ws_low(N, KT), CC = wsb + kseq_ws_cc(N, KT), MSG = wsb + kseq_ws_msg(N, KT);
    SF = wsb + kseq_ws_sf(N, KT);
    masks = a.masks + kseq_mask_at(tile, 0, a.S);
  }
  // entry (i, col) of a node's lower partial: a tip's from its mask
  __device__ __forceinline__ double low(int node, int i, int cl) const {
    if (node < S) return ((masks[(size_t)node * KSEQ_PT + cl] >> i) & 1) ? 1.0 : 0.0;
    return LOW[(size_t)node * kseq_blk(KT) + i * KSEQ_PT + cl];
  }
};

// every component of the draw has its eigensystem (uniform: the records were written by an earlier kernel)
__device__ __forceinline__ bool kseq_draw_ok(const KseqArgs& a, int draw) {
  bool ok = true;
  for (int m = 0; m < a.M; ++m) ok = ok && a.rec[kseq_rec_at(draw, m, a.M, a.K) + KREC_OK] != 0.0;
  return ok;
}

// V, lam, sqrt(pi), 1/sqrt(pi), pi of the item's component into LDS, zero on the padding.  No barrier on exit.
__device__ __forceinline__ void kseq_load_draw(const KseqView& v, const double* rec, const double* freqs) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KT = v.KT;
  const double* rV = rec + kseq_rec_v(K);
  for (int it = tid; it < KT * KT; it += nt) {
    const int i = it / KT, j = it - i * KT;
    v.V[i * v.VS + j] = (i < K && j < K) ? rV[i * K + j] : 0.0;
  }
  for (int i = tid; i < KT; i += nt) {
    const bool in = i < K;
    v.lam[i] = in ? rec[kseq_rec_lam(K) + i] : 0.0;
    v.sq[i] = in ? rec[kseq_rec_sq(K) + i] : 0.0;
    v.isq[i] = in ? rec[kseq_rec_isq(K) + i] : 0.0;
    v.pi[i] = in ? freqs[i] : 0.0;
  }
}

// The eigensystem polished after geo_jacobi: V <- V (3 I - V^T V) / 2 (one Newton-Schulz step: V^T V - I goes from
// delta to 3 delta^2 / 4), then lam_k = v_k^T A v_k on the rebuilt A, into v.dd.  The sweeps' rotations leave V^T V
// - I near 5e-14 at K = 61 (a numpy restatement of geo_jacobi on the tied codon case: 15 sweeps of 1830 rotations);
// a transition probability over three nucleotide changes is near 1e-5, and sum_k V_ik e_k V_jk reaches it by
// cancellation, so that loss alone put a site's log L 1.6e-10 from the truth on that case (the bar is 1e-10;
// LAPACK's eigh on the host: 2.8e-11; with the step: 1.5e-13).  3 K^3 multiply-adds beside sweeps of 1.6 ms.
// Barriers: geo_jacobi's exit on entry; V and dd synchronised on exit.  A and W are spent.
constexpr double KSEQ_POLISH_ABOVE = 4.0 * 2.220446049250313e-16;
__device__ __forceinline__ void kseq_polish(const GeoView& v, const double* rates, double s) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  double *A = v.A, *V = v.V, *W = v.W;
  for (int it = tid; it < K * K; it += nt) {  // W = V^T V
    const int k = it / K, l = it - k * K;
    double acc = 0.0;
    for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k], V[i * KP + l], acc);
    W[k * KP + l] = acc;
  }
  // A V within four ulps of orthonormal is left alone, with the sweeps' lam: the step could only add its own
  // rounding, and an exact zero of sum_k V_ik V_jk (K = 2: c s - s c, the likelihood of a pattern no path reaches)
  // stays an exact zero.
  double far = 0.0;
  for (int it = tid; it < K * K; it += nt) {
    const int k = it / K, l = it - k * K;
    far += fabs(W[k * KP + l] - (k == l ? 1.0 : 0.0)) > KSEQ_POLISH_ABOVE ? 1.0 : 0.0;  // own entries: no barrier
  }
  if (geo_block_sum(far, v.red, tid, nt) == 0.0) {
    for (int i = tid; i < K; i += nt) v.dd[i] = A[i * KP + i];
    __syncthreads();
    return;
  }
  for (int it = tid; it < K * K; it += nt) {  // A = 1.5 V - 0.5 V W
    const int i = it / K, l = it - i * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = fma(V[i * KP + k], W[k * KP + l], acc);
    A[i * KP + l] = 1.5 * V[i * KP + l] - 0.5 * acc;
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {  // V = that; W = the matrix the sweeps started from
    const int i = it / K, j = it - i * K;
    V[i * KP + j] = A[i * KP + j];
    W[i * KP + j] = i == j ? v.qd[i] / s : geo_a_entry(v, rates, s, i, j);
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {  // A = W V
    const int i = it / K, k = it - i * K;
    double acc = 0.0;
    for (int j = 0; j < K; ++j) acc = fma(W[i * KP + j], V[j * KP + k], acc);
    A[i * KP + k] = acc;
  }
  __syncthreads();
  for (int k = tid; k < K; k += nt) {
    double acc = 0.0;
    for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k], A[i * KP + k], acc);
    v.dd[k] = acc;
  }
  __syncthreads();
}

// ---- phase 1: the eigensystem of one (draw, component), to the record
__device__ bool kseq_eigen(const KseqArgs& a, int draw, int m, double* shm, double* rec) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K;
  const GeoView v(shm, K);
  const double* par = a.params + (size_t)draw * kseq_mix_param_len(K, a.M, a.C);
  const double* rates = par + kseq_mix_par_comp(K, m);
  const double* freqs = rates + kseq_par_freqs(K);
  const double* rsps = par + kseq_mix_par_rs(K, a.M);  // rs then ps, all G of each: any component refuses for them
  const double* bl = a.blens + (size_t)draw * a.B;
  double bad = 0.0;
  for (int i = tid; i < 2 * a.G; i += nt) bad += (rsps[i] >= 0.0 && isfinite(rsps[i])) ? 0.0 : 1.0;
  for (int b = tid; b < a.B; b += nt) bad += isfinite(bl[b]) ? 0.0 : 1.0;
  if (!geo_params_ok(v, rates, freqs, bad)) return false;
  for (int i = tid; i < K; i += nt) {
    const double f = freqs[i];
    v.pi[i] = f;
    v.sq[i] = sqrt(f);
  }
  const double s = geo_q_scale(v, rates);
  if (!(s > 0.0) || !isfinite(s)) return false;
  int sweeps;
  const bool converged = geo_jacobi(v, rates, s, sweeps);
  if (tid == 0) rec[KREC_SWEEPS] = (double)sweeps, rec[KREC_S] = s;
  if (!converged) return false;
  kseq_polish(v, rates, s);
  double* rV = rec + kseq_rec_v(K);
  for (int i = tid; i < K; i += nt) {
    rec[kseq_rec_lam(K) + i] = v.dd[i];
    rec[kseq_rec_qd(K) + i] = v.qd[i];
    rec[kseq_rec_sq(K) + i] = v.sq[i];
    rec[kseq_rec_isq(K) + i] = 1.0 / v.sq[i];
  }
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    rV[it] = v.V[i * v.KP + j];
  }
  return true;
}

__global__ void __launch_bounds__(GEO_MAX_THREADS) kseq_eig_kernel(KseqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  for (int dm = blockIdx.x; dm < a.n * a.M; dm += gridDim.x) {
    const int draw = dm / a.M, m = dm - draw * a.M;
    double* rec = a.rec + kseq_rec_at(draw, m, a.M, a.K);
    if (threadIdx.x == 0) rec[KREC_SWEEPS] = -1.0, rec[KREC_S] = 0.0, rec[KREC_BAD] = 1.0, rec[KREC_LL] = -INFINITY;
    const bool ok = kseq_eigen(a, draw, m, shm, rec);
    __syncthreads();  // LDS is free for the next solve
    if (threadIdx.x == 0) rec[KREC_OK] = ok ? 1.0 : 0.0;
  }
}

// ---- phase 2: the way up of one item
__device__ void kseq_up_item(const KseqArgs& a, int dl, int gc, int tile, double* shm, double* wsb) {
  const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int K = a.K, KT = a.KT, S = a.S, draw = a.draw0 + dl;
  const KseqView v(shm, a, wsb, tile);
  const int m = gc / a.C;  // the item's component
  const double* par = a.params + (size_t)draw * kseq_mix_param_len(K, a.M, a.C);
  const double* rec = a.rec + kseq_rec_at(draw, m, a.M, K);
  const double* bl = a.blens + (size_t)draw * a.B;
  double* lcp = a.lc + kseq_lc_at(dl, gc, a.G, a.PP) + (size_t)tile * KSEQ_PT;
  double* shp = a.sh + kseq_lc_at(dl, gc, a.G, a.PP) + (size_t)tile * KSEQ_PT;
  const size_t blk = kseq_blk(KT);
  __syncthreads();  // the previous item's readers of LDS are done
  if (!kseq_draw_ok(a, draw)) {  // an eigensystem is missing: the site phase refuses the draw
    if (tid < KSEQ_PT) lcp[tid] = 0.0, shp[tid] = 0.0;
    return;
  }
  kseq_load_draw(v, rec, par + kseq_mix_par_comp(K, m) + kseq_par_freqs(K));
  const double rc = par[kseq_mix_par_rs(K, a.M) + gc];
  const double small = ldexp(1.0, GEO_SCALE_BELOW);
  int shift_tot = 0;  // of column cl
  for (int r = 0; r < S - 1; ++r) {
    const int* row = a.rows + (size_t)r * KR_INTS;
    const int ca = row[KR_A], cb = row[KR_B], p = row[KR_P], fold = row[KR_FOLD];
    kseq_v4d m[2];
    for (int which = 0; which < 2; ++which) {
      if (which && fold) break;
      const int ch = which ? cb : ca;
      const double t = bl[ch] * rc;
      __syncthreads();  // X0, X1, em are free; the lower partial of ch is written
      for (int it = tid; it < KT * KSEQ_PT; it += nt) {
        const int i = it >> 4, col = it & 15;
        v.X0[i * KSEQ_XS + col] = v.sq[i] * v.low(ch, i, col);
      }
      for (int i = tid; i < KT; i += nt) v.em[i] = expm1(v.lam[i] * t);
      __syncthreads();
      const kseq_v4d cc = kseq_mm_vt(v.V, v.VS, v.X0, KT, wave, lane);
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * wave + g + 4 * q;
        v.CC[(size_t)ch * blk + i * KSEQ_PT + cl] = cc[q];
        v.X1[i * KSEQ_XS + cl] = v.em[i] * cc[q];
      }
      __syncthreads();
      kseq_v4d ms = kseq_mm_v(v.V, v.VS, v.X1, KT, wave, lane);
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * wave + g + 4 * q;
        ms[q] = v.low(ch, i, cl) + ms[q] * v.isq[i];  // x + (P - I) x; this lane wrote that entry of an internal ch
        v.MSG[(size_t)ch * blk + i * KSEQ_PT + cl] = ms[q];
      }
      m[which] = ms;
    }
    double x[4];
    double mx = 0.0;
    for (int q = 0; q < 4; ++q) {
      const int i = 16 * wave + g + 4 * q;
      x[q] = m[0][q] * (fold ? v.low(cb, i, cl) : m[1][q]);
      mx = q == 0 ? x[0] : fmax(mx, x[q]);
    }
    // the column's maximum: the lane's four registers, the four lane groups, the row blocks
    mx = fmax(mx, __shfl_xor(mx, 16));
    mx = fmax(mx, __shfl_xor(mx, 32));
    if (g == 0) v.red[wave * KSEQ_PT + cl] = mx;
    __syncthreads();
    mx = v.red[cl];
    for (int w = 1; w < a.NB; ++w) mx = fmax(mx, v.red[w * KSEQ_PT + cl]);
    int shift = 0;
    double fac = 1.0;
    if (mx > 0.0 && mx < small) {
      shift = -ilogb(mx);
      if (shift > GEO_SHIFT_MAX) shift = GEO_SHIFT_MAX;
      fac = ldexp(1.0, shift);
    }
    shift_tot += shift;
    const bool last = r == S - 2;
    for (int q = 0; q < 4; ++q) {
      const int i = 16 * wave + g + 4 * q;
      x[q] *= fac;
      v.LOW[(size_t)p * blk + i * KSEQ_PT + cl] = x[q];
      if (last) v.X0[i * KSEQ_XS + cl] = x[q];  // X0's readers passed two barriers
    }
    if (wave == 0 && g == 0) v.SF[(size_t)p * KSEQ_PT + cl] = fac;
    if (last) {  // L_g = pi . low(root), state by state in ascending order
      __syncthreads();
      if (tid < KSEQ_PT) {
        double acc = 0.0;
        for (int i = 0; i < K; ++i) acc = fma(v.pi[i], v.X0[i * KSEQ_XS + tid], acc);
        lcp[tid] = acc;
        shp[tid] = (double)shift_tot;  // tid < 16: cl == tid
      }
    }
  }
}

__global__ void __launch_bounds__(256) kseq_up_kernel(KseqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  const size_t wslen = kseq_ws_doubles(a.N, a.KT);
  const int per_draw = a.G * a.ntiles, items = a.ndraw * per_draw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int dl = item / per_draw, rem = item - dl * per_draw, gc = rem / a.ntiles, tile = rem - gc * a.ntiles;
    kseq_up_item(a, dl, gc, tile, shm, a.ws + kseq_item(dl, gc, tile, a.G, a.ntiles) * wslen);
  }
}

// ---- phase 3: the sites of one draw
constexpr double KSEQ_DEAD_BELOW = 900.0;  // kseq.py's DEAD_BELOW
__global__ void __launch_bounds__(KSEQ_SITE_THREADS) kseq_site_kernel(KseqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* red = reinterpret_cast<double*>(geo_smem) + GeoLds(a.K).red();
  const int tid = threadIdx.x, nt = blockDim.x, K = a.K, M = a.M, G = a.G, PP = a.PP;
  for (int dl = blockIdx.x; dl < a.ndraw; dl += gridDim.x) {
    const int draw = a.draw0 + dl;
    double* rec = a.rec + kseq_rec_at(draw, 0, M, K);  // the verdict goes to component 0's
    double* site = a.site + (size_t)draw * a.P;
    double* cpost = a.cpost ? a.cpost + kseq_cpost_at(draw, 0, M, a.P) : nullptr;
    if (!kseq_draw_ok(a, draw)) {
      for (int i = tid; i < a.P; i += nt) site[i] = -INFINITY;
      if (cpost)
        for (int i = tid; i < M * a.P; i += nt) cpost[i] = 0.0;
      continue;
    }
    const double* ps = a.params + (size_t)draw * kseq_mix_param_len(K, M, a.C) + kseq_mix_par_ps(K, M, a.C);
    const double* lc = a.lc + kseq_lc_at(dl, 0, G, PP);
    double* sh = a.sh + kseq_lc_at(dl, 0, G, PP);
    double* down0 = a.down0 + kseq_down0_at(dl, PP);
    double bad = 0.0, ll = 0.0;
    for (int i = tid; i < PP; i += nt) {
      double shmin = INFINITY;
      for (int c = 0; c < G; ++c)
        if (lc[(size_t)c * PP + i] > 0.0 && ps[c] > 0.0) shmin = fmin(shmin, sh[(size_t)c * PP + i]);
      if (!isfinite(shmin)) shmin = 0.0;
      double Ls = 0.0;
      for (int c = 0; c < G; ++c) {
        const double l = lc[(size_t)c * PP + i];
        const double d = sh[(size_t)c * PP + i] - shmin;  // integers; >= 0 for a live category
        const bool alive = l > 0.0 && ps[c] > 0.0;
        // A category that is not alive (L_g = 0 exactly, the +I category at a variable pattern, or ps_g = 0) can lie
        // any distance under shmin, and 2^1024 is inf, which the way down would multiply by its zeros: past
        // KSEQ_DEAD_BELOW bits it takes no part; the exponent stays within KSEQ_DEAD_BELOW.
        const double rel = (!alive && d < -KSEQ_DEAD_BELOW)
                               ? 0.0
                               : ldexp(1.0, -(int)fmin(fmax(d, -KSEQ_DEAD_BELOW), KSEQ_DEAD_BELOW));
        if (alive) Ls += ps[c] * l * rel;
        sh[(size_t)c * PP + i] = rel;
      }
      const double w = a.tile_w[i];
      const bool pos = Ls > 0.0 && isfinite(Ls);
      const double sl = Ls > 0.0 ? log(Ls) - shmin * 0.693147180559945309417232121458 : -INFINITY;
      if (w > 0.0) {
        if (!pos) bad += 1.0;
        ll += w * sl;
      }
      down0[i] = (w > 0.0 && Ls > 0.0) ? w / Ls : 0.0;
      if (i < a.P) site[i] = sl;
      if (cpost && i < a.P)  // sum_c ps L rel of each component over L_i: the terms of Ls, on the shared shift
        for (int m = 0; m < M; ++m) {
          double Lm = 0.0;
          for (int c = m * a.C; c < (m + 1) * a.C; ++c) {
            const double l = lc[(size_t)c * PP + i];
            if (l > 0.0 && ps[c] > 0.0) Lm += ps[c] * l * sh[(size_t)c * PP + i];
          }
          cpost[(size_t)m * a.P + i] = pos ? Lm / Ls : 0.0;
        }
    }
    bad = geo_block_sum(bad, red, tid, nt);
    ll = geo_block_sum(ll, red, tid, nt);
    const bool dead = bad != 0.0 || !isfinite(ll);
    if (tid == 0) rec[KREC_BAD] = dead ? 1.0 : 0.0, rec[KREC_LL] = dead ? -INFINITY : ll;
    if (dead) {
      for (int i = tid; i < a.P; i += nt) site[i] = -INFINITY;
      if (cpost)
        for (int i = tid; i < M * a.P; i += nt) cpost[i] = 0.0;
    }
    __syncthreads();
  }
}

// ---- phase 4: the way down of one item.  SUM (kseq_sum.inc) is the summaries' form of the same walk: it seeds
// with ps rel / L_i at every pattern with a likelihood (weight zero included), leaves each node's posterior share
// up o low in the node's CC block (read for the last time on the node's own branch; the root's and the merged
// child's are never written on the way up), puts w_i on the c operand of a c^T, and in place of the fold into W
// contracts (a c^T) o Phi with the NL tables blab [NL][KT][KT] into slot [NL][B].  It keeps no gradient term.
// The plain form takes blab = nullptr, NL = 0 and is the code it was.
template <bool SUM>
__device__ void kseq_down_item(const KseqArgs& a, int dl, int gc, int tile, double* shm, double* wsb, double* slot,
                               const double* blab, int NL) {
  const int tid = threadIdx.x, nt = blockDim.x, wave = tid >> 6, lane = tid & 63, g = lane >> 4, cl = lane & 15;
  const int K = a.K, KT = a.KT, S = a.S, NB = a.NB, draw = a.draw0 + dl, root = 2 * S - 2;
  const KseqView v(shm, a, wsb, tile);
  const int m = gc / a.C;  // the item's component
  const double* par = a.params + (size_t)draw * kseq_mix_param_len(K, a.M, a.C);
  const double* rec = a.rec + kseq_rec_at(draw, m, a.M, K);
  const double* bl = a.blens + (size_t)draw * a.B;
  const size_t blk = kseq_blk(KT);
  __syncthreads();  // the previous item's readers of LDS are done
  // a bad draw: the combine phase reads no slot of it
  if (!kseq_draw_ok(a, draw) || a.rec[kseq_rec_at(draw, 0, a.M, K) + KREC_BAD] != 0.0) return;
  kseq_load_draw(v, rec, par + kseq_mix_par_comp(K, m) + kseq_par_freqs(K));
  const double rc = par[kseq_mix_par_rs(K, a.M) + gc], psc = par[kseq_mix_par_ps(K, a.M, a.C) + gc];
  if (tid < KSEQ_PT) {
    const size_t at = kseq_lc_at(dl, gc, a.G, a.PP) + (size_t)tile * KSEQ_PT + tid;
    if constexpr (SUM) {  // L_i again from the site phase's terms ps L rel, in its order; the weight apart
      const double* ps = par + kseq_mix_par_ps(K, a.M, a.C);
      double Ls = 0.0;
      for (int c = 0; c < a.G; ++c) {
        const size_t ac = kseq_lc_at(dl, c, a.G, a.PP) + (size_t)tile * KSEQ_PT + tid;
        const double l = a.lc[ac];
        if (l > 0.0 && ps[c] > 0.0) Ls += ps[c] * l * a.sh[ac];
      }
      v.col[tid] = (Ls > 0.0 && isfinite(Ls)) ? a.sh[at] / Ls * psc : 0.0;
      v.col[KSEQ_PT + tid] = a.tile_w[(size_t)tile * KSEQ_PT + tid];
    } else {
      const double d = a.down0[kseq_down0_at(dl, a.PP) + (size_t)tile * KSEQ_PT + tid] * a.sh[at];
      v.col[tid] = d * psc;
      v.col[KSEQ_PT + tid] = d * a.lc[at];
    }
  }
  __syncthreads();
  for (int it = tid; it < KT * KT; it += nt) {  // 1 / (lam_k - lam_l), 0 inside the near window and on the padding
    const int k = it / KT, l = it - k * KT;
    v.RT[k * v.VS + l] = (k < K && l < K) ? phi_rinv(v.lam[k], v.lam[l], PHI_NEAR) : 0.0;
  }
  double grs = 0.0;  // thread 0's
  if constexpr (!SUM) {
    if (tid == 0) {
      double acc = 0.0;
      for (int i = 0; i < KSEQ_PT; ++i) acc += v.col[KSEQ_PT + i];
      slot[kseq_slot_gps(KT, a.B)] = acc;
    }
  }
  kseq_v4d W[4];
  for (int lb = 0; lb < 4; ++lb) W[lb] = kseq_v4d{0.0, 0.0, 0.0, 0.0};
  double dv[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = S - 2; r >= 0; --r) {
    const int* row = a.rows + (size_t)r * KR_INTS;
    const int ca = row[KR_A], cb = row[KR_B], p = row[KR_P], fold = row[KR_FOLD];
    double ut[2][4], ma[4], mb[4];
    __syncthreads();  // X0's readers are done; RT and col are written
    for (int q = 0; q < 4; ++q) {
      const int i = 16 * wave + g + 4 * q;
      const size_t e = (size_t)i * KSEQ_PT + cl;
      double upp;
      if (p == root) {  // the root's upward vector, and its row for d/dfreqs
        upp = v.col[cl] * v.pi[i];
        if constexpr (SUM)
          v.CC[(size_t)p * blk + e] = upp * v.LOW[(size_t)p * blk + e];  // the root's share
        else
          v.X0[i * KSEQ_XS + cl] = v.LOW[(size_t)p * blk + e] * v.col[cl];
      } else {
        upp = v.LOW[(size_t)p * blk + e];  // overwritten with up[p] by p's parent row
      }
      upp *= v.SF[(size_t)p * KSEQ_PT + cl];
      ma[q] = v.MSG[(size_t)ca * blk + e];
      mb[q] = fold ? v.LOW[(size_t)cb * blk + e] : v.MSG[(size_t)cb * blk + e];
      ut[0][q] = upp * mb[q];
      ut[1][q] = upp * ma[q];
      if (fold) v.LOW[(size_t)cb * blk + e] = ut[1][q];  // the merged child has no branch: this is its upward vector
      if constexpr (SUM)
        if (fold) v.CC[(size_t)cb * blk + e] = ut[1][q] * mb[q];  // and its share: the root's point of the tree
    }
    if (!SUM && p == root) {
      __syncthreads();
      if (tid < KT) {
        double acc = 0.0;
        for (int col = 0; col < KSEQ_PT; ++col) acc += v.X0[tid * KSEQ_XS + col];
        slot[kseq_slot_rootpi(KT) + tid] = acc;
      }
    }
    for (int which = 0; which < 2; ++which) {
      if (which && fold) break;
      const int ch = which ? cb : ca;
      const double t = bl[ch] * rc;
      __syncthreads();  // X0 .. X3, ev, em and red are free
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * wave + g + 4 * q;
        v.X0[i * KSEQ_XS + cl] = ut[which][q] * v.isq[i];
      }
      for (int i = tid; i < KT; i += nt) v.ev[i] = exp(v.lam[i] * t), v.em[i] = expm1(v.lam[i] * t);
      __syncthreads();
      const kseq_v4d aa = kseq_mm_vt(v.V, v.VS, v.X0, KT, wave, lane);
      double gp = 0.0;
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * wave + g + 4 * q;
        const double cc = v.CC[(size_t)ch * blk + i * KSEQ_PT + cl];
        if constexpr (!SUM) gp = fma(aa[q] * (v.lam[i] * v.ev[i]), cc, gp);
        v.X1[i * KSEQ_XS + cl] = v.em[i] * aa[q];
        v.X2[i * KSEQ_XS + cl] = aa[q];
        if constexpr (SUM)
          v.X3[i * KSEQ_XS + cl] = cc * v.col[KSEQ_PT + cl];  // w_i here: a zero-weight column counts nothing
        else
          v.X3[i * KSEQ_XS + cl] = cc;
      }
      if constexpr (!SUM) {
        for (int o = 32; o > 0; o >>= 1) gp += __shfl_xor(gp, o);
        if (lane == 0) v.red[wave] = gp;
      }
      __syncthreads();
      if constexpr (!SUM) {
        if (tid == 0) {
          double G = v.red[0];
          for (int w = 1; w < NB; ++w) G += v.red[w];
          slot[kseq_slot_gb(KT) + ch] = G;
          grs = fma(bl[ch], G, grs);
        }
      }
      const kseq_v4d up = kseq_mm_v(v.V, v.VS, v.X1, KT, wave, lane);
      for (int q = 0; q < 4; ++q) {
        const int i = 16 * wave + g + 4 * q;
        const double du = v.sq[i] * up[q], lo = v.low(ch, i, cl);  // up - u~, as the message is low + (msg - low)
        if constexpr (!SUM) dv[q] += du * lo - ut[which][q] * ((which ? mb[q] : ma[q]) - lo);
        if (ch >= S) v.LOW[(size_t)ch * blk + i * KSEQ_PT + cl] = ut[which][q] + du;
        if constexpr (SUM)  // this lane read the entry's c above: the block is free for the node's share
          if (ch >= S) v.CC[(size_t)ch * blk + i * KSEQ_PT + cl] = (ut[which][q] + du) * lo;
      }
      double cnt[KSEQ_SUM_LMAX] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int lb = 0; lb < 4; ++lb) {
        if (lb >= NB) break;
        const kseq_v4d M = kseq_mm_outer(v.X2, v.X3, wave, lb, lane);
        const int l = 16 * lb + cl;
        const double ll = v.lam[l], El = v.ev[l], Ml = v.em[l];
        for (int q = 0; q < 4; ++q) {
          const int k = 16 * wave + g + 4 * q;
          const double ri = v.RT[k * v.VS + l];
          const double phi = ri == 0.0 ? phi_close(v.lam[k], ll, t, v.ev[k], El) : (v.em[k] - Ml) * ri;
          if constexpr (SUM) {
            const double mp = M[q] * phi;  // exactly 0 at t = 0, every arm of Phi
#pragma unroll
            for (int lab = 0; lab < KSEQ_SUM_LMAX; ++lab)
              if (lab < NL) cnt[lab] = fma(mp, blab[(size_t)lab * KT * KT + (size_t)k * KT + l], cnt[lab]);
          } else {
            W[lb][q] = fma(M[q], phi, W[lb][q]);
          }
        }
      }
      if constexpr (SUM) {  // as G: the wave's butterfly, then the waves in order
#pragma unroll
        for (int lab = 0; lab < KSEQ_SUM_LMAX; ++lab) {
          if (lab >= NL) break;
          double c = cnt[lab];
          for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
          if (lane == 0) v.red[wave * KSEQ_SUM_LMAX + lab] = c;
        }
        __syncthreads();
        if (tid < NL) {
          double acc = v.red[tid];
          for (int w = 1; w < NB; ++w) acc += v.red[w * KSEQ_SUM_LMAX + tid];
          slot[kseq_sum_slot_at(tid, ch, a.B)] = acc;
        }
      }
    }
  }
  if constexpr (SUM) return;
  __syncthreads();
  for (int q = 0; q < 4; ++q) {
    const int k = 16 * wave + g + 4 * q;
    v.X0[k * KSEQ_XS + cl] = dv[q];
#pragma unroll
    for (int lb = 0; lb < 4; ++lb)
      if (lb < NB) slot[kseq_slot_w(KT) + (size_t)k * KT + 16 * lb + cl] = W[lb][q];
  }
  __syncthreads();
  if (tid < KT) {
    double acc = 0.0;
    for (int col = 0; col < KSEQ_PT; ++col) acc += v.X0[tid * KSEQ_XS + col];
    slot[kseq_slot_dvec(KT) + tid] = acc;
  }
  if (tid == 0) slot[kseq_slot_grs(KT, a.B)] = grs;
}

__global__ void __launch_bounds__(256) kseq_down_kernel(KseqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  const size_t wslen = kseq_ws_doubles(a.N, a.KT), slotlen = kseq_slot_doubles(a.KT, a.B);
  const int per_draw = a.G * a.ntiles, items = a.ndraw * per_draw;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int dl = item / per_draw, rem = item - dl * per_draw, gc = rem / a.ntiles, tile = rem - gc * a.ntiles;
    const size_t at = kseq_item(dl, gc, tile, a.G, a.ntiles);
    kseq_down_item<false>(a, dl, gc, tile, shm, a.ws + at * wslen, a.slots + at * slotlen, nullptr, 0);
  }
}

// ---- phase 5: component m's share of one draw's row; component 0's workgroup also writes what the components
// share (log L, d/dblens, d/drs, d/dps).  false: a bad draw.
__device__ bool kseq_combine(const KseqArgs& a, int dl, int m, double* shm) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, KT = a.KT, M = a.M, C = a.C, G = a.G, B = a.B, ntiles = a.ntiles, draw = a.draw0 + dl;
  const GeoView v(shm, K);
  const int KP = v.KP;
  const double* par = a.params + (size_t)draw * kseq_mix_param_len(K, M, C);
  const double* rates = par + kseq_mix_par_comp(K, m);
  const double* freqs = rates + kseq_par_freqs(K);
  const double* rs = par + kseq_mix_par_rs(K, M);
  const double* rec = a.rec + kseq_rec_at(draw, m, M, K);
  const double* rec0 = a.rec + kseq_rec_at(draw, 0, M, K);
  double* orow = a.out + (size_t)draw * kseq_mix_row_len(B, K, M, C);
  if (!kseq_draw_ok(a, draw) || rec0[KREC_BAD] != 0.0) return false;
  const double s = rec[KREC_S];
  const size_t slotlen = kseq_slot_doubles(KT, B);
  const double* slots0 = a.slots + kseq_item(dl, 0, 0, G, ntiles) * slotlen;  // the draw's
  const double* slots = slots0 + (size_t)m * C * ntiles * slotlen;            // the component's
  const int nslot = C * ntiles;  // ascending (category, tile)
  for (int i = tid; i < K; i += nt) {
    v.pi[i] = freqs[i];
    v.sq[i] = rec[kseq_rec_sq(K) + i];
    v.isq[i] = rec[kseq_rec_isq(K) + i];
    v.qd[i] = rec[kseq_rec_qd(K) + i];
  }
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    v.V[i * KP + j] = rec[kseq_rec_v(K) + it];
    double acc = 0.0;
    for (int sl = 0; sl < nslot; ++sl) acc += slots[(size_t)sl * slotlen + kseq_slot_w(KT) + (size_t)i * KT + j];
    v.W[i * KP + j] = acc;
  }
  for (int i = tid; i < K; i += nt) {
    double d = 0.0, rp = 0.0;
    for (int sl = 0; sl < nslot; ++sl) {
      d += slots[(size_t)sl * slotlen + kseq_slot_dvec(KT) + i];
      rp += slots[(size_t)sl * slotlen + kseq_slot_rootpi(KT) + i];
    }
    v.dvec[i] = d;
    v.rrow[i] = rp;
  }
  if (m == 0) {  // over all G: component ascending, then category, then tile
    for (int b = tid; b < B; b += nt) {
      double acc = 0.0;
      for (int c = 0; c < G; ++c) {
        double in = 0.0;
        for (int tl = 0; tl < ntiles; ++tl) in += slots0[(size_t)(c * ntiles + tl) * slotlen + kseq_slot_gb(KT) + b];
        acc = fma(rs[c], in, acc);
      }
      orow[kseq_row_blens() + b] = acc;
    }
    for (int c = tid; c < G; c += nt) {
      double x = 0.0, y = 0.0;
      for (int tl = 0; tl < ntiles; ++tl) {
        x += slots0[(size_t)(c * ntiles + tl) * slotlen + kseq_slot_grs(KT, B)];
        y += slots0[(size_t)(c * ntiles + tl) * slotlen + kseq_slot_gps(KT, B)];
      }
      orow[kseq_row_rs(B) + c] = x;
      orow[kseq_row_ps(B, G) + c] = y;
    }
  }
  __syncthreads();
  geo_sym_vwvt(v, [](int, int, double) {});
  __syncthreads();
  double* g_freqs = orow + kseq_mix_row_freqs(B, K, M, C, m);
  geo_chain_rule(v, rates, s, orow + kseq_mix_row_rates(B, K, M, C, m), g_freqs);
  __syncthreads();
  for (int j = tid; j < K; j += nt) g_freqs[j] += v.rrow[j];  // the root term
  if (tid == 0 && m == 0) orow[0] = rec0[KREC_LL];
  return true;
}

__global__ void __launch_bounds__(GEO_MAX_THREADS) kseq_combine_kernel(KseqArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* shm = reinterpret_cast<double*>(geo_smem);
  const int rowlen = kseq_mix_row_len(a.B, a.K, a.M, a.C);
  for (int dm = blockIdx.x; dm < a.ndraw * a.M; dm += gridDim.x) {
    const int dl = dm / a.M, m = dm - dl * a.M;
    __syncthreads();  // the previous component's readers of LDS are done
    const bool ok = kseq_combine(a, dl, m, shm);
    __syncthreads();
    if (!ok && m == 0) {  // a bad draw: no component's workgroup wrote to its row
      const int draw = a.draw0 + dl;
      double* orow = a.out + (size_t)draw * rowlen;
      for (int i = threadIdx.x; i < rowlen; i += blockDim.x) orow[i] = i == 0 ? -INFINITY : 0.0;
      double* site = a.site + (size_t)draw * a.P;
      for (int i = threadIdx.x; i < a.P; i += blockDim.x) site[i] = -INFINITY;
      if (a.cpost) {
        double* cpost = a.cpost + kseq_cpost_at(draw, 0, a.M, a.P);
        for (int i = threadIdx.x; i < a.M * a.P; i += blockDim.x) cpost[i] = 0.0;
      }
    }
  }
}

// One context type behind both boundaries (phy_kseq_mix_ctx is its other name): phy_kseq_create makes it at M = 1.
struct phy_kseq_ctx {
  KseqPlan plan;
  int device = 0;
  hipStream_t stream = nullptr;
  uint64_t* d_masks = nullptr;
  int* d_rows = nullptr;
  double *d_tile_w = nullptr, *d_blens = nullptr, *d_params = nullptr, *d_rec = nullptr, *d_ws = nullptr;
  double *d_slots = nullptr, *d_lc = nullptr, *d_sh = nullptr, *d_down0 = nullptr, *d_out = nullptr, *d_site = nullptr;
  double* d_cpost = nullptr;
  std::vector<double> sweeps;  // the last call's, per (draw, component)
  int last_n = 0;
};

namespace {
void free_kseq(phy_kseq_ctx* c) {
  if (!c) return;
  DeviceGuard on(c->device);
  for (void* p : {(void*)c->d_masks, (void*)c->d_rows, (void*)c->d_tile_w, (void*)c->d_blens, (void*)c->d_params,
                  (void*)c->d_rec, (void*)c->d_ws, (void*)c->d_slots, (void*)c->d_lc, (void*)c->d_sh,
                  (void*)c->d_down0, (void*)c->d_out, (void*)c->d_site, (void*)c->d_cpost})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

void kseq_facts(const KseqPlan& pl, long long* f) {
  const long long fv[16] = {pl.KT,
                            pl.ntiles,
                            pl.items_per_draw,
                            pl.chunk_draws,
                            pl.threads,
                            pl.workgroups,
                            pl.draw_workgroups,
                            (long long)pl.lds_up,
                            (long long)pl.lds_down,
                            (long long)pl.lds_draw,
                            (long long)pl.ws_doubles,
                            (long long)pl.slot_doubles,
                            (long long)pl.rec_doubles,
                            pl.row_len,
                            pl.B,
                            (long long)(pl.n_ws * sizeof(double))};
  std::copy(fv, fv + 16, f);
}

// who: "phy_kseq_create: " or "phy_kseq_mix_create: "
// n_labels > 0: the summaries' context (kseq_sum.inc), whose label refusals join the plan's
int kseq_create(const std::string& who, int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks,
                const double* weights, const int32_t* peel, int max_draws, int device, phy_kseq_ctx** out,
                int n_labels = 0, const double* labels = nullptr) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, who + "out is NULL");
  *out = nullptr;
  {
    KseqPlan probe;  // every refusal before the first device call
    int rc = kseq_mix_plan(S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, 1, probe, who);
    if (rc) return rc;
    KseqSumPlan sprobe;
    if (labels || n_labels) rc = kseq_sum_plan(probe, n_labels, labels, 1, sprobe, who);
    if (rc) return rc;
  }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  std::unique_ptr<phy_kseq_ctx, void (*)(phy_kseq_ctx*)> c(new phy_kseq_ctx(), free_kseq);
  HIP_TRY(hipSetDevice(device));
  c->device = device;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  int rc = kseq_mix_plan(S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, cus, c->plan, who);
  if (rc) return rc;
  const KseqPlan& pl = c->plan;
  for (const void* f : {(const void*)kseq_eig_kernel, (const void*)kseq_up_kernel, (const void*)kseq_site_kernel,
                        (const void*)kseq_down_kernel, (const void*)kseq_combine_kernel})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KSEQ_LDS_CAP));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  if ((rc = dalloc(&c->d_masks, pl.tile_masks.size())) || (rc = dalloc(&c->d_tile_w, pl.tile_w.size())) ||
      (rc = dalloc(&c->d_rows, pl.rows.size())) || (rc = dalloc(&c->d_blens, pl.n_blens)) ||
      (rc = dalloc(&c->d_params, pl.n_params)) || (rc = dalloc(&c->d_rec, pl.n_rec)) ||
      (rc = dalloc(&c->d_ws, pl.n_ws)) || (rc = dalloc(&c->d_slots, pl.n_slots)) ||
      (rc = dalloc(&c->d_lc, pl.n_lc)) || (rc = dalloc(&c->d_sh, pl.n_sh)) ||
      (rc = dalloc(&c->d_down0, pl.n_down0)) || (rc = dalloc(&c->d_out, pl.n_rows_out)) ||
      (rc = dalloc(&c->d_site, pl.n_site)) || (rc = dalloc(&c->d_cpost, pl.n_cpost)))
    return rc;
  if ((rc = upload(c->d_masks, pl.tile_masks)) || (rc = upload(c->d_tile_w, pl.tile_w)) ||
      (rc = upload(c->d_rows, pl.rows)))
    return rc;
  c->sweeps.assign((size_t)max_draws * M, -1.0);
  *out = c.release();
  return PHY_OK;
}

// who: "phy_kseq_eval" or "phy_kseq_mix_eval"
int kseq_eval(const std::string& who, phy_kseq_ctx* ctx, int n_draws, const double* blens, const double* params,
              double* rows, double* site_ll, double* class_post) {
  if (!ctx) return fail(PHY_EINVAL, who + ": NULL ctx");
  if (!blens || !params || !rows) return fail(PHY_EINVAL, who + ": NULL host buffer");
  if (n_draws < 1 || n_draws > ctx->plan.max_draws)
    return fail(PHY_ERANGE, who + ": n_draws out of range (1..max_draws)");
  const KseqPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_blens, blens, sizeof(double) * n * pl.B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * pl.param_len, hipMemcpyHostToDevice, st));
  KseqArgs a{};
  a.masks = ctx->d_masks, a.tile_w = ctx->d_tile_w, a.rows = ctx->d_rows, a.blens = ctx->d_blens;
  a.params = ctx->d_params, a.rec = ctx->d_rec, a.ws = ctx->d_ws, a.slots = ctx->d_slots, a.lc = ctx->d_lc;
  a.sh = ctx->d_sh, a.down0 = ctx->d_down0, a.out = ctx->d_out, a.site = ctx->d_site;
  a.cpost = class_post ? ctx->d_cpost : nullptr;
  a.S = pl.S, a.P = pl.P, a.K = pl.K, a.M = pl.M, a.C = pl.C, a.G = pl.G, a.B = pl.B, a.N = pl.N, a.KT = pl.KT;
  a.NB = pl.NB, a.ntiles = pl.ntiles, a.PP = pl.PP, a.n = n_draws;
  hipLaunchKernelGGL(kseq_eig_kernel, dim3(std::min(n_draws * pl.M, pl.comp_workgroups)), dim3(pl.draw_threads),
                     pl.lds_draw, st, a);
  HIP_TRY(hipGetLastError());
  for (int d0 = 0; d0 < n_draws; d0 += pl.chunk_draws) {  // a draw's rows do not depend on the chunk it falls in
    a.draw0 = d0, a.ndraw = std::min(pl.chunk_draws, n_draws - d0);
    const long long items = (long long)a.ndraw * pl.items_per_draw;
    const dim3 igrid((int)std::min<long long>(items, pl.workgroups)), dgrid(std::min(a.ndraw, pl.draw_workgroups));
    const dim3 cgrid(std::min(a.ndraw * pl.M, pl.comp_workgroups));
    hipLaunchKernelGGL(kseq_up_kernel, igrid, dim3(pl.threads), pl.lds_up, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_site_kernel, dgrid, dim3(pl.site_threads), pl.lds_draw, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_down_kernel, igrid, dim3(pl.threads), pl.lds_down, st, a);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(kseq_combine_kernel, cgrid, dim3(pl.draw_threads), pl.lds_draw, st, a);
    HIP_TRY(hipGetLastError());
  }
  HIP_TRY(hipMemcpyAsync(rows, ctx->d_out, sizeof(double) * n * pl.row_len, hipMemcpyDeviceToHost, st));
  if (site_ll) HIP_TRY(hipMemcpyAsync(site_ll, ctx->d_site, sizeof(double) * n * pl.P, hipMemcpyDeviceToHost, st));
  if (class_post)
    HIP_TRY(hipMemcpyAsync(class_post, ctx->d_cpost, sizeof(double) * n * pl.M * pl.P, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpy2DAsync(ctx->sweeps.data(), sizeof(double), ctx->d_rec + KREC_SWEEPS,
                           sizeof(double) * pl.rec_doubles, sizeof(double), n * pl.M, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->last_n = n_draws;
  return PHY_OK;
}

int kseq_info(const std::string& who, const phy_kseq_ctx* ctx, int n, int32_t* sweeps, long long* facts) {
  if (!ctx) return fail(PHY_EINVAL, who + ": NULL ctx");
  if (sweeps) {
    if (n < 0 || n > ctx->last_n) return fail(PHY_ERANGE, who + ": the last call had fewer draws");
    for (int i = 0; i < n * ctx->plan.M; ++i) sweeps[i] = (int32_t)ctx->sweeps[(size_t)i];
  }
  if (facts) kseq_facts(ctx->plan, facts);
  return PHY_OK;
}
}  // namespace

extern "C" {

int phy_kseq_create(int S, int P, int K, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                    const int32_t* peel, int max_draws, int device, phy_kseq_ctx** out) {
  return kseq_create("phy_kseq_create: ", S, P, K, 1, C, rooted, tipmasks, weights, peel, max_draws, device, out);
}

int phy_kseq_destroy(phy_kseq_ctx* ctx) {
  free_kseq(ctx);
  return PHY_OK;
}

int phy_kseq_num_branches(const phy_kseq_ctx* ctx) { return ctx ? ctx->plan.B : -1; }

int phy_kseq_row_len(const phy_kseq_ctx* ctx) { return ctx ? ctx->plan.row_len : -1; }

int phy_kseq_eval(phy_kseq_ctx* ctx, int n_draws, const double* blens, const double* params, double* rows,
                  double* site_ll) {
  if (ctx && ctx->plan.M != 1) return fail(PHY_EINVAL, "phy_kseq_eval: the context is a mixture's (phy_kseq_mix_eval)");
  return kseq_eval("phy_kseq_eval", ctx, n_draws, blens, params, rows, site_ll, nullptr);
}

int phy_kseq_plan(int S, int P, int K, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                  const int32_t* peel, int max_draws, int cu_count, long long* facts) {
  g_err.clear();
  KseqPlan pl;
  const int rc = kseq_plan(S, P, K, C, rooted, tipmasks, weights, peel, max_draws, cu_count, pl);
  if (rc) return rc;
  if (facts) kseq_facts(pl, facts);
  return PHY_OK;
}

int phy_kseq_info(const phy_kseq_ctx* ctx, int n, int32_t* sweeps, long long* facts) {
  return kseq_info("phy_kseq_info", ctx, n, sweeps, facts);
}

int phy_kseq_mix_create(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks,
                        const double* weights, const int32_t* peel, int max_draws, int device,
                        phy_kseq_ctx** out) {
  return kseq_create("phy_kseq_mix_create: ", S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, device, out);
}

int phy_kseq_mix_destroy(phy_kseq_ctx* ctx) {
  free_kseq(ctx);
  return PHY_OK;
}

int phy_kseq_mix_num_branches(const phy_kseq_ctx* ctx) { return ctx ? ctx->plan.B : -1; }

int phy_kseq_mix_row_len(const phy_kseq_ctx* ctx) { return ctx ? ctx->plan.row_len : -1; }

int phy_kseq_mix_eval(phy_kseq_ctx* ctx, int n_draws, const double* blens, const double* params, double* rows,
                      double* site_ll, double* class_post) {
  return kseq_eval("phy_kseq_mix_eval", ctx, n_draws, blens, params, rows, site_ll, class_post);
}

int phy_kseq_mix_plan(int S, int P, int K, int M, int C, int rooted, const uint64_t* tipmasks, const double* weights,
                      const int32_t* peel, int max_draws, int cu_count, long long* facts) {
  g_err.clear();
  KseqPlan pl;
  const int rc = kseq_mix_plan(S, P, K, M, C, rooted, tipmasks, weights, peel, max_draws, cu_count, pl);
  if (rc) return rc;
  if (facts) kseq_facts(pl, facts);
  return PHY_OK;
}

int phy_kseq_mix_info(const phy_kseq_ctx* ctx, int n, int32_t* sweeps, long long* facts) {
  return kseq_info("phy_kseq_mix_info", ctx, n, sweeps, facts);
}

}  // extern "C"
