// geo_phases.inc -- the device phases both K-state engines run, each stated
// once: geo_engine.inc (one tree: geo_draw runs them all) and geo_trees.inc (a
// tree sample: its eigen, tree and combine kernels run them in three parts).
// Included by phylo_hip.hip before geo_engine.inc.
//
// A phase is a __device__ __forceinline__ function over a GeoView, the LDS and
// workspace pointers of one workgroup.  What differs between the callers (the
// refusal terms, where results are stored, the rn / ro fold of the tree kernel,
// the summary rows) stays in the callers; CLOCK is the one compile-time switch:
// it multiplies a branch length by mu wherever one is read.  Every phase is
// called by the whole workgroup, and the line above each states its barriers:
// what must be synchronised on entry, what is on exit.
//
// Two small phases are not here but written out in both callers: the 1 / (lam_k
// - lam_l) table and the root sum with log L.  As shared functions they gave the
// same bits and slower kernels: phy_geo_eval +0.3 to +2.4 percent over the
// parent commit at all 9 shapes timed (+0.3 to +0.8 at K = 64), phy_geo_trees_eval
// up to +1.0 at K = 20, where written out they are at or below it
// (profiles/geo_shared_phases_variants.json, DESIGN.md 5f).

constexpr int GEO_SWEEP_CAP = 60;
constexpr double GEO_JTOL = 1e-32;    // off(A)^2 <= GEO_JTOL |A|^2
constexpr int GEO_SCALE_BELOW = -64;  // a node whose largest partial is below 2^-64 is rescaled to [1, 2)
constexpr int GEO_SHIFT_MAX = 1000;

// sum over the workgroup in a fixed order (nt a power of two)
__device__ __forceinline__ double geo_block_sum(double v, double* red, int tid, int nt) {
  __syncthreads();
  red[tid] = v;
  __syncthreads();
  for (int s = nt >> 1; s > 0; s >>= 1) {
    if (tid < s) red[tid] += red[tid + s];
    __syncthreads();
  }
  return red[0];
}

// rates_geo entry of the pair (i, j), i != j: the emitter fills the strict lower triangle column by column
__device__ __forceinline__ int geo_rate_index(int K, int i, int j) {
  const int row = i > j ? i : j, col = i > j ? j : i;
  return col * (K - 1) - col * (col - 1) / 2 + (row - col - 1);
}

// One workgroup's pointers: the LDS layout of GeoLds and, for the phases that walk a tree, the per-node K-vectors
// of its workspace block (GW_*) and the tips.
struct GeoView {
  int K, KP, S, N, B, root;
  double *A, *V, *W;                                      // GeoLds: what each holds, phase by phase
  double *lam, *sq, *isq, *pi, *qd, *dvec, *rrow, *dd;    // dvec: colt - rowt; rrow: the root row (tree sample)
  double *rcs, *rsn, *red;
  int *rp, *rq;
  const double* tips;
  double *LOW, *CC, *MSG, *UT, *AA, *EE, *UP, *EM;  // EE: exp(lam t) of each branch; EM: expm1(lam t)
  double *sfac, *sexp;  // [N] 2^shift of each internal node; [N] the shift
  __device__ __forceinline__ GeoView(double* sh, int K_) : K(K_), S(0), N(0), B(0), root(0), tips(nullptr) {
    const GeoLds L(K);
    KP = L.KP;
    A = sh + L.A(), V = sh + L.V(), W = sh + L.W();
    lam = sh + L.vecs(0), sq = sh + L.vecs(1), isq = sh + L.vecs(2), pi = sh + L.vecs(3), qd = sh + L.vecs(4);
    dvec = sh + L.vecs(5), rrow = sh + L.vecs(6), dd = sh + L.vecs(7);
    rcs = sh + L.cs(), rsn = sh + L.sn(), red = sh + L.red();
    rp = reinterpret_cast<int*>(sh + L.pq());
    rq = rp + GEO_KMAX / 2;
    LOW = CC = MSG = UT = AA = EE = UP = EM = sfac = sexp = nullptr;
  }
  __device__ __forceinline__ GeoView(double* sh, int K_, double* wsb, const double* tips_, int S_) : GeoView(sh, K_) {
    S = S_, N = 2 * S - 1, B = 2 * S - 3, root = 2 * S - 2, tips = tips_;
    const size_t NK = (size_t)N * K;
    LOW = wsb + GW_LOW * NK, CC = wsb + GW_C * NK, MSG = wsb + GW_MSG * NK, UT = wsb + GW_UT * NK;
    AA = wsb + GW_AA * NK, EE = wsb + GW_E * NK, UP = wsb + GW_UP * NK, EM = wsb + GW_EM * NK;
    sfac = wsb + GEO_WS_ARRAYS * NK;
    sexp = sfac + N;
  }
  __device__ __forceinline__ const double* low(int node) const {
    return node < S ? tips + (size_t)node * K : LOW + (size_t)node * K;
  }
};

// The parameters: refuse what has no likelihood.  bad: this thread's share of the caller's further refusal terms.
// Barriers: none needed on entry (red is free); ends on geo_block_sum's.  The result is workgroup-uniform.
__device__ __forceinline__ bool geo_params_ok(const GeoView& v, const double* rates, const double* freqs, double bad) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, R = K * (K - 1) / 2;
  for (int i = tid; i < K; i += nt) bad += (freqs[i] > 0.0 && isfinite(freqs[i])) ? 0.0 : 1.0;
  for (int i = tid; i < R; i += nt) bad += (rates[i] >= 0.0 && isfinite(rates[i])) ? 0.0 : 1.0;
  return geo_block_sum(bad, v.red, tid, nt) == 0.0;
}

// qd, the diagonal of the unnormalised Q (generate_script.py:922-926), and s = -sum_i qd_i pi_i, returned.  No
// likelihood unless s > 0 and finite: the caller's refusal.
// Barriers: the caller has written pi (no barrier yet); ends on geo_block_sum's, qd synchronised.  s is uniform.
__device__ __forceinline__ double geo_q_scale(const GeoView& v, const double* rates) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K;
  __syncthreads();
  for (int i = tid; i < K; i += nt) {
    double acc = 0.0;
    for (int j = 0; j < K; ++j)
      if (j != i) acc += rates[geo_rate_index(K, i, j)] * v.pi[j];
    v.qd[i] = -acc;
  }
  __syncthreads();
  return geo_block_sum(tid < K ? -v.qd[tid] * v.pi[tid] : 0.0, v.red, tid, nt);
}

// A's entry (i, j), i != j: geo_jacobi builds A from it, and the summaries take it again once A is spent.
__device__ __forceinline__ double geo_a_entry(const GeoView& v, const double* rates, double s, int i, int j) {
  return (v.sq[i] * v.sq[j]) * rates[geo_rate_index(v.K, i, j)] / s;
}

// The eigensystem of A = D^1/2 Q D^-1/2 by cyclic Jacobi.  true: converged within GEO_SWEEP_CAP sweeps, lam on the
// diagonal of A and the eigenvectors in V; sweeps is the count either way.
// Barriers: geo_q_scale's exit and sq synchronised on entry; A and V synchronised on exit.  The result is uniform.
__device__ __forceinline__ bool geo_jacobi(const GeoView& v, const double* rates, double s, int& sweeps) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  double *A = v.A, *V = v.V, *qd = v.qd, *rcs = v.rcs, *rsn = v.rsn, *red = v.red;
  int *rp = v.rp, *rq = v.rq;
  // ---- A = D^1/2 Q D^-1/2 (symmetric to the bit: sq_i sq_j is commutative), V = I
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    A[i * KP + j] = i == j ? qd[i] / s : geo_a_entry(v, rates, s, i, j);
    V[i * KP + j] = i == j ? 1.0 : 0.0;
  }
  // ---- cyclic Jacobi, round-robin ordering: n - 1 rounds of n / 2 disjoint pairs (n = K, or K + 1 with a bye)
  const int n = K + (K & 1), nr = n - 1, np = n / 2;
  bool converged = false;
  for (sweeps = 0; sweeps <= GEO_SWEEP_CAP; ++sweeps) {
    double off = 0.0, tot = 0.0;
    __syncthreads();
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      const double x = A[i * KP + j];
      tot += x * x;
      if (i != j) off += x * x;
    }
    off = geo_block_sum(off, red, tid, nt);
    tot = geo_block_sum(tot, red, tid, nt);
    if (off <= GEO_JTOL * tot || off == 0.0) {
      converged = true;
      break;
    }
    if (sweeps == GEO_SWEEP_CAP || !isfinite(off)) break;
    for (int r = 0; r < nr; ++r) {
      if (tid < np) {
        int x = tid == 0 ? r : (r + tid) % nr, y = tid == 0 ? n - 1 : (r - tid + nr) % nr;
        int p = x < y ? x : y, q = x < y ? y : x;
        double c = 1.0, sn = 0.0;
        if (q >= K) {
          p = -1;  // the bye
        } else {
          jacobi_rot(A[p * KP + p], A[q * KP + q], A[p * KP + q], c, sn);
        }
        rp[tid] = p, rq[tid] = q, rcs[tid] = c, rsn[tid] = sn;
      }
      __syncthreads();
      for (int it = tid; it < np * K; it += nt) {  // A <- A J, V <- V J (columns p, q of every row k)
        const int m = it / K, k = it - m * K, p = rp[m], q = rq[m];
        if (p < 0) continue;
        const double c = rcs[m], sn = rsn[m];
        const double a1 = A[k * KP + p], b1 = A[k * KP + q];
        A[k * KP + p] = c * a1 - sn * b1;
        A[k * KP + q] = sn * a1 + c * b1;
        const double v1 = V[k * KP + p], w1 = V[k * KP + q];
        V[k * KP + p] = c * v1 - sn * w1;
        V[k * KP + q] = sn * v1 + c * w1;
      }
      __syncthreads();
      for (int it = tid; it < np * K; it += nt) {  // A <- J^T A (rows p, q of every column k)
        const int m = it / K, k = it - m * K, p = rp[m], q = rq[m];
        if (p < 0) continue;
        const double c = rcs[m], sn = rsn[m];
        const double a1 = A[p * KP + k], b1 = A[q * KP + k];
        A[p * KP + k] = k == q ? 0.0 : c * a1 - sn * b1;
        A[q * KP + k] = k == p ? 0.0 : sn * a1 + c * b1;
      }
      __syncthreads();
    }
  }
  return converged;
}

// Pruning in the eigenbasis, level by level, on one tree's schedule (rows, lvl[nlev + 1]) and branch lengths.
// A message is P(t) x = x + (P(t) - I) x, the second term through em = expm1(lam t): V V^T is the identity to
// 1e-16 only, which on a short branch is 1e-16 / (q t) of a transition probability q t, and at t = 0 it lets a
// parent take a state its tip forbids.  A zero-length branch passes x through exactly.
// Barriers: V, lam, sq, isq synchronised and the workspace's readers done on entry; LOW, sfac, sexp (and CC, EE,
// EM, MSG) synchronised on exit.
template <bool CLOCK>
__device__ __forceinline__ void geo_prune(const GeoView& v, const int* rows, const int* lvl, int nlev,
                                          const double* bl, double mu) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  const double *V = v.V, *lam = v.lam, *sq = v.sq, *isq = v.isq;
  double *LOW = v.LOW, *CC = v.CC, *MSG = v.MSG, *EE = v.EE, *EM = v.EM, *sfac = v.sfac, *sexp = v.sexp;
  const double small = ldexp(1.0, GEO_SCALE_BELOW);
  const int wave = tid >> 6, lane = tid & 63, nwaves = nt >> 6;
  for (int lv = 0; lv < nlev; ++lv) {
    const int r0 = lvl[lv], nrow = lvl[lv + 1] - r0;
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // c = V^T (sqrt(pi) v), e = exp(lam t), em = expm1(lam t)
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, k = rem - which * K;
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* x = v.low(ch);
      double acc = 0.0;
      for (int j = 0; j < K; ++j) acc = fma(V[j * KP + k], sq[j] * x[j], acc);
      CC[(size_t)ch * K + k] = acc;
      double lt;
      if constexpr (CLOCK)
        lt = lam[k] * (mu * bl[ch]);
      else
        lt = lam[k] * bl[ch];
      EE[(size_t)ch * K + k] = exp(lt);
      EM[(size_t)ch * K + k] = expm1(lt);
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // message = v + (V (em c)) / sqrt(pi)
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* em = EM + (size_t)ch * K;
      const double* c = CC + (size_t)ch * K;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(V[i * KP + k], em[k] * c[k], acc);
      MSG[(size_t)ch * K + i] = v.low(ch)[i] + isq[i] * acc;
    }
    __syncthreads();
    for (int idx = wave; idx < nrow; idx += nwaves) {  // one wave per node: the product and its rescaling
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      const int ca = row[GR_A], cb = row[GR_B], p = row[GR_P];
      double x = 0.0;
      if (lane < K) x = MSG[(size_t)ca * K + lane] * (row[GR_LAST] ? v.low(cb)[lane] : MSG[(size_t)cb * K + lane]);
      double mx = x;
      for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
      int shift = 0;
      double fac = 1.0;
      if (mx > 0.0 && mx < small) {
        shift = -ilogb(mx);
        if (shift > GEO_SHIFT_MAX) shift = GEO_SHIFT_MAX;
        fac = ldexp(1.0, shift);
      }
      if (lane < K) LOW[(size_t)p * K + lane] = x * fac;
      if (lane == 0) sfac[p] = fac, sexp[p] = (double)shift;
    }
    __syncthreads();
  }
}

// The reverse pass, top level first: per branch u~ (UT), a = V^T (u~ / sqrt(pi)) (AA), the downward message (UP),
// P^T u~ = u~ + (P^T - I) u~ through em as the way up.
// Barriers: geo_prune's exit and Ls uniform on entry; UT, AA, UP synchronised on exit.
__device__ __forceinline__ void geo_reverse(const GeoView& v, const int* rows, const int* lvl, int nlev, double Ls) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  const double *V = v.V, *sq = v.sq, *isq = v.isq, *MSG = v.MSG, *EM = v.EM, *sfac = v.sfac;
  double *UT = v.UT, *AA = v.AA, *UP = v.UP;
  for (int i = tid; i < K; i += nt) UP[(size_t)v.root * K + i] = 1.0 / Ls;
  __syncthreads();
  for (int lv = nlev - 1; lv >= 0; --lv) {
    const int r0 = lvl[lv], nrow = lvl[lv + 1] - r0;
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // u~ = up[p] o (the sibling's message) 2^shift
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      const int ca = row[GR_A], cb = row[GR_B], p = row[GR_P], last = row[GR_LAST];
      const double upv = UP[(size_t)p * K + i] * sfac[p];
      if (!which)
        UT[(size_t)ca * K + i] = upv * (last ? v.low(cb)[i] : MSG[(size_t)cb * K + i]);
      else if (last)
        UP[(size_t)cb * K + i] = upv * MSG[(size_t)ca * K + i];  // the merged child: no branch of its own
      else
        UT[(size_t)cb * K + i] = upv * MSG[(size_t)ca * K + i];
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // a = V^T (u~ / sqrt(pi))
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, k = rem - which * K;
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* u = UT + (size_t)ch * K;
      double acc = 0.0;
      for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k], u[i] * isq[i], acc);
      AA[(size_t)ch * K + k] = acc;
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // up[child] = u~ + sqrt(pi) (V (em a)) = P^T u~
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, j = rem - which * K;
      const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* em = EM + (size_t)ch * K;
      const double* aa = AA + (size_t)ch * K;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(V[j * KP + k], em[k] * aa[k], acc);
      UP[(size_t)ch * K + j] = UT[(size_t)ch * K + j] + sq[j] * acc;
    }
    __syncthreads();
  }
}

// W_kl = sum_b (a_bk c_bl) Phi_kl(lam, t_b), the three-arm rule: the 1 / (lam_k - lam_l) table where it is not 0,
// phi_close inside the near window.  The quotient is taken of em = expm1(lam t): on a short branch both
// exponentials are near 1 and their own difference keeps 1e-16 / (lam t) of it.  Returned; the caller stores or
// folds it.
// Barriers: geo_reverse's exit and the 1 / (lam_k - lam_l) table in A synchronised on entry; none on exit.
template <bool CLOCK>
__device__ __forceinline__ double geo_w_entry(const GeoView& v, int k, int l, const double* bl, double mu) {
  const int K = v.K;
  const double ri = v.A[k * v.KP + l], lk = v.lam[k], ll = v.lam[l];
  double acc = 0.0;
  for (int b = 0; b < v.B; ++b) {
    const double Ek = v.EE[(size_t)b * K + k], El = v.EE[(size_t)b * K + l];
    const double dm = v.EM[(size_t)b * K + k] - v.EM[(size_t)b * K + l];
    double phi;
    if constexpr (CLOCK)
      phi = ri == 0.0 ? phi_close(lk, ll, mu * bl[b], Ek, El) : dm * ri;
    else
      phi = ri == 0.0 ? phi_close(lk, ll, bl[b], Ek, El) : dm * ri;
    acc = fma(v.AA[(size_t)b * K + k] * v.CC[(size_t)b * K + l], phi, acc);
  }
  return acc;
}

// The direct D^{+-1/2} terms of P for state i, colt - rowt = sum_b (P^T u~) o v - sum_b u~ o (P v), formed branch
// by branch from the two differences, (P^T u~ - u~) o v - u~ o (P v - v): each sum alone is of the order of the
// number of branches, the two differences of the order of q t.
// Barriers: geo_reverse's exit on entry; none on exit.
__device__ __forceinline__ double geo_col_minus_row(const GeoView& v, int i) {
  const int K = v.K;
  double acc = 0.0;
  for (int b = 0; b < v.B; ++b) {
    const double ut = v.UT[(size_t)b * K + i], lo = v.low(b)[i];
    acc = fma(v.UP[(size_t)b * K + i] - ut, lo, acc);
    acc = fma(-ut, v.MSG[(size_t)b * K + i] - lo, acc);
  }
  return acc;
}

// ---- the dwell times of the summaries.  E[time in i] = G_ii, G = V W V^T, is of the order of the branch lengths
// while G's off-diagonal entries are of the order of 1 / q whatever the lengths are: on a short tree the product
// keeps 1e-16 of the latter on its diagonal.  Phi = t + Psi, and the t part of G_ii is sum_b t_b u~_bi v_bi exactly
// (V a = u~ / sqrt(pi), V c = sqrt(pi) v: geo_dwell_first); the rest, diag(V W2 V^T) with Psi in Phi's place
// (geo_dwell_f, geo_w2_entry, geo_w2_vt, geo_dwell_second), is of second order in t.  geo.py: psi_rule.
//
// expm1(x) - x = x^2 / 2 + x^3 / 6 + ...: the series to x^16 / 16! where |x| < 1/2 (the difference keeps 1e-16 / |x|
// of it), the difference beyond.  geo.py: expm1_less_x.
__device__ __forceinline__ double geo_expm1_less_x(double x, double em) {
  if (!(fabs(x) < 0.5)) return em - x;
  double h = 0.0;
  for (int n = 16; n > 2; --n) h = (x / (double)n) * (1.0 + h);
  return 0.5 * x * x * (1.0 + h);
}
// Psi_kl = Phi_kl - t inside the near window: phi_close's arms, each less t in closed form
__device__ __forceinline__ double geo_psi_close(double lk, double ll, double t, double Mk, double Ml, double Fk,
                                                double Fl) {
  const double d = lk - ll;
  if (fabs(d) < PHI_TIE * fmax(1.0, fabs(lk))) return t * Mk;
  const double x = d * t;
  if (fabs(x) < PHI_SERIES) {
    const double pm1 = x * fma(x, fma(x, fma(x, 1.0 / 120.0, 1.0 / 24.0), 1.0 / 6.0), 0.5);
    return t * fma(Ml, 1.0 + pm1, pm1);
  }
  return (Fk - Fl) / d;
}
// F[b][k] = expm1(lam_k t_b) - lam_k t_b over MSG, which is spent once colt - rowt is formed.
// Barriers: geo_col_minus_row's readers of MSG done on entry; the caller synchronises before F is read.
template <bool CLOCK>
__device__ __forceinline__ void geo_dwell_f(const GeoView& v, const double* bl, double mu) {
  const int K = v.K;
  for (int it = threadIdx.x; it < v.B * K; it += blockDim.x) {
    const int b = it / K, k = it - b * K;
    double lt;
    if constexpr (CLOCK)
      lt = v.lam[k] * (mu * bl[b]);
    else
      lt = v.lam[k] * bl[b];
    v.MSG[it] = geo_expm1_less_x(lt, v.EM[it]);
  }
}
// W2_kl = sum_b (a_bk c_bl) Psi_kl(lam, t_b).
// Barriers: geo_dwell_f's F and the 1 / (lam_k - lam_l) table in A synchronised on entry; none on exit.
template <bool CLOCK>
__device__ __forceinline__ double geo_w2_entry(const GeoView& v, int k, int l, const double* bl, double mu) {
  const int K = v.K;
  const double ri = v.A[k * v.KP + l], lk = v.lam[k], ll = v.lam[l];
  const double* F = v.MSG;
  double acc = 0.0;
  for (int b = 0; b < v.B; ++b) {
    const double Fk = F[(size_t)b * K + k], Fl = F[(size_t)b * K + l];
    double psi = (Fk - Fl) * ri;
    if (ri == 0.0) {
      const double Mk = v.EM[(size_t)b * K + k], Ml = v.EM[(size_t)b * K + l];
      if constexpr (CLOCK)
        psi = geo_psi_close(lk, ll, mu * bl[b], Mk, Ml, Fk, Fl);
      else
        psi = geo_psi_close(lk, ll, bl[b], Mk, Ml, Fk, Fl);
    }
    acc = fma(v.AA[(size_t)b * K + k] * v.CC[(size_t)b * K + l], psi, acc);
  }
  return acc;
}
// The first order of state i's dwell time: sum_b t_b u~_bi v_bi.  Barriers: geo_reverse's exit on entry.
template <bool CLOCK>
__device__ __forceinline__ double geo_dwell_first(const GeoView& v, int i, const double* bl, double mu) {
  const int K = v.K;
  double acc = 0.0;
  for (int b = 0; b < v.B; ++b) {
    double t = bl[b];
    if constexpr (CLOCK) t = mu * bl[b];
    acc = fma(t * v.UT[(size_t)b * K + i], v.low(b)[i], acc);
  }
  return acc;
}
// W2 V^T over A, W2 in W.  Barriers: W and V synchronised and A's readers done on entry; the caller synchronises
// before geo_dwell_second.
__device__ __forceinline__ void geo_w2_vt(const GeoView& v) {
  const int K = v.K, KP = v.KP;
  for (int it = threadIdx.x; it < K * K; it += blockDim.x) {
    const int k = it / K, i = it - k * K;
    double acc = 0.0;
    for (int l = 0; l < K; ++l) acc = fma(v.W[k * KP + l], v.V[i * KP + l], acc);
    v.A[k * KP + i] = acc;
  }
}
// (V W2 V^T)_ii from geo_w2_vt's A
__device__ __forceinline__ double geo_dwell_second(const GeoView& v, int i) {
  double acc = 0.0;
  for (int k = 0; k < v.K; ++k) acc = fma(v.V[i * v.KP + k], v.A[k * v.KP + i], acc);
  return acc;
}

// dlogL/dA = sym(V W V^T): T = W V^T over A (the spent table), then sym(V T) over the spent W.  each(i, j, G_ij)
// is called by the thread of entry (i, j) with G = V W V^T before it is symmetrised: the caller's summary write.
// Barriers: W and V synchronised and A's readers done on entry; none on exit, the caller synchronises before W is
// read.
template <class Each>
__device__ __forceinline__ void geo_sym_vwvt(const GeoView& v, Each each) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  double *A = v.A, *V = v.V, *W = v.W;
  for (int it = tid; it < K * K; it += nt) {
    const int k = it / K, j = it - k * K;
    double acc = 0.0;
    for (int l = 0; l < K; ++l) acc = fma(W[k * KP + l], V[j * KP + l], acc);
    A[k * KP + j] = acc;
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    double x = 0.0, y = 0.0;
    for (int k = 0; k < K; ++k) {
      x = fma(V[i * KP + k], A[k * KP + j], x);
      y = fma(V[j * KP + k], A[k * KP + i], y);
    }
    W[i * KP + j] = 0.5 * (x + y);
    each(i, j, x);
  }
}

// The chain rule to rates_geo and freqs_geo: A = D^1/2 Q D^-1/2, Q = Qu / s, s = -sum_i Qu_ii pi_i, Qu_ii =
// -sum_{j != i} R_ij pi_j, and the direct term 0.5 dvec / pi, dvec = colt - rowt (entries of freqs independent).
// Barriers: W = sym(V W V^T), dvec, pi, sq, isq, qd synchronised on entry; none after the rows' writes.
__device__ __forceinline__ void geo_chain_rule(const GeoView& v, const double* rates, double s, double* g_rates,
                                               double* g_freqs) {
  const int tid = threadIdx.x, nt = blockDim.x, K = v.K, KP = v.KP;
  const double *W = v.W, *sq = v.sq, *isq = v.isq, *pi = v.pi, *qd = v.qd, *dvec = v.dvec;
  double* dd = v.dd;
  double part = 0.0;
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    const double qu = i == j ? qd[i] : rates[geo_rate_index(K, i, j)] * pi[j];
    part = fma(W[i * KP + j] * sq[i] * isq[j], qu, part);
  }
  const double ds = -geo_block_sum(part, v.red, tid, nt) / (s * s);
  for (int i = tid; i < K; i += nt) dd[i] = W[i * KP + i] / s - ds * pi[i];
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {
    const int row = it / K, col = it - row * K;
    if (row <= col) continue;
    const double o1 = W[row * KP + col] * sq[row] * isq[col] / s - dd[row];
    const double o2 = W[col * KP + row] * sq[col] * isq[row] / s - dd[col];
    g_rates[geo_rate_index(K, row, col)] = o1 * pi[col] + o2 * pi[row];
  }
  for (int j = tid; j < K; j += nt) {
    double acc = 0.0;
    for (int i = 0; i < K; ++i)
      if (i != j) acc = fma(W[i * KP + j] * sq[i] * isq[j] / s - dd[i], rates[geo_rate_index(K, i, j)], acc);
    g_freqs[j] = 0.5 * dvec[j] / pi[j] - ds * qd[j] + acc;
  }
}
