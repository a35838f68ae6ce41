// geo_engine.inc -- the K-state discrete-trait ("phylogeography") likelihood
// engine: log L and its full gradient of one site of K locations on a fixed
// tree, K from 2 to 64, fp64 throughout.  Included by phylo_hip.hip.
//
// It replaces what the reference's --geo model leaves to Stan:
// calculate_p_matrices (generate_script.py:895-950: Q = R diag(pi) normalised,
// the symmetric eigendecomposition of A = D^1/2 Q D^-1/2, one K x K matrix
// product per branch) and the pruning loop (:1085-1096), both differentiated by
// reverse-mode autodiff on every log_prob.
//
// One workgroup evaluates one draw end to end in one launch (workgroups loop
// when there are more draws than workgroups):
//   1. A in LDS; cyclic Jacobi in the round-robin ordering of the 4 x 4 solver
//      (jacobi4): floor(K/2) disjoint rotations per round, odd K with a bye,
//      until off(A)^2 <= 1e-32 |A|^2; GEO_SWEEP_CAP sweeps without that is -inf.
//   2. pruning in the eigenbasis, P_b never formed: c = V^T (sqrt(pi) v),
//      message = (V (e^{lam t} c)) / sqrt(pi), level by level (geo_plan.h), with
//      power-of-two rescaling after every internal node;
//   3. the reverse pass: per branch u~ (dlogL / dmessage), a = V^T (u~ /
//      sqrt(pi)), the downward message sqrt(pi) (V (e^{lam t} a));
//   4. dlogL/dt_b = sum_k a_k lam_k e^{lam_k t} c_k, W = sum_b (a_b c_b^T) o
//      Phi(lam, t_b) with the three-arm rule (phi_rinv / phi_close), dlogL/dA =
//      sym(V W V^T), and the chain rule to rates_geo and freqs_geo (entries of
//      freqs independent, as grad_freqs of the 4-state rows).
//   5. (geo_draw<true>, phy_geo_eval_summaries) the posterior summaries those
//      leave behind: node marginals low o up, expected transitions A_ij G_ij and
//      dwell times G_ii from G = V W V^T, transitions per branch from M = V^T
//      A_off V.
// The per-node K-vectors live in a per-workgroup global workspace (GW_*): at
// K = 64 the three matrices leave no LDS for 7 (2S-1) K doubles, and each is
// written once and read a few times by the same CU (its L1 / L2 hold them).

constexpr int GEO_SWEEP_CAP = 60;
constexpr double GEO_JTOL = 1e-32;    // off(A)^2 <= GEO_JTOL |A|^2
constexpr int GEO_SCALE_BELOW = -64;  // a node whose largest partial is below 2^-64 is rescaled to [1, 2)
constexpr int GEO_SHIFT_MAX = 1000;

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

// The summaries form (phy_geo_eval_summaries) writes one more row per draw:
// marg[N][K], jumps[K][K], bjumps[B] (include/phylo_hip_geo.h).
struct GeoSumArgs : GeoArgs {
  double* summ;  // [n][N K + K K + B]
};
template <bool SUM>
using GeoArgsOf = std::conditional_t<SUM, GeoSumArgs, GeoArgs>;
inline int geo_summary_len(int S, int K) { return (2 * S - 1) * K + K * K + (2 * S - 3); }

// One draw.  false: the likelihood is not finite (the row is then -inf and zeros).
// SUM adds the posterior summaries from what the gradient leaves behind; every
// line of it is under if constexpr, so geo_draw<false> is the plain evaluation.
template <bool SUM>
__device__ bool geo_draw(const GeoArgsOf<SUM>& a, int draw, double* sh, double* wsb) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, S = a.S, N = 2 * S - 1, B = 2 * S - 3, R = K * (K - 1) / 2;
  const GeoLds L(K);
  const int KP = L.KP;
  double* A = sh + L.A();
  double* V = sh + L.V();
  double* W = sh + L.W();
  double* lam = sh + L.vecs(0);
  double* sq = sh + L.vecs(1);
  double* isq = sh + L.vecs(2);
  double* pi = sh + L.vecs(3);
  double* qd = sh + L.vecs(4);
  double* rowt = sh + L.vecs(5);
  double* colt = sh + L.vecs(6);
  double* dd = sh + L.vecs(7);
  double* rcs = sh + L.cs();
  double* rsn = sh + L.sn();
  double* red = sh + L.red();
  int* rp = reinterpret_cast<int*>(sh + L.pq());
  int* rq = rp + GEO_KMAX / 2;
  const double* rates = a.params + (size_t)draw * (R + K);
  const double* freqs = rates + R;
  const double* bl = a.blens + (size_t)draw * B;
  double* orow = a.out + (size_t)draw * (1 + B + R + K);
  const size_t NK = (size_t)N * K;
  double* LOW = wsb + GW_LOW * NK;
  double* CC = wsb + GW_C * NK;
  double* MSG = wsb + GW_MSG * NK;
  double* UT = wsb + GW_UT * NK;
  double* AA = wsb + GW_AA * NK;
  double* EE = wsb + GW_E * NK;
  double* UP = wsb + GW_UP * NK;
  double* sfac = wsb + GEO_WS_ARRAYS * NK;  // [N] 2^shift of each internal node
  double* sexp = sfac + N;                  // [N] the shift
  auto low = [&](int node) -> const double* { return node < S ? a.tips + (size_t)node * K : LOW + (size_t)node * K; };
  double* srow = nullptr;  // this draw's summary row
  if constexpr (SUM) srow = a.summ + (size_t)draw * (NK + (size_t)K * K + B);

  // ---- the parameters: refuse what has no likelihood
  {
    double bad = 0.0;
    for (int i = tid; i < K; i += nt) bad += (freqs[i] > 0.0 && isfinite(freqs[i])) ? 0.0 : 1.0;
    for (int i = tid; i < R; i += nt) bad += (rates[i] >= 0.0 && isfinite(rates[i])) ? 0.0 : 1.0;
    for (int i = tid; i < B; i += nt) bad += isfinite(bl[i]) ? 0.0 : 1.0;
    if (geo_block_sum(bad, red, tid, nt) != 0.0) return false;
  }
  for (int i = tid; i < K; i += nt) {
    const double f = freqs[i], r = sqrt(f);
    pi[i] = f;
    sq[i] = r;
    isq[i] = 1.0 / r;
  }
  __syncthreads();
  for (int i = tid; i < K; i += nt) {  // diagonal of the unnormalised Q (generate_script.py:922-926)
    double acc = 0.0;
    for (int j = 0; j < K; ++j)
      if (j != i) acc += rates[geo_rate_index(K, i, j)] * pi[j];
    qd[i] = -acc;
  }
  __syncthreads();
  const double s = geo_block_sum(tid < K ? -qd[tid] * pi[tid] : 0.0, red, tid, nt);
  if (!(s > 0.0) || !isfinite(s)) return false;
  // ---- A = D^1/2 Q D^-1/2 (symmetric to the bit: sq_i sq_j is commutative), V = I
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    A[i * KP + j] = i == j ? qd[i] / s : (sq[i] * sq[j]) * rates[geo_rate_index(K, i, j)] / s;
    V[i * KP + j] = i == j ? 1.0 : 0.0;
  }
  // ---- cyclic Jacobi, round-robin ordering: n - 1 rounds of n / 2 disjoint pairs (n = K, or K + 1 with a bye)
  const int n = K + (K & 1), nr = n - 1, np = n / 2;
  int sweeps = 0;
  bool converged = false;
  for (; sweeps <= GEO_SWEEP_CAP; ++sweeps) {
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

  // ---- pruning, level by level
  const double small = ldexp(1.0, GEO_SCALE_BELOW);
  const int wave = tid >> 6, lane = tid & 63, nwaves = nt >> 6;
  for (int lv = 0; lv < a.nlev; ++lv) {
    const int r0 = a.lvl_off[lv], nrow = a.lvl_off[lv + 1] - r0;
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // c = V^T (sqrt(pi) v), e = exp(lam t)
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, k = rem - which * K;
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* v = low(ch);
      double acc = 0.0;
      for (int j = 0; j < K; ++j) acc = fma(V[j * KP + k], sq[j] * v[j], acc);
      CC[(size_t)ch * K + k] = acc;
      EE[(size_t)ch * K + k] = exp(lam[k] * bl[ch]);
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // message = (V (e c)) / sqrt(pi)
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* e = EE + (size_t)ch * K;
      const double* c = CC + (size_t)ch * K;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(V[i * KP + k], e[k] * c[k], acc);
      MSG[(size_t)ch * K + i] = isq[i] * acc;
    }
    __syncthreads();
    for (int idx = wave; idx < nrow; idx += nwaves) {  // one wave per node: the product and its rescaling
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      const int ca = row[GR_A], cb = row[GR_B], p = row[GR_P];
      double x = 0.0;
      if (lane < K) x = MSG[(size_t)ca * K + lane] * (row[GR_LAST] ? low(cb)[lane] : MSG[(size_t)cb * K + lane]);
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
  const int root = 2 * S - 2;
  const double Ls = geo_block_sum(tid < K ? LOW[(size_t)root * K + tid] : 0.0, red, tid, nt);
  double shifts = 0.0;
  for (int node = S + tid; node < N; node += nt) shifts += sexp[node];
  shifts = geo_block_sum(shifts, red, tid, nt);  // integers: exact
  const double logL = log(Ls) - shifts * 0.693147180559945309417232121458;
  if (!(Ls > 0.0) || !isfinite(logL)) return false;

  // ---- reverse pass, top level first
  for (int i = tid; i < K; i += nt) UP[(size_t)root * K + i] = 1.0 / Ls;
  __syncthreads();
  for (int lv = a.nlev - 1; lv >= 0; --lv) {
    const int r0 = a.lvl_off[lv], nrow = a.lvl_off[lv + 1] - r0;
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // u~ = up[p] o (the sibling's message) 2^shift
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      const int ca = row[GR_A], cb = row[GR_B], p = row[GR_P], last = row[GR_LAST];
      const double upv = UP[(size_t)p * K + i] * sfac[p];
      if (!which)
        UT[(size_t)ca * K + i] = upv * (last ? low(cb)[i] : MSG[(size_t)cb * K + i]);
      else if (last)
        UP[(size_t)cb * K + i] = upv * MSG[(size_t)ca * K + i];  // the merged child: no branch of its own
      else
        UT[(size_t)cb * K + i] = upv * MSG[(size_t)ca * K + i];
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // a = V^T (u~ / sqrt(pi))
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, k = rem - which * K;
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* u = UT + (size_t)ch * K;
      double acc = 0.0;
      for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k], u[i] * isq[i], acc);
      AA[(size_t)ch * K + k] = acc;
    }
    __syncthreads();
    for (int it = tid; it < nrow * 2 * K; it += nt) {  // up[child] = sqrt(pi) (V (e a)) = P^T u~
      const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, j = rem - which * K;
      const int* row = a.rows + (size_t)(r0 + idx) * GR_INTS;
      if (which && row[GR_LAST]) continue;
      const int ch = row[which ? GR_B : GR_A];
      const double* e = EE + (size_t)ch * K;
      const double* aa = AA + (size_t)ch * K;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(V[j * KP + k], e[k] * aa[k], acc);
      UP[(size_t)ch * K + j] = sq[j] * acc;
    }
    __syncthreads();
  }
  if constexpr (SUM) {
    // ---- node marginals: low(n) o up[n] sums to 1 by multilinearity of L, the 2^shift of n cancelling (up[n] is
    // the derivative with respect to the scaled partial); the merged root child carries the root's row
    for (int it = tid; it < N * K; it += nt) {
      const int node = it / K, i = it - node * K, src = node == root - 1 ? root : node;
      srow[it] = low(src)[i] * UP[(size_t)src * K + i];
    }
  }

  // ---- branch gradients, W, and the direct D^{+-1/2} terms of P
  for (int b = tid; b < B; b += nt) {
    const double *aa = AA + (size_t)b * K, *e = EE + (size_t)b * K, *c = CC + (size_t)b * K;
    double acc = 0.0;
    for (int k = 0; k < K; ++k) acc = fma(aa[k] * lam[k], e[k] * c[k], acc);
    orow[1 + b] = acc;
  }
  for (int it = tid; it < K * K; it += nt) {
    const int k = it / K, l = it - k * K;
    const double ri = A[k * KP + l], lk = lam[k], ll = lam[l];
    double acc = 0.0;
    for (int b = 0; b < B; ++b) {
      const double Ek = EE[(size_t)b * K + k], El = EE[(size_t)b * K + l];
      const double phi = ri == 0.0 ? phi_close(lk, ll, bl[b], Ek, El) : (Ek - El) * ri;
      acc = fma(AA[(size_t)b * K + k] * CC[(size_t)b * K + l], phi, acc);
    }
    W[k * KP + l] = acc;
  }
  for (int i = tid; i < K; i += nt) {
    double rt = 0.0, ct = 0.0;
    for (int b = 0; b < B; ++b) {
      rt = fma(UT[(size_t)b * K + i], MSG[(size_t)b * K + i], rt);  // sum_b u~ o (P v)
      ct = fma(UP[(size_t)b * K + i], low(b)[i], ct);               // sum_b (P^T u~) o v
    }
    rowt[i] = rt;
    colt[i] = ct;
  }
  __syncthreads();
  // ---- dlogL/dA = sym(V W V^T)
  for (int it = tid; it < K * K; it += nt) {  // T = W V^T, over the spent 1 / (lam_k - lam_l)
    const int k = it / K, j = it - k * K;
    double acc = 0.0;
    for (int l = 0; l < K; ++l) acc = fma(W[k * KP + l], V[j * KP + l], acc);
    A[k * KP + j] = acc;
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {  // over the spent W
    const int i = it / K, j = it - i * K;
    double x = 0.0, y = 0.0;
    for (int k = 0; k < K; ++k) {
      x = fma(V[i * KP + k], A[k * KP + j], x);
      y = fma(V[j * KP + k], A[k * KP + i], y);
    }
    W[i * KP + j] = 0.5 * (x + y);
    if constexpr (SUM) {
      // x = G_ij, G = V W V^T = dlogL/dA entry by entry: E[i -> j transitions] = A_ij G_ij, E[time in i] = G_ii
      // (Minin & Suchard 2008; A_ij G_ij = Q_ij dlogL/dQ_ij).  A is spent: its entry again, as it was built
      srow[NK + it] = i == j ? x : ((sq[i] * sq[j]) * rates[geo_rate_index(K, i, j)] / s) * x;
    }
  }
  __syncthreads();
  // ---- chain rule: A = D^1/2 Q D^-1/2, Q = Qu / s, s = -sum_i Qu_ii pi_i, Qu_ii = -sum_{j != i} R_ij pi_j
  double part = 0.0;
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    const double qu = i == j ? qd[i] : rates[geo_rate_index(K, i, j)] * pi[j];
    part = fma(W[i * KP + j] * sq[i] * isq[j], qu, part);
  }
  const double ds = -geo_block_sum(part, red, tid, nt) / (s * s);
  for (int i = tid; i < K; i += nt) dd[i] = W[i * KP + i] / s - ds * pi[i];
  __syncthreads();
  double* g_rates = orow + 1 + B;
  double* g_freqs = g_rates + R;
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
    g_freqs[j] = 0.5 * (colt[j] - rowt[j]) / pi[j] - ds * qd[j] + acc;
  }
  if constexpr (SUM) {
    // ---- transitions per branch: n_b = sum_kl a_bk c_bl Phi_kl(t_b) M_kl, M = V^T A_off V.  V^T A V = diag(lam),
    // so M = diag(lam) - V^T diag(A) V: one K^3 product.  A and W are both spent: 1 / (lam_k - lam_l) again over
    // A, M over W
    __syncthreads();  // the chain rule has read W
    for (int it = tid; it < K * K; it += nt) {
      const int k = it / K, l = it - k * K;
      double acc = 0.0;
      for (int i = 0; i < K; ++i) acc = fma(V[i * KP + k] * V[i * KP + l], qd[i], acc);
      A[k * KP + l] = phi_rinv(lam[k], lam[l], PHI_NEAR);
      W[k * KP + l] = (k == l ? lam[k] : 0.0) - acc / s;
    }
    __syncthreads();
    double* bj = srow + NK + (size_t)K * K;
    for (int b = wave; b < B; b += nwaves) {  // one wave per branch, its K^2 terms in a fixed order
      const double *aa = AA + (size_t)b * K, *e = EE + (size_t)b * K, *c = CC + (size_t)b * K;
      const double t = bl[b];
      double acc = 0.0;
      for (int it = lane; it < K * K; it += 64) {
        const int k = it / K, l = it - k * K;
        const double ri = A[k * KP + l], Ek = e[k], El = e[l];
        const double phi = ri == 0.0 ? phi_close(lam[k], lam[l], t, Ek, El) : (Ek - El) * ri;
        acc = fma(aa[k] * c[l] * phi, W[k * KP + l], acc);
      }
      for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
      if (lane == 0) bj[b] = acc;
    }
  }
  if (tid == 0) orow[0] = logL;
  return true;
}

template <bool SUM>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_kernel(GeoArgsOf<SUM> a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  double* wsb = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const int rowlen = 1 + (2 * a.S - 3) + a.K * (a.K - 1) / 2 + a.K;
  for (int draw = blockIdx.x; draw < a.n; draw += gridDim.x) {
    if (a.sweeps && threadIdx.x == 0) a.sweeps[draw] = -1;
    const bool ok = geo_draw<SUM>(a, draw, sh, wsb);
    __syncthreads();  // the row's writers are done; LDS and the workspace are free for the next draw
    if (!ok) {
      double* orow = a.out + (size_t)draw * rowlen;
      for (int i = threadIdx.x; i < rowlen; i += blockDim.x) orow[i] = i == 0 ? -INFINITY : 0.0;
      if constexpr (SUM) {
        const int slen = (2 * a.S - 1) * a.K + a.K * a.K + (2 * a.S - 3);
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
  int dev_old = 0;
  (void)hipGetDevice(&dev_old);
  (void)hipSetDevice(c->device);
  for (void* p : {(void*)c->d_tips, (void*)c->d_blens, (void*)c->d_params, (void*)c->d_out, (void*)c->d_ws,
                  (void*)c->d_rows, (void*)c->d_lvl, (void*)c->d_sweeps, (void*)c->d_summ})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  (void)hipSetDevice(dev_old);
  delete c;
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
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, "phy_geo_eval: n_draws out of range");
  if (!blens || !params || !out) return fail(PHY_EINVAL, "NULL host buffer");
  const GeoPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_blens, blens, sizeof(double) * n * pl.B, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * geo_param_len(pl.K), hipMemcpyHostToDevice, st));
  GeoArgs a{};
  a.tips = ctx->d_tips, a.rows = ctx->d_rows, a.lvl_off = ctx->d_lvl;
  a.blens = ctx->d_blens, a.params = ctx->d_params, a.out = ctx->d_out, a.ws = ctx->d_ws, a.sweeps = ctx->d_sweeps;
  a.ws_stride = pl.ws_doubles, a.S = pl.S, a.K = pl.K, a.nlev = pl.nlev, a.n = n_draws;
  const int grid = std::min(n_draws, pl.workgroups);
  hipLaunchKernelGGL(geo_kernel<false>, dim3(grid), dim3(pl.threads), pl.lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(out, ctx->d_out, sizeof(double) * n * geo_row_len(pl.S, pl.K), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->last_n = n_draws;
  return PHY_OK;
}

int phy_geo_summary_len(const phy_geo_ctx* ctx) { return ctx ? geo_summary_len(ctx->plan.S, ctx->plan.K) : -1; }

int phy_geo_eval_summaries(phy_geo_ctx* ctx, int n_draws, const double* blens, const double* params, double* out,
                           double* summaries) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (n_draws < 1 || n_draws > ctx->max_draws)
    return fail(PHY_ERANGE, "phy_geo_eval_summaries: n_draws out of range");
  if (!blens || !params || !summaries) return fail(PHY_EINVAL, "NULL host buffer");
  const GeoPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t slen = (size_t)geo_summary_len(pl.S, pl.K);
  if (!ctx->d_summ) {  // a context that never asks pays for neither the buffer nor the second kernel's attribute
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
  hipLaunchKernelGGL(geo_kernel<true>, dim3(grid), dim3(pl.threads), pl.lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  if (out)
    HIP_TRY(hipMemcpyAsync(out, ctx->d_out, sizeof(double) * n * geo_row_len(pl.S, pl.K), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipMemcpyAsync(summaries, ctx->d_summ, sizeof(double) * n * slen, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  ctx->last_n = n_draws;
  return PHY_OK;
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
