// geo_trees.inc -- the discrete-trait likelihood over a sample of T trees on
// the same tips: the mixture L_mix = sum_t w_t L_t, its gradient with respect
// to rates_geo and freqs_geo, and the posterior summaries that do not depend on
// a topology (expected transitions, dwell times, the root's location).
// Included by phylo_hip.hip after geo_engine.inc, whose device helpers
// (geo_block_sum, geo_rate_index, jacobi_rot, phi_rinv, phi_close, GeoLds) it
// calls; geo_kernel and everything phy_geo_eval launches are not touched.
//
// The reference has no counterpart: its --geo model conditions on one tree.
//
//   grad log L_mix = sum_t p_t grad log L_t,  p_t = w_t L_t / L_mix.
// Given a draw's eigensystem the gradient rows are linear in what a tree leaves
// behind -- W_t = sum_b (a_b c_b^T) o Phi, colt - rowt, and for the summaries
// the root row low(root) o up[root] -- so their p_t-weighted sums are formed
// first and sym(V W V^T) and the chain rule run once per draw.  Three phases:
//   1. geo_trees_eig_kernel: one workgroup per draw, the Jacobi solve of
//      geo_draw, its results (ok, sweeps, s, lam, qd, V) to a per-draw record;
//   2. geo_trees_tree_kernel: one workgroup per (draw, group) item.  It loads
//      the record into LDS and walks the group's trees in ascending order: the
//      pruning and the reverse pass of geo_draw on tree t's schedule and branch
//      lengths, then W_t, colt - rowt and the root row folded into the item's
//      slot as sum_t exp(x_t - m) (.), x_t = log w_t + log L_t, m the running
//      maximum of x_t (the slot is rescaled by exp(m_old - m_new) when it
//      rises).  A tree whose exp(x_t - m) is 0 adds nothing and skips its
//      reverse pass; one without a finite log L_t has tree_ll = -inf and no
//      weight;
//   3. geo_trees_combine_kernel: one workgroup per draw merges the G slots in
//      ascending order (weights exp(m_g - M), M their maximum), forms log L_mix
//      = M + log Z, divides by Z, and runs W V^T, sym(V .) and the chain rule
//      exactly as geo_draw states them.
// Every sum has one fixed order that depends on the context alone (geo_plan.h:
// G and the split do not depend on n_draws), so a draw's rows are bitwise the
// same alone, in any batch and on repeat.  No atomics.
//
// A trait clock (phy_geo_trees_eval_clock): a draw's rate mu > 0 scales every
// branch of every tree, P_b = exp(Q mu t_b).  Phases 2 and 3 are templates on
// CLOCK; the plain calls instantiate CLOCK = false, which is the code as it was.
// With CLOCK the item loads mu once, forms t_eff = mu t_tb as one fp64 product
// wherever a branch length is read, and phase 3 forms
//   dlogL_mix/dmu = (1/mu) sum_k lam_k Wbar_kk
// from the p_t-weighted, Z-normalised W before W is overwritten: W_kk = sum_b
// a_bk c_bk t_eff e^{lam_k t_eff} and dlogL/dt_eff,b = sum_k a_bk lam_k e^{lam_k
// t_eff} c_bk, so sum_b t_eff,b dlogL/dt_eff,b = sum_k lam_k W_kk.  The slot
// layout does not change.  Dwell times leave as G_ii / mu, in the tree's unit.

struct GeoTreesArgs {
  const double* tips;    // [S][K]
  const int* rows;       // [T][S-1][GR_INTS]
  const int* lvl_off;    // tree t's level starts at lvl_start[t]
  const int* lvl_start;  // [T+1]
  const int* grp_off;    // [G+1]
  const double* blens;   // [T][B]
  const double* logw;    // [T]
  const double* params;  // [n][R+K]
  double* rec;           // [n][rec_doubles]
  double* slots;         // [chunk][G][slot_doubles]
  double* tree_ll;       // [n][T]
  double* out;           // [n][1+R+K], with CLOCK [n][2+R+K]
  double* summ;          // [n][K K + K], the summaries form only
  double* ws;            // [workgroups][ws_stride]
  size_t ws_stride;
  int S, K, T, G, n;
  int draw0, ndraw;  // the chunk of draws phases 2 and 3 run on
  const double* clock;  // [n] mu per draw, read by the CLOCK kernels alone; last, so that no other field moves
};

// ---- phase 1: the eigensystem of one draw (geo_draw's, to the record)
__device__ bool geo_trees_eigen(const GeoTreesArgs& a, int draw, double* sh, double* rec) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, R = K * (K - 1) / 2;
  const GeoLds L(K);
  const int KP = L.KP;
  double* A = sh + L.A();
  double* V = sh + L.V();
  double* sq = sh + L.vecs(1);
  double* pi = sh + L.vecs(3);
  double* qd = sh + L.vecs(4);
  double* rcs = sh + L.cs();
  double* rsn = sh + L.sn();
  double* red = sh + L.red();
  int* rp = reinterpret_cast<int*>(sh + L.pq());
  int* rq = rp + GEO_KMAX / 2;
  const double* rates = a.params + (size_t)draw * (R + K);
  const double* freqs = rates + R;
  {
    double bad = 0.0;
    for (int i = tid; i < K; i += nt) bad += (freqs[i] > 0.0 && isfinite(freqs[i])) ? 0.0 : 1.0;
    for (int i = tid; i < R; i += nt) bad += (rates[i] >= 0.0 && isfinite(rates[i])) ? 0.0 : 1.0;
    if (geo_block_sum(bad, red, tid, nt) != 0.0) return false;
  }
  for (int i = tid; i < K; i += nt) {
    const double f = freqs[i];
    pi[i] = f;
    sq[i] = sqrt(f);
  }
  __syncthreads();
  for (int i = tid; i < K; i += nt) {
    double acc = 0.0;
    for (int j = 0; j < K; ++j)
      if (j != i) acc += rates[geo_rate_index(K, i, j)] * pi[j];
    qd[i] = -acc;
  }
  __syncthreads();
  const double s = geo_block_sum(tid < K ? -qd[tid] * pi[tid] : 0.0, red, tid, nt);
  if (!(s > 0.0) || !isfinite(s)) return false;
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    A[i * KP + j] = i == j ? qd[i] / s : (sq[i] * sq[j]) * rates[geo_rate_index(K, i, j)] / s;
    V[i * KP + j] = i == j ? 1.0 : 0.0;
  }
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
      for (int it = tid; it < np * K; it += nt) {  // A <- A J, V <- V J
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
      for (int it = tid; it < np * K; it += nt) {  // A <- J^T A
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
  if (tid == 0) rec[GT_SWEEPS] = (double)sweeps, rec[GT_S] = s;
  if (!converged) return false;
  double* rlam = rec + GT_HEAD;
  double* rqd = rlam + K;
  double* rV = rqd + K;
  for (int i = tid; i < K; i += nt) rlam[i] = A[i * KP + i], rqd[i] = qd[i];
  for (int it = tid; it < K * K; it += nt) {
    const int i = it / K, j = it - i * K;
    rV[it] = V[i * KP + j];
  }
  return true;
}

__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_eig_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  const size_t reclen = GT_HEAD + 2 * (size_t)a.K + (size_t)a.K * a.K;
  for (int draw = blockIdx.x; draw < a.n; draw += gridDim.x) {
    double* rec = a.rec + (size_t)draw * reclen;
    if (threadIdx.x == 0) rec[GT_SWEEPS] = -1.0, rec[GT_S] = 0.0;
    const bool ok = geo_trees_eigen(a, draw, sh, rec);
    __syncthreads();  // LDS is free for the next draw
    if (threadIdx.x == 0) rec[GT_OK] = ok ? 1.0 : 0.0;
  }
}

// ---- phase 2: one (draw, group) item
template <bool CLOCK>
__device__ void geo_trees_group(const GeoTreesArgs& a, int draw, int g, double* slot, double* sh, double* wsb) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, S = a.S, N = 2 * S - 1, B = 2 * S - 3, R = K * (K - 1) / 2;
  const GeoLds L(K);
  const int KP = L.KP;
  double* A = sh + L.A();
  double* V = sh + L.V();
  double* lam = sh + L.vecs(0);
  double* sq = sh + L.vecs(1);
  double* isq = sh + L.vecs(2);
  double* red = sh + L.red();
  const double* freqs = a.params + (size_t)draw * (R + K) + R;
  const double* rec = a.rec + (size_t)draw * (GT_HEAD + 2 * (size_t)K + (size_t)K * K);
  const int t0 = a.grp_off[g], t1 = a.grp_off[g + 1];
  double* tll = a.tree_ll + (size_t)draw * a.T;
  __syncthreads();  // the previous item's readers of LDS and of the workspace are done
  double mu = 1.0;  // uniform over the workgroup: one load per item
  if constexpr (CLOCK) mu = a.clock[draw];
  bool dead = rec[GT_OK] == 0.0;
  if constexpr (CLOCK) dead = dead || !(mu > 0.0) || !isfinite(mu);
  if (dead) {  // no eigensystem (or no rate): every tree of the draw is -inf, the slot is empty
    for (int t = t0 + tid; t < t1; t += nt) tll[t] = -INFINITY;
    if (tid == 0) slot[GS_MAX] = -INFINITY, slot[GS_SUM] = 0.0;
    return;
  }
  const size_t NK = (size_t)N * K;
  double* LOW = wsb + GW_LOW * NK;
  double* CC = wsb + GW_C * NK;
  double* MSG = wsb + GW_MSG * NK;
  double* UT = wsb + GW_UT * NK;
  double* AA = wsb + GW_AA * NK;
  double* EE = wsb + GW_E * NK;
  double* UP = wsb + GW_UP * NK;
  double* sfac = wsb + GEO_WS_ARRAYS * NK;
  double* sexp = sfac + N;
  auto low = [&](int node) -> const double* { return node < S ? a.tips + (size_t)node * K : LOW + (size_t)node * K; };
  {
    const double* rlam = rec + GT_HEAD;
    const double* rV = rlam + 2 * K;
    for (int i = tid; i < K; i += nt) {
      const double r = sqrt(freqs[i]);
      lam[i] = rlam[i];
      sq[i] = r;
      isq[i] = 1.0 / r;
    }
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      V[i * KP + j] = rV[it];
    }
  }
  __syncthreads();
  for (int it = tid; it < K * K; it += nt) {  // 1 / (lam_k - lam_l), 0 inside the near window
    const int k = it / K, l = it - k * K;
    A[k * KP + l] = phi_rinv(lam[k], lam[l], PHI_NEAR);
  }
  const double small = ldexp(1.0, GEO_SCALE_BELOW);
  const int wave = tid >> 6, lane = tid & 63, nwaves = nt >> 6;
  const int root = 2 * S - 2;
  double m = -INFINITY, sumw = 0.0;  // uniform over the workgroup
  double* sW = slot + GS_HEAD;
  double* sv = sW + (size_t)K * K;
  double* sr = sv + K;
  for (int t = t0; t < t1; ++t) {
    const int* rows = a.rows + (size_t)t * (S - 1) * GR_INTS;
    const int* lvl = a.lvl_off + a.lvl_start[t];
    const int nlev = a.lvl_start[t + 1] - a.lvl_start[t] - 1;
    const double* bl = a.blens + (size_t)t * B;
    __syncthreads();  // the previous tree's fold has read the workspace; A is written
    // ---- pruning, level by level
    for (int lv = 0; lv < nlev; ++lv) {
      const int r0 = lvl[lv], nrow = lvl[lv + 1] - r0;
      for (int it = tid; it < nrow * 2 * K; it += nt) {  // c = V^T (sqrt(pi) v), e = exp(lam t)
        const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, k = rem - which * K;
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
        if (which && row[GR_LAST]) continue;
        const int ch = row[which ? GR_B : GR_A];
        const double* v = low(ch);
        double acc = 0.0;
        for (int j = 0; j < K; ++j) acc = fma(V[j * KP + k], sq[j] * v[j], acc);
        CC[(size_t)ch * K + k] = acc;
        if constexpr (CLOCK)
          EE[(size_t)ch * K + k] = exp(lam[k] * (mu * bl[ch]));
        else
          EE[(size_t)ch * K + k] = exp(lam[k] * bl[ch]);
      }
      __syncthreads();
      for (int it = tid; it < nrow * 2 * K; it += nt) {  // message = (V (e c)) / sqrt(pi)
        const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
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
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
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
    const double Ls = geo_block_sum(tid < K ? LOW[(size_t)root * K + tid] : 0.0, red, tid, nt);
    double shifts = 0.0;
    for (int node = S + tid; node < N; node += nt) shifts += sexp[node];
    shifts = geo_block_sum(shifts, red, tid, nt);  // integers: exact
    const double logL = log(Ls) - shifts * 0.693147180559945309417232121458;
    if (!(Ls > 0.0) || !isfinite(logL)) {  // no likelihood on this tree: no weight
      if (tid == 0) tll[t] = -INFINITY;
      continue;
    }
    if (tid == 0) tll[t] = logL;
    const double x = a.logw[t] + logL;
    const double mn = fmax(m, x);
    const bool first = m == -INFINITY;
    const double ro = first ? 0.0 : exp(m - mn);
    const double rn = exp(x - mn);
    if (rn == 0.0) continue;  // the term underflows against the group's maximum: exactly nothing

    // ---- reverse pass, top level first
    for (int i = tid; i < K; i += nt) UP[(size_t)root * K + i] = 1.0 / Ls;
    __syncthreads();
    for (int lv = nlev - 1; lv >= 0; --lv) {
      const int r0 = lvl[lv], nrow = lvl[lv + 1] - r0;
      for (int it = tid; it < nrow * 2 * K; it += nt) {  // u~ = up[p] o (the sibling's message) 2^shift
        const int idx = it / (2 * K), rem = it - idx * 2 * K, which = rem / K, i = rem - which * K;
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
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
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
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
        const int* row = rows + (size_t)(r0 + idx) * GR_INTS;
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
    // ---- W_t, colt - rowt and the root row, folded into the slot: each entry by one thread, always the same
    for (int it = tid; it < K * K; it += nt) {
      const int k = it / K, l = it - k * K;
      const double ri = A[k * KP + l], lk = lam[k], ll = lam[l];
      double acc = 0.0;
      for (int b = 0; b < B; ++b) {
        const double Ek = EE[(size_t)b * K + k], El = EE[(size_t)b * K + l];
        double phi;
        if constexpr (CLOCK)
          phi = ri == 0.0 ? phi_close(lk, ll, mu * bl[b], Ek, El) : (Ek - El) * ri;
        else
          phi = ri == 0.0 ? phi_close(lk, ll, bl[b], Ek, El) : (Ek - El) * ri;
        acc = fma(AA[(size_t)b * K + k] * CC[(size_t)b * K + l], phi, acc);
      }
      sW[it] = fma(acc, rn, first ? 0.0 : sW[it] * ro);
    }
    for (int i = tid; i < K; i += nt) {
      double rt = 0.0, ct = 0.0;
      for (int b = 0; b < B; ++b) {
        rt = fma(UT[(size_t)b * K + i], MSG[(size_t)b * K + i], rt);  // sum_b u~ o (P v)
        ct = fma(UP[(size_t)b * K + i], low(b)[i], ct);               // sum_b (P^T u~) o v
      }
      sv[i] = fma(ct - rt, rn, first ? 0.0 : sv[i] * ro);
      sr[i] = fma(LOW[(size_t)root * K + i] * UP[(size_t)root * K + i], rn, first ? 0.0 : sr[i] * ro);
    }
    sumw = fma(sumw, ro, rn);
    m = mn;
  }
  if (tid == 0) slot[GS_MAX] = m, slot[GS_SUM] = sumw;
}

template <bool CLOCK>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_tree_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  double* wsb = a.ws + (size_t)blockIdx.x * a.ws_stride;
  const size_t slotlen = GS_HEAD + (size_t)a.K * a.K + 2 * (size_t)a.K;
  const int items = a.ndraw * a.G;
  for (int item = blockIdx.x; item < items; item += gridDim.x) {
    const int dl = item / a.G, g = item - dl * a.G;
    geo_trees_group<CLOCK>(a, a.draw0 + dl, g, a.slots + (size_t)item * slotlen, sh, wsb);
  }
}

// ---- phase 3: one draw.  false: the mixture has no finite likelihood.
template <bool SUM, bool CLOCK>
__device__ bool geo_trees_combine(const GeoTreesArgs& a, int draw, const double* slots, double* sh) {
  const int tid = threadIdx.x, nt = blockDim.x;
  const int K = a.K, R = K * (K - 1) / 2, G = a.G;
  const GeoLds L(K);
  const int KP = L.KP;
  double* A = sh + L.A();
  double* V = sh + L.V();
  double* W = sh + L.W();
  double* sq = sh + L.vecs(1);
  double* isq = sh + L.vecs(2);
  double* pi = sh + L.vecs(3);
  double* qd = sh + L.vecs(4);
  double* dvec = sh + L.vecs(5);  // colt - rowt
  double* rrow = sh + L.vecs(6);  // the root row
  double* dd = sh + L.vecs(7);
  double* red = sh + L.red();     // first the G merge weights, then reduction scratch
  const double* rates = a.params + (size_t)draw * (R + K);
  const double* freqs = rates + R;
  const double* rec = a.rec + (size_t)draw * (GT_HEAD + 2 * (size_t)K + (size_t)K * K);
  const size_t slotlen = GS_HEAD + (size_t)K * K + 2 * (size_t)K;
  double* orow = a.out + (size_t)draw * (1 + R + K + (CLOCK ? 1 : 0));
  if (rec[GT_OK] == 0.0) return false;
  double mu = 1.0;
  if constexpr (CLOCK) {
    mu = a.clock[draw];
    if (!(mu > 0.0) || !isfinite(mu)) return false;
  }
  double M = -INFINITY;
  for (int g = 0; g < G; ++g) M = fmax(M, slots[(size_t)g * slotlen + GS_MAX]);
  if (!(M > -INFINITY) || !isfinite(M)) return false;
  for (int g = tid; g < G; g += nt) {
    const double mg = slots[(size_t)g * slotlen + GS_MAX];
    red[g] = mg == -INFINITY ? 0.0 : exp(mg - M);
  }
  __syncthreads();
  double Z = 0.0;
  for (int g = 0; g < G; ++g)
    if (red[g] != 0.0) Z = fma(slots[(size_t)g * slotlen + GS_SUM], red[g], Z);
  const double logL = M + log(Z);
  if (!(Z > 0.0) || !isfinite(logL)) return false;
  const double s = rec[GT_S];
  {
    const double* rqd = rec + GT_HEAD + K;
    const double* rV = rqd + K;
    for (int i = tid; i < K; i += nt) {
      const double f = freqs[i], r = sqrt(f);
      pi[i] = f;
      sq[i] = r;
      isq[i] = 1.0 / r;
      qd[i] = rqd[i];
    }
    for (int it = tid; it < K * K; it += nt) {
      const int i = it / K, j = it - i * K;
      V[i * KP + j] = rV[it];
    }
  }
  for (int it = tid; it < K * K + 2 * K; it += nt) {  // the G slots in ascending order, then / Z: the posterior mean
    double acc = 0.0;
    for (int g = 0; g < G; ++g) {
      const double sc = red[g];
      if (sc != 0.0) acc = fma(slots[(size_t)g * slotlen + GS_HEAD + it], sc, acc);
    }
    acc /= Z;
    if (it < K * K) {
      const int k = it / K, l = it - k * K;
      W[k * KP + l] = acc;
    } else if (it < K * K + K) {
      dvec[it - K * K] = acc;
    } else {
      rrow[it - K * K - K] = acc;
    }
  }
  __syncthreads();
  if constexpr (CLOCK) {  // dlogL_mix/dmu from the diagonal of W, which the next phase but one overwrites
    if (tid == 0) {
      const double* rlam = rec + GT_HEAD;
      double acc = 0.0;
      for (int k = 0; k < K; ++k) acc = fma(rlam[k], W[k * KP + k], acc);
      orow[1 + R + K] = acc / mu;
    }
  }
  // ---- dlogL/dA = sym(V W V^T)
  for (int it = tid; it < K * K; it += nt) {  // T = W V^T
    const int k = it / K, j = it - k * K;
    double acc = 0.0;
    for (int l = 0; l < K; ++l) acc = fma(W[k * KP + l], V[j * KP + l], acc);
    A[k * KP + j] = acc;
  }
  __syncthreads();
  double* srow = nullptr;
  if constexpr (SUM) srow = a.summ + (size_t)draw * ((size_t)K * K + K);
  for (int it = tid; it < K * K; it += nt) {  // over the spent W
    const int i = it / K, j = it - i * K;
    double x = 0.0, y = 0.0;
    for (int k = 0; k < K; ++k) {
      x = fma(V[i * KP + k], A[k * KP + j], x);
      y = fma(V[j * KP + k], A[k * KP + i], y);
    }
    W[i * KP + j] = 0.5 * (x + y);
    if constexpr (SUM) {
      // x = G_ij: E[i -> j transitions] = A_ij G_ij, E[time in i] = G_ii, A's entry again as it was built
      // with CLOCK the tree's lengths are t_eff / mu: the time in i leaves in the tree's unit
      if constexpr (CLOCK)
        srow[it] = i == j ? x / mu : ((sq[i] * sq[j]) * rates[geo_rate_index(K, i, j)] / s) * x;
      else
        srow[it] = i == j ? x : ((sq[i] * sq[j]) * rates[geo_rate_index(K, i, j)] / s) * x;
    }
  }
  if constexpr (SUM)
    for (int i = tid; i < K; i += nt) srow[(size_t)K * K + i] = rrow[i];
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
  double* g_rates = orow + 1;
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
    g_freqs[j] = 0.5 * dvec[j] / pi[j] - ds * qd[j] + acc;
  }
  if (tid == 0) orow[0] = logL;
  return true;
}

template <bool SUM, bool CLOCK>
__global__ void __launch_bounds__(GEO_MAX_THREADS) geo_trees_combine_kernel(GeoTreesArgs a) {
  extern __shared__ __attribute__((aligned(16))) char geo_smem[];
  double* sh = reinterpret_cast<double*>(geo_smem);
  const size_t slotlen = GS_HEAD + (size_t)a.K * a.K + 2 * (size_t)a.K;
  const int rowlen = 1 + a.K * (a.K - 1) / 2 + a.K + (CLOCK ? 1 : 0);
  for (int dl = blockIdx.x; dl < a.ndraw; dl += gridDim.x) {
    const int draw = a.draw0 + dl;
    __syncthreads();  // the previous draw's readers of LDS are done
    const bool ok = geo_trees_combine<SUM, CLOCK>(a, draw, a.slots + (size_t)dl * a.G * slotlen, sh);
    __syncthreads();
    if (!ok) {
      double* orow = a.out + (size_t)draw * rowlen;
      for (int i = threadIdx.x; i < rowlen; i += blockDim.x) orow[i] = i == 0 ? -INFINITY : 0.0;
      double* tll = a.tree_ll + (size_t)draw * a.T;
      for (int t = threadIdx.x; t < a.T; t += blockDim.x) tll[t] = -INFINITY;
      if constexpr (SUM) {
        double* srow = a.summ + (size_t)draw * ((size_t)a.K * a.K + a.K);
        for (int i = threadIdx.x; i < a.K * a.K + a.K; i += blockDim.x) srow[i] = 0.0;
      }
    }
  }
}

struct phy_geo_trees_ctx {
  GeoTreesPlan plan;
  int device = 0, max_draws = 0;
  hipStream_t stream = nullptr;
  double *d_tips = nullptr, *d_blens = nullptr, *d_logw = nullptr, *d_params = nullptr, *d_rec = nullptr;
  double *d_slots = nullptr, *d_tll = nullptr, *d_out = nullptr, *d_ws = nullptr;
  int *d_rows = nullptr, *d_lvl = nullptr, *d_lvs = nullptr, *d_grp = nullptr;
  double* d_summ = nullptr;  // [max_draws][K K + K], allocated by the first phy_geo_trees_eval_summaries
  double *d_clock = nullptr, *d_outc = nullptr;  // [max_draws], [max_draws][2+R+K]: the first clock call's
  bool attr_sum = false, attr_clock = false, attr_clock_sum = false;  // kernels whose LDS attribute is set
};

namespace {
void free_geo_trees(phy_geo_trees_ctx* c) {
  if (!c) return;
  int dev_old = 0;
  (void)hipGetDevice(&dev_old);
  (void)hipSetDevice(c->device);
  for (void* p : {(void*)c->d_tips, (void*)c->d_blens, (void*)c->d_logw, (void*)c->d_params, (void*)c->d_rec,
                  (void*)c->d_slots, (void*)c->d_tll, (void*)c->d_out, (void*)c->d_ws, (void*)c->d_rows,
                  (void*)c->d_lvl, (void*)c->d_lvs, (void*)c->d_grp, (void*)c->d_summ, (void*)c->d_clock,
                  (void*)c->d_outc})
    if (p) (void)hipFree(p);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  (void)hipSetDevice(dev_old);
  delete c;
}

template <bool SUM, bool CLOCK>
int geo_trees_launch(const GeoTreesPlan& pl, GeoTreesArgs& a, int n_draws, hipStream_t st) {
  hipLaunchKernelGGL(geo_trees_eig_kernel, dim3(std::min(n_draws, pl.draw_workgroups)), dim3(pl.threads),
                     pl.lds_bytes, st, a);
  HIP_TRY(hipGetLastError());
  for (int d0 = 0; d0 < n_draws; d0 += pl.chunk_draws) {  // a draw's rows do not depend on the chunk it falls in
    a.draw0 = d0, a.ndraw = std::min(pl.chunk_draws, n_draws - d0);
    const long long items = (long long)a.ndraw * pl.G;
    hipLaunchKernelGGL(geo_trees_tree_kernel<CLOCK>, dim3((int)std::min<long long>(items, pl.workgroups)),
                       dim3(pl.threads), pl.lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
    const dim3 cgrid(std::min(a.ndraw, pl.draw_workgroups));
    hipLaunchKernelGGL((geo_trees_combine_kernel<SUM, CLOCK>), cgrid, dim3(pl.threads), pl.lds_bytes, st, a);
    HIP_TRY(hipGetLastError());
  }
  return PHY_OK;
}

// the three phases of n_draws draws; sum takes the combine phase's summaries form, clock != NULL the CLOCK kernels
// (rows of 2 + R + K)
int geo_trees_run(phy_geo_trees_ctx* ctx, const char* who, int n_draws, const double* params, const double* clock,
                  bool with_clock, double* out, double* tree_ll, double* summaries, bool sum) {
  if (!ctx) return fail(PHY_EINVAL, std::string(who) + ": NULL ctx");
  if (n_draws < 1 || n_draws > ctx->max_draws) return fail(PHY_ERANGE, std::string(who) + ": n_draws out of range");
  if (!params || (sum ? !summaries : !out)) return fail(PHY_EINVAL, std::string(who) + ": NULL host buffer");
  if (with_clock && !clock) return fail(PHY_EINVAL, std::string(who) + ": clock is NULL");
  const GeoTreesPlan& pl = ctx->plan;
  HIP_TRY(hipSetDevice(ctx->device));
  const size_t slen = (size_t)geo_trees_summary_len(pl.K);
  const size_t rowlen = (size_t)geo_trees_row_len(pl.K) + (with_clock ? 1 : 0);
  // a context that never asks pays for neither the buffers nor the further kernels' attributes
  if (sum && !with_clock && !ctx->attr_sum) {
    HIP_TRY(hipFuncSetAttribute((const void*)geo_trees_combine_kernel<true, false>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_sum = true;
  }
  if (with_clock && !ctx->attr_clock) {
    for (const void* f : {(const void*)geo_trees_tree_kernel<true>, (const void*)geo_trees_combine_kernel<false, true>})
      HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_clock = true;
  }
  if (with_clock && sum && !ctx->attr_clock_sum) {
    HIP_TRY(hipFuncSetAttribute((const void*)geo_trees_combine_kernel<true, true>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
    ctx->attr_clock_sum = true;
  }
  if (sum && !ctx->d_summ) {
    const int rc = dalloc(&ctx->d_summ, (size_t)ctx->max_draws * slen);
    if (rc) return rc;
  }
  if (with_clock && !ctx->d_clock) {
    const int rc = dalloc(&ctx->d_clock, (size_t)ctx->max_draws);
    if (rc) return rc;
  }
  if (with_clock && !ctx->d_outc) {
    const int rc = dalloc(&ctx->d_outc, (size_t)ctx->max_draws * rowlen);
    if (rc) return rc;
  }
  hipStream_t st = ctx->stream;
  const size_t n = (size_t)n_draws;
  HIP_TRY(hipMemcpyAsync(ctx->d_params, params, sizeof(double) * n * geo_param_len(pl.K), hipMemcpyHostToDevice, st));
  if (with_clock) HIP_TRY(hipMemcpyAsync(ctx->d_clock, clock, sizeof(double) * n, hipMemcpyHostToDevice, st));
  GeoTreesArgs a{};
  a.tips = ctx->d_tips, a.rows = ctx->d_rows, a.lvl_off = ctx->d_lvl, a.lvl_start = ctx->d_lvs, a.grp_off = ctx->d_grp;
  a.blens = ctx->d_blens, a.logw = ctx->d_logw, a.params = ctx->d_params, a.rec = ctx->d_rec, a.slots = ctx->d_slots;
  a.clock = with_clock ? ctx->d_clock : nullptr;
  a.tree_ll = ctx->d_tll, a.out = with_clock ? ctx->d_outc : ctx->d_out, a.summ = ctx->d_summ, a.ws = ctx->d_ws;
  a.ws_stride = pl.ws_doubles;
  a.S = pl.S, a.K = pl.K, a.T = pl.T, a.G = pl.G, a.n = n_draws;
  const int rc = with_clock ? (sum ? geo_trees_launch<true, true>(pl, a, n_draws, st)
                                   : geo_trees_launch<false, true>(pl, a, n_draws, st))
                            : (sum ? geo_trees_launch<true, false>(pl, a, n_draws, st)
                                   : geo_trees_launch<false, false>(pl, a, n_draws, st));
  if (rc) return rc;
  if (out) HIP_TRY(hipMemcpyAsync(out, a.out, sizeof(double) * n * rowlen, hipMemcpyDeviceToHost, st));
  if (tree_ll) HIP_TRY(hipMemcpyAsync(tree_ll, ctx->d_tll, sizeof(double) * n * pl.T, hipMemcpyDeviceToHost, st));
  if (sum) HIP_TRY(hipMemcpyAsync(summaries, ctx->d_summ, sizeof(double) * n * slen, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return PHY_OK;
}
}  // namespace

extern "C" {

int phy_geo_trees_create(int S, int K, const double* tip_partials, int T, const int32_t* peels, const double* blens,
                         const double* log_weights, int max_draws, int device, phy_geo_trees_ctx** out) {
  g_err.clear();
  if (!out) return fail(PHY_EINVAL, "out is NULL");
  *out = nullptr;
  if (!tip_partials) return fail(PHY_EINVAL, "phy_geo_trees_create: tip_partials is NULL");
  if (!blens) return fail(PHY_EINVAL, "phy_geo_trees_create: blens is NULL");
  GeoTreesPlan made;
  int rc = geo_trees_plan(S, K, T, peels, max_draws, 1, made);  // refusals before any device call
  if (rc) return rc;
  for (size_t i = 0; i < (size_t)S * K; ++i)
    if (!(tip_partials[i] >= 0.0 && tip_partials[i] <= 1.0))
      return fail(PHY_EINVAL, "phy_geo_trees_create: tip partials must lie in [0, 1]");
  const size_t B = (size_t)made.B;
  for (size_t i = 0; i < (size_t)T * B; ++i)
    if (!std::isfinite(blens[i]))
      return fail(PHY_EINVAL, "phy_geo_trees_create: tree " + std::to_string(i / B) + ": branch length " +
                                  std::to_string(i % B) + " is not finite");
  std::vector<double> logw((size_t)T, -std::log((double)T));
  if (log_weights)
    for (int t = 0; t < T; ++t) {
      if (!std::isfinite(log_weights[t]))
        return fail(PHY_EINVAL, "phy_geo_trees_create: tree " + std::to_string(t) + ": log weight is not finite");
      logw[t] = log_weights[t];
    }
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(PHY_EINVAL, "bad device ordinal");
  std::unique_ptr<phy_geo_trees_ctx, void (*)(phy_geo_trees_ctx*)> c(new phy_geo_trees_ctx(), free_geo_trees);
  HIP_TRY(hipSetDevice(device));
  c->device = device;
  c->max_draws = max_draws;
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus < 1) cus = 256;
  if ((rc = geo_trees_plan(S, K, T, peels, max_draws, cus, c->plan))) return rc;
  const GeoTreesPlan& pl = c->plan;
  for (const void* f : {(const void*)geo_trees_eig_kernel, (const void*)geo_trees_tree_kernel<false>,
                        (const void*)geo_trees_combine_kernel<false, false>})
    HIP_TRY(hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)GEO_LDS_CAP));
  HIP_TRY(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
  const size_t nd = (size_t)max_draws;
  const size_t wgs = (size_t)std::min<long long>((long long)pl.chunk_draws * pl.G, pl.workgroups);
  if ((rc = dalloc(&c->d_tips, (size_t)S * K)) || (rc = dalloc(&c->d_rows, pl.rows.size())) ||
      (rc = dalloc(&c->d_lvl, pl.lvl_off.size())) || (rc = dalloc(&c->d_lvs, pl.lvl_start.size())) ||
      (rc = dalloc(&c->d_grp, pl.grp_off.size())) || (rc = dalloc(&c->d_blens, (size_t)T * B)) ||
      (rc = dalloc(&c->d_logw, (size_t)T)) || (rc = dalloc(&c->d_params, nd * geo_param_len(K))) ||
      (rc = dalloc(&c->d_rec, nd * pl.rec_doubles)) ||
      (rc = dalloc(&c->d_slots, (size_t)pl.chunk_draws * pl.G * pl.slot_doubles)) ||
      (rc = dalloc(&c->d_tll, nd * (size_t)T)) || (rc = dalloc(&c->d_out, nd * geo_trees_row_len(K))) ||
      (rc = dalloc(&c->d_ws, wgs * pl.ws_doubles)))
    return rc;
  HIP_TRY(hipMemcpy(c->d_tips, tip_partials, sizeof(double) * S * K, hipMemcpyHostToDevice));
  HIP_TRY(hipMemcpy(c->d_blens, blens, sizeof(double) * (size_t)T * B, hipMemcpyHostToDevice));
  if ((rc = upload(c->d_rows, pl.rows)) || (rc = upload(c->d_lvl, pl.lvl_off)) ||
      (rc = upload(c->d_lvs, pl.lvl_start)) || (rc = upload(c->d_grp, pl.grp_off)) || (rc = upload(c->d_logw, logw)))
    return rc;
  *out = c.release();
  return PHY_OK;
}

int phy_geo_trees_destroy(phy_geo_trees_ctx* ctx) {
  free_geo_trees(ctx);
  return PHY_OK;
}

int phy_geo_trees_num_trees(const phy_geo_trees_ctx* ctx) { return ctx ? ctx->plan.T : -1; }

int phy_geo_trees_output_len(const phy_geo_trees_ctx* ctx) { return ctx ? geo_trees_row_len(ctx->plan.K) : -1; }

int phy_geo_trees_summary_len(const phy_geo_trees_ctx* ctx) { return ctx ? geo_trees_summary_len(ctx->plan.K) : -1; }

int phy_geo_trees_eval(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out, double* tree_ll) {
  return geo_trees_run(ctx, "phy_geo_trees_eval", n_draws, params, nullptr, false, out, tree_ll, nullptr, false);
}

int phy_geo_trees_eval_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params, double* out,
                                 double* tree_ll, double* summaries) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_summaries", n_draws, params, nullptr, false, out, tree_ll, summaries,
                       true);
}

int phy_geo_trees_clock_output_len(const phy_geo_trees_ctx* ctx) {
  return ctx ? geo_trees_row_len(ctx->plan.K) + 1 : -1;
}

int phy_geo_trees_eval_clock(phy_geo_trees_ctx* ctx, int n_draws, const double* params, const double* clock,
                             double* out, double* tree_ll) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_clock", n_draws, params, clock, true, out, tree_ll, nullptr, false);
}

int phy_geo_trees_eval_clock_summaries(phy_geo_trees_ctx* ctx, int n_draws, const double* params, const double* clock,
                                       double* out, double* tree_ll, double* summaries) {
  return geo_trees_run(ctx, "phy_geo_trees_eval_clock_summaries", n_draws, params, clock, true, out, tree_ll,
                       summaries, true);
}

int phy_geo_trees_info(const phy_geo_trees_ctx* ctx, int* widest_level, int* max_levels, int* groups, int* threads,
                       int* lds_bytes, int* workgroups) {
  if (!ctx) return fail(PHY_EINVAL, "NULL ctx");
  if (widest_level) *widest_level = ctx->plan.widest;
  if (max_levels) *max_levels = ctx->plan.max_nlev;
  if (groups) *groups = ctx->plan.G;
  if (threads) *threads = ctx->plan.threads;
  if (lds_bytes) *lds_bytes = (int)ctx->plan.lds_bytes;
  if (workgroups) *workgroups = ctx->plan.workgroups;
  return PHY_OK;
}

}  // extern "C"
