// quad_engine.inc -- the small-batch pattern sweep with a QUAD of lanes per
// (pattern, category) column; included by phylo_hip.hip after sweep_kernel
// (uses SweepArgs, the ST_* / F_* step fields, V4, dpp_d, swap32 / swap16, build_record,
// flags and the finalize's slot layouts).
//
// A sampler's call carries a few draws (NUTS: one per chain; phylostan's
// default ADVI gradient: one), so the one-column-per-lane latency plan runs
// one wave per SIMD on a few dozen SIMDs and its time is the serial chain of
// one wave's instructions: ~270 per program step, 16-FMA mat-vecs per lane
// and a 63-instruction transpose-reduce of a 16-entry outer product per
// branch (DESIGN.md 7, r03 SQ counters).  Here lane 4 col + i owns state i of
// column col (16 columns per wave), so
//   * a mat-vec is 4 FMAs per lane on operands shared inside the quad by DPP
//     (P v: row i of P against v broadcast from the quad; P^T r: column i);
//   * the outer product r (x) p of a branch is 4 products per lane (lane i
//     forms row i), reduced over the wave's 16 columns in 15 instructions;
//   * the same program (build_program's post-order steps, deep stack) runs,
//     every matrix record of the (draw, category) staged in LDS once;
//   * 4x the waves over the SIMDs for the same columns.
// Moved partials a_v (one double per lane) go to a per-workgroup global
// scratch in the forward and come back in the reverse, one step ahead (the
// step records, tip operands and matrix rows a step ahead too measured slower:
// fluA 4 draws 118 against 112 us per call, HCV 113 against 106, r04g -- the
// step's scalar loads share lgkmcnt with the LDS reads it waits on).  The
// dL/dP and scalar slots are the pattern sweep's (a wave's slot: a plain
// store in its workgroup's first block, atomic adds after, same address
// order: bitwise reproducible); the epilogue is qfin_kernel (phylo_hip.hip),
// split over workgroups.
//
// qsweep_kernel and qmw_kernel (below) run that program to the same bits: what
// both compute is stated once, in QLane; what each loads when is a measurement
// and stays in it, as do the wave sums (shared, they cost 1 %: DESIGN.md 5d).

struct QuadArgs {
  SweepArgs s;
  double* qscr;  // [wg][nslots][C][64] moved partials, one double per lane
  int nblk;      // 16-column blocks
  // build: the waves form their (draw, category)'s matrix records from the
  // eigensystem (s.eig) straight into LDS -- no pmat launch ahead of the
  // sweep; the draw's first workgroup also stores them (s.pmat) for the
  // epilogue.  build_record's arithmetic: pmat_kernel's bits.
  double* pmat_out;
  int build;
};

// lane j's value (j = 0..3 inside the quad) in every lane of the quad
template <int J>
__device__ __forceinline__ double qbc(double v) {
  return dpp_d<J * 0x55>(v);  // quad_perm [J, J, J, J]
}

// the 4 products v[k] of this lane (row i of an outer product, k = 0..3)
// summed over the wave's 16 columns (lane bits 2..5); on return lanes with
// bits 2, 3 clear hold entry (i, k) with k = b4 + 2 b5 -- a fixed tree:
// deterministic
__device__ __forceinline__ double qreduce(double (&v)[4]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) {  // bit 5: lanes < 32 keep k = u, >= 32 k = u + 2
    swap32(v[u], v[u + 2]);
    v[u] += v[u + 2];
  }
  swap16(v[0], v[1]);  // bit 4: even rows keep k = 2 b5, odd rows 2 b5 + 1
  v[0] += v[1];
  v[0] += dpp_d<DPP_ROW_ROR8>(v[0]);  // bit 3
  v[0] += dpp_d<0x124>(v[0]);         // bit 2 (row_ror:4, symmetric after the ror:8 stage)
  return v[0];
}

struct QStep {
  int xt, yt, mxb, myb, mvb, vso, fl, xso, yso, xdo, vdo, mxg, myg, mvg;
};
__device__ __forceinline__ QStep ld_qstep_raw(const int* __restrict__ prog, int s) {
  const int4* q = reinterpret_cast<const int4*>(prog + s * STEP_INTS);
  const int4 a = q[0], b = q[1], c = q[2], d = q[3];
  return {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w, d.x, d.y};
}
// every field in SGPRs here (the record's scalar loads complete before this point)
__device__ __forceinline__ void qpin(const QStep& t) {
  asm volatile("" ::"s"(t.xt), "s"(t.yt), "s"(t.mxb), "s"(t.myb), "s"(t.mvb), "s"(t.vso), "s"(t.fl), "s"(t.xso),
               "s"(t.yso), "s"(t.xdo), "s"(t.vdo), "s"(t.mxg), "s"(t.myg), "s"(t.mvg));
}
__device__ __forceinline__ QStep ld_qstep(const int* __restrict__ prog, int s) {
  const QStep t = ld_qstep_raw(prog, s);
  qpin(t);
  return t;
}

// lane m of the category-c wave builds matrices m, m + 64, ... of the draw
// into the wave's LDS records, entry by entry (build_record's arithmetic and
// order, so pmat_kernel's bits, without holding a 16-entry P in registers:
// the sweep loop's register budget is the kernel's)
__device__ __forceinline__ void qbuild_records(const SweepArgs& a, const double* se, int draw, int c, double* mats,
                                               int lane, int m0 = 0, int mstride = WAVE) {
  const double rc = a.model[(size_t)draw * (10 + 2 * a.C) + 10 + c];
  const int rec = a.R * 4;
  for (int m = m0 + lane; m < a.nmat; m += mstride) {
    const double t = a.blens[(size_t)draw * a.B + a.mat_branch[m]] * rc;
    double* R0 = mats + (size_t)m * rec;  // column j of P at R0[4 j]
    if (a.kind == PHY_JC69) {
      const double ex = exp(-t / 0.75);
      const double off = 0.25 - 0.25 * ex, d = 0.25 + 0.75 * ex;
      for (int q = 0; q < 16; ++q) R0[q] = (q % 5 == 0) ? d : off;
    } else {
      double E[4];
#pragma unroll
      for (int l = 0; l < 4; ++l) E[l] = exp(se[EIG_LAM + l] * t);
      for (int i = 0; i < 4; ++i) {  // row i of P, then row i of each extra-mask vector from it
        double Pi[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          double acc = 0.0;
#pragma unroll
          for (int l = 0; l < 4; ++l) acc = fma(se[EIG_M1 + i * 4 + l] * E[l], se[EIG_M2 + l * 4 + j], acc);
          Pi[j] = acc;
          R0[j * 4 + i] = acc;
        }
        for (int v = 4; v < a.R; ++v) {
          const unsigned tm = (unsigned)(a.extra >> (4 * (v - 4))) & 15u;
          double acc = Pi[0] * (double)(tm & 1u);
#pragma unroll
          for (int j = 1; j < 4; ++j) acc = fma(Pi[j], (double)((tm >> j) & 1u), acc);
          R0[v * 4 + i] = acc;
        }
      }
      continue;
    }
    for (int v = 4; v < a.R; ++v) {  // JC69: the extra-mask vectors from the stored rows
      const unsigned tm = (unsigned)(a.extra >> (4 * (v - 4))) & 15u;
      for (int i = 0; i < 4; ++i) {
        double acc = R0[i] * (double)(tm & 1u);
#pragma unroll
        for (int j = 1; j < 4; ++j) acc = fma(R0[j * 4 + i], (double)((tm >> j) & 1u), acc);
        R0[v * 4 + i] = acc;
      }
    }
  }
}

// The tip state vectors' LDS table ([16][4]: tipvec_b of every record index), by the workgroup's first 64 threads.
__device__ __forceinline__ void fill_tipvecs(double* tvec, unsigned long long extra) {
  if (threadIdx.x < 64) {
    const unsigned b = threadIdx.x >> 2, j = threadIdx.x & 3;
    const unsigned m = b < 4 ? (1u << b) : (unsigned)(extra >> (4 * (b - 4))) & 15u;
    tvec[threadIdx.x] = (double)((m >> j) & 1u);
  }
}

// This block's tip nibbles, by the whole workgroup: S rows of 8 bytes.
__device__ __forceinline__ void stage_tip_nibbles(const SweepArgs& a, unsigned char* tipl, int blk) {
  const uint32_t* src = reinterpret_cast<const uint32_t*>(a.tips);
  uint32_t* dst = reinterpret_cast<uint32_t*>(tipl);
  const int rowq = a.Ppad / 8;
  for (int k = threadIdx.x; k < a.S * 2; k += blockDim.x) dst[k] = src[(size_t)(k >> 1) * rowq + blk * 2 + (k & 1)];
}

// A lane of either quad sweep -- state st of column col in category c's wave -- and the arithmetic both
// kernels run, on values the caller has loaded.  st, col and gfirst are REFERENCES to the kernel's locals and
// LDS addresses are formed by the caller: otherwise the kernels compile to other spills (DESIGN.md 5d).
struct QLane {
  const int &st, &col;
  const bool& gfirst;                 // wave-uniform: the first block stores to the dL/dP slot, later ones add
  const unsigned char* const mbytes;  // the category's matrix records
  double *const tvec, *const gs;      // tip state vectors [16][4]; the wave's dL/dP slot
  const bool gowner;                  // the lanes that hold a sum: its entry gent = (i, k)
  const int gent, c;
  const V4 pi;
  const double pi_st, ps_c;

  // this column's nibble of the byte it shares with its neighbour
  __device__ __forceinline__ unsigned nib(unsigned n) const { return (n >> ((col & 1) * 4)) & 15u; }
  // (P t_b)[i] of the record at byte offset mb
  __device__ __forceinline__ double recv(int mb, unsigned b) const {
    return *reinterpret_cast<const double*>(mbytes + mb + b * 32 + st * 8);
  }
  __device__ __forceinline__ void gput(int mg, double s) const {  // mg: the matrix's slot offset
    if (gowner) {
      if (gfirst)
        gs[mg + gent] = s;
      else
        unsafeAtomicAdd(gs + mg + gent, s);
    }
  }
  // dL/dP_m += r (x) p (p spread over the quad)
  __device__ __forceinline__ void gq(int m, double r, double p) const {
    double v[4] = {r * qbc<0>(p), r * qbc<1>(p), r * qbc<2>(p), r * qbc<3>(p)};
    gput(m, qreduce(v));
  }
  // dL/dP_m += r (x) t_b (a tip's 0/1 state vector)
  __device__ __forceinline__ void gt(int m, double r, unsigned b) const {
    const double2* t = reinterpret_cast<const double2*>(tvec + b * 4);
    const double2 t01 = t[0], t23 = t[1];
    double v[4] = {r * t01.x, r * t01.y, r * t23.x, r * t23.y};
    gput(m, qreduce(v));
  }
  // forward step: (P p)[i] in pv_row's order from row i of P (m0, m4, m8, m12), p = a_x a_y
  __device__ __forceinline__ static double pv(double p, double m0, double m4, double m8, double m12) {
    const double v0 = qbc<0>(p), v1 = qbc<1>(p), v2 = qbc<2>(p), v3 = qbc<3>(p);
    return fma(m12, v3, fma(m8, v2, fma(m4, v1, m0 * v0)));
  }
  // reverse step: r_v through P_v^T in ptv_col's order (column i: c01, c23) where the step has a matrix
  // (F_MV; the merged root branch is the identity), the dL/dP terms of that matrix and of the tip
  // children's (records bx, by); -> (r_x, r_y)
  __device__ __forceinline__ double2 reverse(int fl, int xt, int yt, int mxg, int myg, int mvg, double rv, double ax,
                                             double ay, double2 c01, double2 c23, unsigned bx, unsigned by) const {
    const double r0 = qbc<0>(rv), r1 = qbc<1>(rv), r2 = qbc<2>(rv), r3 = qbc<3>(rv);
    const double ptr = fma(c23.y, r3, fma(c23.x, r2, fma(c01.y, r1, c01.x * r0)));
    const double q = (fl & F_MV) ? ptr : rv;
    if (fl & F_MV) gq(mvg, rv, ax * ay);  // dL/dP_v += r_v (x) p_v
    const double rx = q * ay, ry = q * ax;
    if (xt >= 0) gt(mxg, rx, bx);
    if (yt >= 0) gt(myg, ry, by);
    return make_double2(rx, ry);
  }
  // the root: vdot(pi, p_root); each column's lane 0 publishes the category's term of the site likelihood (slot)
  __device__ __forceinline__ double root_put(double proot, double* slot) const {
    const double q0 = qbc<0>(proot), q1 = qbc<1>(proot), q2 = qbc<2>(proot), q3 = qbc<3>(proot);
    const double fp = fma(pi.w, q3, fma(pi.z, q2, fma(pi.y, q1, pi.x * q0)));
    if (st == 0) *slot = ps_c * fp;
    return fp;
  }
  // past the barrier: the site's log L over the categories (xcol: the column's entries) and the accumulators; -> the root's r
  __device__ __forceinline__ double site(const SweepArgs& a, const double* xcol, int draw, int blk, double fp,
                                         double proot, double& acc_ll, double& acc_dps, double& acc_f) const {
    double L = 0.0;
    for (int cc = 0; cc < a.C; ++cc) L += xcol[cc * QCOLS];
    const int i = blk * QCOLS + col;
    const bool live = i < a.P;
    const double wt = a.weights[i];  // 0 on padding
    if (st == 0) {
      const double lnL = live ? log(L) : 0.0;
      if (c == 0) {
        acc_ll += wt * lnL;
        if (a.site_ll != nullptr && live) a.site_ll[(size_t)draw * a.P + i] = lnL;
      }
    }
    const double sc = live ? wt / L : 0.0;
    const double s_c = sc * ps_c;
    if (st == 0) acc_dps = fma(sc, fp, acc_dps);
    acc_f = fma(s_c, proot, acc_f);  // this lane's component of the root frequency term
    return pi_st * s_c;
  }
};

// MAXT: 256 when C <= 4 (one wave per category: the register budget of one
// wave per SIMD, which is all a small call puts there), else 1024
template <int MAXT>
__global__ void __launch_bounds__(MAXT) qsweep_kernel(QuadArgs qa, const int* __restrict__ prog) {
  const SweepArgs& a = qa.s;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int c = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int C = a.C, nsteps = a.nsteps, nmat = a.nmat, ndeep = a.ndeep;
  const int col = lane >> 2, st = lane & 3;
  const int draw = blockIdx.y;
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  const int rec = a.R * 4;  // doubles per matrix record
  const QuadLds lds(a.S, C, nmat, a.R, ndeep, false);
  double* mats0 = reinterpret_cast<double*>(lds_raw);
  double* tvec = mats0 + lds.recs;
  double* xch = tvec + lds.tvec;
  double* deep = xch + lds.xch + (size_t)c * ndeep * WAVE;
  unsigned char* tipl = reinterpret_cast<unsigned char*>(xch + lds.xch + lds.tail);
  double* mats = mats0 + (size_t)c * nmat * rec;
  fill_tipvecs(tvec, a.extra);
  if (qa.build) {  // this wave's records, built here (lane m owns matrices m, m + 64, ...)
    __shared__ double se[EIG_LEN];
    if (threadIdx.x < EIG_LEN) se[threadIdx.x] = a.eig[(size_t)draw * EIG_LEN + threadIdx.x];
    __syncthreads();
    qbuild_records(a, se, draw, c, mats, lane);
    if (blockIdx.x == 0) {  // the epilogue's copy: the wave's records as one contiguous run
      __syncthreads();
      const double2* src = reinterpret_cast<const double2*>(mats);
      double2* dst = reinterpret_cast<double2*>(qa.pmat_out + ((size_t)draw * C + c) * nmat * rec);
      for (int k = lane; k < nmat * rec / 2; k += WAVE) dst[k] = src[k];
    }
  } else {  // this wave's records: every matrix of the (draw, category), once
    const double2* src = reinterpret_cast<const double2*>(a.pmat + ((size_t)draw * C + c) * nmat * rec);
    double2* dst = reinterpret_cast<double2*>(mats);
    const int q2 = nmat * rec / 2;
    for (int k0 = lane; k0 < q2; k0 += WAVE * 8) {
      double2 buf[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u * WAVE;
        buf[u] = (k < q2) ? src[k] : make_double2(0.0, 0.0);
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int k = k0 + u * WAVE;
        if (k < q2) dst[k] = buf[u];
      }
    }
  }
  const double* mdl = a.model + (size_t)draw * (10 + 2 * C);
  const V4 pi = {mdl[0], mdl[1], mdl[2], mdl[3]};
  const double pi_st = st == 0 ? pi.x : st == 1 ? pi.y : st == 2 ? pi.z : pi.w;
  const double ps_c = mdl[10 + C + c];
  double* scr = qa.qscr + (size_t)wg * a.nslots * C * WAVE + (size_t)c * WAVE + lane;  // + slot * C * 64
  double* gs = a.gslot + ((size_t)wg * C + c) * nmat * 16;
  bool gfirst = true;  // wave-uniform
  const bool gowner = (lane & 12) == 0;
  const int gent = st * 4 + ((lane >> 4) & 1) + 2 * ((lane >> 5) & 1);  // entry (i, k) of this lane's sum
  const unsigned char* mbytes = reinterpret_cast<const unsigned char*>(mats);
  double acc_ll = 0.0, acc_dps = 0.0, acc_f = 0.0;
  const QLane ln{.st = st, .col = col, .gfirst = gfirst, .mbytes = mbytes, .tvec = tvec, .gs = gs, .gowner = gowner,
                 .gent = gent, .c = c, .pi = pi, .pi_st = pi_st, .ps_c = ps_c};

  for (int blk = blockIdx.x; blk < qa.nblk; blk += gridDim.x) {
    __syncthreads();  // the previous block's tip / exchange reads are done (first pass: records staged)
    stage_tip_nibbles(a, tipl, blk);
    __syncthreads();
    // ---- forward
    double top = 0.0, proot = 0.0;
    QStep tf = ld_qstep(prog, 0);
    for (int s = 0; s < nsteps; ++s) {
      qpin(tf);  // issued during the previous step, after its LDS waits
      const QStep t = tf;
      // every LDS read of the step issued together, branch-free (the fields
      // default to valid offsets): one round trip for the tips' nibbles,
      // one for their records, the deep entry and the matrix row
      const unsigned nx = tipl[max(t.xt, 0) + (col >> 1)], ny = tipl[max(t.yt, 0) + (col >> 1)];
      const double dx = deep[t.xdo + lane];
      const double* M = reinterpret_cast<const double*>(mbytes + t.mvb) + st;
      double m0 = M[0], m4 = M[4], m8 = M[8], m12 = M[12];
      // keep the row's reads here, with the nibble and deep reads (the
      // compiler would sink them behind the root-step branch: a third round)
      asm volatile("" : "+v"(m0), "+v"(m4), "+v"(m8), "+v"(m12));
      const double tx = ln.recv(t.mxb, ln.nib(nx)), ty = ln.recv(t.myb, ln.nib(ny));
      const double ay = t.yt >= 0 ? ty : top;
      const double ax = t.xt >= 0 ? tx : (t.yt >= 0 ? top : dx);
      // P v formed on every step and selected (the merged root branch is the
      // identity): the matrix row's reads then issue with the step's other
      // LDS reads instead of behind a branch
      const double p = ax * ay;
      const double pv = QLane::pv(p, m0, m4, m8, m12);
      // the next step's record: its scalar loads share lgkmcnt with the LDS
      // reads, so they go out only after this step's last LDS wait
      asm volatile("" ::: "memory");
      if (s + 1 < nsteps) tf = ld_qstep_raw(prog, s + 1);
      if (t.vso >= 0) {
        const double av = (t.fl & F_MV) ? pv : p;
        scr[t.vso] = av;
        if (t.fl & F_VDEEP) deep[t.vdo + lane] = av;
        top = av;
      } else {
        proot = p;
      }
    }
    // ---- root / site log L
    const double fp = ln.root_put(proot, xch + c * QCOLS + col);
    __syncthreads();
    double topr = ln.site(a, xch + col, draw, blk, fp, proot, acc_ll, acc_dps, acc_f);
    // ---- reverse (operands from scratch one step ahead)
    auto lx_of = [&](const QStep& u) __attribute__((always_inline)) -> double {
      return u.xt < 0 ? scr[u.xso] : 0.0;
    };
    auto ly_of = [&](const QStep& u) __attribute__((always_inline)) -> double {
      return u.yt < 0 ? scr[u.yso] : 0.0;
    };
    // step records two steps ahead (issued after a step's LDS waits), the
    // scratch operands one step ahead
    QStep tn = ld_qstep(prog, nsteps - 1);
    QStep tnn = ld_qstep(prog, nsteps > 1 ? nsteps - 2 : 0);
    double lxn = lx_of(tn), lyn = ly_of(tn);
    for (int s = nsteps - 1; s >= 0; --s) {
      const QStep t = tn;
      const double lx = lxn, ly = lyn;
      if (s > 0) {
        qpin(tnn);
        tn = tnn;
        lxn = lx_of(tn);
        lyn = ly_of(tn);
      }
      // the step's LDS reads together, branch-free (as the forward)
      const unsigned nx = tipl[max(t.xt, 0) + (col >> 1)], ny = tipl[max(t.yt, 0) + (col >> 1)];
      const double dv = deep[t.vdo + lane];
      const double2* Mc = reinterpret_cast<const double2*>(mbytes + t.mvb + st * 32);
      double2 c01 = Mc[0], c23 = Mc[1];
      asm volatile("" : "+v"(c01.x), "+v"(c01.y), "+v"(c23.x), "+v"(c23.y));  // (as the forward)
      const unsigned bx = t.xt >= 0 ? ln.nib(nx) : 0u;
      const unsigned by = t.yt >= 0 ? ln.nib(ny) : 0u;
      const double tx = ln.recv(t.mxb, bx), ty = ln.recv(t.myb, by);
      const double rv = (t.fl & F_VDEEP) ? dv : topr;
      double axr = t.xt >= 0 ? tx : lx, ayr = t.yt >= 0 ? ty : ly;
      asm volatile("" : "+v"(axr), "+v"(ayr) :: "memory");  // after the step's LDS waits:
      if (s > 1) tnn = ld_qstep_raw(prog, s - 2);               // the record two steps ahead
      // P^T r formed on every step and selected (as the forward)
      const auto [rx, ry] = ln.reverse(t.fl, t.xt, t.yt, t.mxg, t.myg, t.mvg, rv, axr, ayr, c01, c23, bx, by);
      if (t.xt < 0 && t.yt < 0) {  // r_x waits on the deep stack while y's subtree runs
        deep[t.xdo + lane] = rx;
        topr = ry;
      } else if (t.yt < 0) {
        topr = ry;
      } else if (t.xt < 0) {
        topr = rx;
      }
    }
    gfirst = false;
  }
  // per-wave scalar partials: [ll, dps, dfreq0..3]
  const double f0 = wave_sum(st == 0 ? acc_f : 0.0), f1 = wave_sum(st == 1 ? acc_f : 0.0);
  const double f2 = wave_sum(st == 2 ? acc_f : 0.0), f3 = wave_sum(st == 3 ? acc_f : 0.0);
  acc_ll = wave_sum(acc_ll);
  acc_dps = wave_sum(acc_dps);
  if (lane == 0) {
    double* ss = a.sslot + ((size_t)wg * C + c) * 8;
    ss[0] = acc_ll;
    ss[1] = acc_dps;
    ss[2] = f0;
    ss[3] = f1;
    ss[4] = f2;
    ss[5] = f3;
  }
}

// ===========================================================================
// The multi-wave quad sweep (qmw_kernel): W waves per category share one
// 16-column block.  The quad sweep's chain is the whole post-order program
// (fluA: 68 steps forward, 68 back, ~0.5 us each on one wave); independent
// subtrees need not wait for each other, so a host list-scheduler splits the
// steps over W waves (HLFET: the ready step farthest from the root first,
// preferring the wave that produced one of its children -- its value then
// stays in a register).  A child produced elsewhere (another wave, or this
// wave earlier) travels through an LDS slot whose flag the producer raises
// after the value (workgroup-scope release; the consumer polls with acquire
// loads, bounded).  The reverse runs each wave's list backwards: every r
// that the forward passed in a register passes in one again, every slot
// hand-off is mirrored.  Each step's arithmetic is qsweep_kernel's and every
// dL/dP entry is written by the one wave owning its step, so the rows are
// bitwise the single-wave sweep's.  fluA: level widths 20 12 6 4 2, then 23
// single-node levels: 68 -> ~36 step times per direction with W = 4.
// ===========================================================================
struct QmwArgs {
  QuadArgs q;
  const int* mprog;  // [W][maxst][QMW_INTS]
  int W, maxst, nslot, root_wave;
  int nst0, nst1, nst2, nst3;  // steps per wave
};
constexpr int QMW_SPIN_MAX = 1 << 22;  // polls before a hand-off counts as lost (the rows turn NaN)

__global__ void __launch_bounds__(1024) qmw_kernel(QmwArgs ma) {
  const QuadArgs& qa = ma.q;
  const SweepArgs& a = qa.s;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int lane = threadIdx.x & (WAVE - 1);
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  // wave wv = w C + c: the C waves of one schedule position w are consecutive, so each SIMD
  // (wave index mod 4) holds a different category's waves -- the critical waves (one per
  // category) do not share a SIMD
  const int W = ma.W, w = wv / a.C, c = wv - w * a.C;
  const int C = a.C, nmat = a.nmat, nslot = ma.nslot;
  const int col = lane >> 2, st = lane & 3;
  const int draw = blockIdx.y;
  const int wg = blockIdx.y * gridDim.x + blockIdx.x;
  const int rec = a.R * 4;
  const QuadLds lds(a.S, C, nmat, a.R, nslot, true);
  double* mats0 = reinterpret_cast<double*>(lds_raw);
  double* tvec = mats0 + lds.recs;
  double* xch = tvec + lds.tvec;
  double* slots = xch + lds.xch + (size_t)c * nslot * WAVE;
  int* flags0 = reinterpret_cast<int*>(xch + lds.xch + lds.tail);
  int* flags = flags0 + (size_t)c * nslot;
  int* errw = flags0 + (size_t)C * nslot;  // behind the flags, inside their padded block
  unsigned char* tipl = reinterpret_cast<unsigned char*>(flags0) + lds.flags;
  double* mats = mats0 + (size_t)c * nmat * rec;
  fill_tipvecs(tvec, a.extra);
  for (int k = threadIdx.x; k < C * nslot; k += blockDim.x) flags0[k] = -1;
  if (threadIdx.x == 0) *errw = 0;
  const int m0 = w * WAVE, mstride = W * WAVE;  // this wave's share of its category's records
  if (qa.build) {
    __shared__ double se[EIG_LEN];
    if (threadIdx.x < EIG_LEN) se[threadIdx.x] = a.eig[(size_t)draw * EIG_LEN + threadIdx.x];
    __syncthreads();
    qbuild_records(a, se, draw, c, mats, lane, m0, mstride);
    if (blockIdx.x == 0) {
      __syncthreads();
      const double2* src = reinterpret_cast<const double2*>(mats);
      double2* dst = reinterpret_cast<double2*>(qa.pmat_out + ((size_t)draw * C + c) * nmat * rec);
      for (int k = m0 + lane; k < nmat * rec / 2; k += mstride) dst[k] = src[k];
    }
  } else {
    const double2* src = reinterpret_cast<const double2*>(a.pmat + ((size_t)draw * C + c) * nmat * rec);
    double2* dst = reinterpret_cast<double2*>(mats);
    for (int k = m0 + lane; k < nmat * rec / 2; k += mstride) dst[k] = src[k];
  }
  const double* mdl = a.model + (size_t)draw * (10 + 2 * C);
  const V4 pi = {mdl[0], mdl[1], mdl[2], mdl[3]};
  const double pi_st = st == 0 ? pi.x : st == 1 ? pi.y : st == 2 ? pi.z : pi.w;
  const double ps_c = mdl[10 + C + c];
  double* scr = qa.qscr + (size_t)wg * a.nslots * C * WAVE + (size_t)c * WAVE + lane;
  double* gs = a.gslot + ((size_t)wg * C + c) * nmat * 16;
  bool gfirst = true;
  const bool gowner = (lane & 12) == 0;
  const int gent = st * 4 + ((lane >> 4) & 1) + 2 * ((lane >> 5) & 1);
  const int* myprog = ma.mprog + (size_t)w * ma.maxst * QMW_INTS;
  const int nst = w == 0 ? ma.nst0 : w == 1 ? ma.nst1 : w == 2 ? ma.nst2 : ma.nst3;
  const bool rootw = w == ma.root_wave;
  const unsigned char* mbytes = reinterpret_cast<const unsigned char*>(mats);
  double acc_ll = 0.0, acc_dps = 0.0, acc_f = 0.0;
  const QLane ln{.st = st, .col = col, .gfirst = gfirst, .mbytes = mbytes, .tvec = tvec, .gs = gs, .gowner = gowner,
                 .gent = gent, .c = c, .pi = pi, .pi_st = pi_st, .ps_c = ps_c};

  // slot hand-offs: the value, then (one lane) its flag, workgroup-scope release;
  // the consumer polls with acquire loads
  auto put = [&](int slot, int tag, double v) __attribute__((always_inline)) {
    slots[slot * WAVE + lane] = v;
    if (lane == 0) __hip_atomic_store(flags + slot, tag, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
  };
  auto await = [&](int slot, int tag) __attribute__((always_inline)) {
    int n = 0;
    while (__hip_atomic_load(flags + slot, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) != tag) {
      __builtin_amdgcn_s_sleep(1);
      if (++n > QMW_SPIN_MAX) {
        if (lane == 0) __hip_atomic_store(errw, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        break;
      }
    }
  };
  auto ldm = [&](int i) __attribute__((always_inline)) -> const int* { return myprog + (size_t)i * QMW_INTS; };

  int trip = 0;
  for (int blk = blockIdx.x; blk < qa.nblk; blk += gridDim.x, ++trip) {
    __syncthreads();
    stage_tip_nibbles(a, tipl, blk);
    __syncthreads();
    // ---- forward: this wave's steps
    double top = 0.0, proot = 0.0;
    for (int i = 0; i < nst; ++i) {
      const int* q = ldm(i);
      const int4 q0 = *reinterpret_cast<const int4*>(q), q1 = *reinterpret_cast<const int4*>(q + 4);
      const int4 q2 = *reinterpret_cast<const int4*>(q + 8), q4 = *reinterpret_cast<const int4*>(q + 16);
      const int xt = q0.x, yt = q0.y, mxb = q0.z, myb = q0.w, mvb = q1.x, vso = q1.y, fl = q1.z;
      const int xs = q2.y, ys = q2.z, vout = q2.w, sid = q4.x, xid = q4.y, yid = q4.z;
      const unsigned nx = tipl[max(xt, 0) + (col >> 1)], ny = tipl[max(yt, 0) + (col >> 1)];
      const double* M = reinterpret_cast<const double*>(mbytes + mvb) + st;
      const double mm0 = M[0], mm4 = M[4], mm8 = M[8], mm12 = M[12];
      const double tx = ln.recv(mxb, ln.nib(nx)), ty = ln.recv(myb, ln.nib(ny));
      double sx = 0.0, sy = 0.0;
      if (xs >= 0) {
        if (fl & QM_XW) await(xs, qmw_tag(trip, 0, xid));
        sx = slots[xs * WAVE + lane];
      }
      if (ys >= 0) {
        if (fl & QM_YW) await(ys, qmw_tag(trip, 0, yid));
        sy = slots[ys * WAVE + lane];
      }
      const double ax = xt >= 0 ? tx : (xs >= 0 ? sx : top);
      const double ay = yt >= 0 ? ty : (ys >= 0 ? sy : top);
      const double p = ax * ay;
      const double pv = QLane::pv(p, mm0, mm4, mm8, mm12);
      if (vso >= 0) {
        const double av = (fl & F_MV) ? pv : p;
        scr[vso] = av;
        if (vout >= 0) put(vout, qmw_tag(trip, 0, sid), av);
        top = av;
      } else {
        proot = p;
      }
    }
    // ---- root / site log L (the root's wave of each category)
    __syncthreads();  // (also: every wave's scratch stores before the reverse reads them)
    double fp = 0.0;
    if (rootw) fp = ln.root_put(proot, xch + c * QCOLS + col);
    __syncthreads();
    double topr = 0.0;
    if (rootw) topr = ln.site(a, xch + col, draw, blk, fp, proot, acc_ll, acc_dps, acc_f);
    // ---- reverse: this wave's steps backwards
    double lxn = 0.0, lyn = 0.0;  // the children's stored partials, a step ahead
    if (nst > 0) {
      const int* q = ldm(nst - 1);
      if (q[QM_XT] < 0) lxn = scr[q[QM_XSO]];
      if (q[QM_YT] < 0) lyn = scr[q[QM_YSO]];
    }
    for (int i = nst - 1; i >= 0; --i) {
      const int* q = ldm(i);
      const int4 q0 = *reinterpret_cast<const int4*>(q), q1 = *reinterpret_cast<const int4*>(q + 4);
      const int4 q2 = *reinterpret_cast<const int4*>(q + 8), q3 = *reinterpret_cast<const int4*>(q + 12);
      const int4 q4 = *reinterpret_cast<const int4*>(q + 16);
      const int xt = q0.x, yt = q0.y, mxb = q0.z, myb = q0.w, mvb = q1.x, fl = q1.z;
      const int xs = q2.y, ys = q2.z, vout = q2.w, mxg = q3.x, myg = q3.y, mvg = q3.z, nxso = q3.w;
      const int sid = q4.x, xid = q4.y, yid = q4.z, nyso = q4.w;
      const double lx = lxn, ly = lyn;
      lxn = nxso >= 0 ? scr[nxso] : 0.0;
      lyn = nyso >= 0 ? scr[nyso] : 0.0;
      const unsigned nx = tipl[max(xt, 0) + (col >> 1)], ny = tipl[max(yt, 0) + (col >> 1)];
      const double2* Mc = reinterpret_cast<const double2*>(mbytes + mvb + st * 32);
      const double2 c01 = Mc[0], c23 = Mc[1];
      const unsigned bx = xt >= 0 ? ln.nib(nx) : 0u;
      const unsigned by = yt >= 0 ? ln.nib(ny) : 0u;
      const double tx = ln.recv(mxb, bx), ty = ln.recv(myb, by);
      double rv = topr;
      if (vout >= 0) {
        if (fl & QM_RW) await(vout, qmw_tag(trip, 1, sid));
        rv = slots[vout * WAVE + lane];
      }
      const double ax = xt >= 0 ? tx : lx, ay = yt >= 0 ? ty : ly;
      const auto [rx, ry] = ln.reverse(fl, xt, yt, mxg, myg, mvg, rv, ax, ay, c01, c23, bx, by);
      if (xt < 0) {
        if (fl & QM_XTOP) topr = rx;
        else put(xs, qmw_tag(trip, 1, xid), rx);
      }
      if (yt < 0) {
        if (fl & QM_YTOP) topr = ry;
        else put(ys, qmw_tag(trip, 1, yid), ry);
      }
    }
    gfirst = false;
  }
  __syncthreads();  // every wave's hand-offs done: the error word is final
  if (!rootw) return;
  if (__hip_atomic_load(errw, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) acc_ll = NAN;  // a lost hand-off
  const double f0 = wave_sum(st == 0 ? acc_f : 0.0), f1 = wave_sum(st == 1 ? acc_f : 0.0);
  const double f2 = wave_sum(st == 2 ? acc_f : 0.0), f3 = wave_sum(st == 3 ? acc_f : 0.0);
  acc_ll = wave_sum(acc_ll);
  acc_dps = wave_sum(acc_dps);
  if (lane == 0) {
    double* ss = a.sslot + ((size_t)wg * C + c) * 8;
    ss[0] = acc_ll;
    ss[1] = acc_dps;
    ss[2] = f0;
    ss[3] = f1;
    ss[4] = f2;
    ss[5] = f3;
  }
}
