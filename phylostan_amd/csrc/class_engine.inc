// class_engine.inc -- the site-repeat ("class") sweep, included by
// phylo_hip.hip inside its second anonymous namespace (uses V4, reduce16,
// wave_sum, pvec/ptvec-style helpers, fail, HIP_TRY, dalloc).
//
// SURVEY.md 8a row a10: the reference's prototype skips a node when the tip
// states under it repeat those of an earlier column (pruner/tree.cpp:140-174,
// used at :201-226).  Here that idea is made exact and total:
//
//   * the *class* of (node v, pattern i) is the tuple of tip states under v
//     (host-built once per context: a class of v is a pair (class of x,
//     class of y) of its children's classes).  p_v and a_v = P_v p_v depend
//     on i only through it, so the forward pass runs once per class, not
//     once per pattern: fluA 3,743 non-root classes instead of 15,946
//     node-patterns, the synthetic 128 x 1M workload 1.16M instead of 66.5M;
//   * the reverse pass is linear in the upper partials, so it runs on
//     *aggregated* upper partials R_v[k] = sum of r_v,i over the patterns i
//     in class k:  G_v = sum_k R_v[k] (x) p_v[k],  Q_v[k] = P_v^T R_v[k],
//     R_x[k'] = sum over v's classes k whose x-part is k' of Q_v[k] * a_y[.].
//     The last sum is a segmented reduction: v's classes are ordered by the
//     class of one child (the *primary*: contiguous segments) and a
//     host-built permutation orders them for the other (*secondary*).
//     Segments can be very long (one class of a small clade may collect
//     55,000 of its parent's classes), so the reduction is a per-wave
//     segmented scan over 64-element tiles plus a fix-up of the segments
//     that cross tiles -- skew-proof and deterministic (fixed order).
//
// Everything is level-synchronous: level(v) = 1 + max(level of children);
// the forward runs levels 1..L-1 (one launch each), the root (level L) in
// one launch (a workgroup of C category waves per 64 root classes), then
// for L-1..1: RED (tiles of secondary children) + REV.  A segment that
// crosses at most SPAN_LANE_MAX tiles past its first is summed from its tile
// partials by the REV lane of its class, beside the child gathers (no
// launch); longer ones by a FIX launch (one wave each) before the level's
// REV.  One wave handles a
// chunk of up to 64 classes of ONE node (one class per lane: the big levels
// put tens of thousands of independent gathers in flight), so the node's
// matrix, children and flags are wave-uniform; its dL/dP contribution is ONE
// 16-entry wave reduction per chunk.
//
// Data per (draw, category) "dc", fp64, 32 B per class vector:
//   A[dc][slot]      moved partials a_v[k] (p_v[k] for the merged branch)
//   RR[dc][slot]     aggregated upper partials R_v[k]
//   STAGE[dc][pos]   per-child incoming contributions (parent's class order,
//                    permuted for the secondary child)
//   PART0/1[dc][tile] open-segment partial sums of the tiles
//   GPART[dc][gslot][16] per-chunk dL/dP partials (summed in order by the epilogue)

// waves per workgroup of the level-wide FWD / RED / FIX / REV launches (2:
// measured ~1 % over 4 on the synthetic workload, 8 slower; DESIGN.md 9)
constexpr int CLS_WPG = 2;
constexpr int CLS_THREADS = CLS_WPG * 64;
constexpr int SPAN_BATCH = 8;     // tile partials a REV lane has in flight while it sums a segment (SPAN_LANE_MAX)

struct ClassArgs {
  const CNode* nodes;
  const CChunkN* chunks;
  const int* cls;      // [slot][2]: child classes (x, y); tips: record index
  const int* secpos;   // [slot] staging position for the secondary child (sord = 0)
  const int* stperm;   // [nstage] staging position -> the STAGE entry its contribution was written to
  const CTile* tiles;
  const CSpan* spans;
  const double* pmat;  // [dc][nmat][R][4] matrix records
  const double* model; // [draw][10+2C]
  const double* wroot; // [nroot] pattern weight of each root class
  double* A;
  double* RR;
  double* STAGE;
  double* PART0;
  double* PART1;
  double* gpart;       // [dc][ngs][16]
  const int2* sspan;   // [slot] (t0, n): the class's segment crosses tiles t0..t0+n, summed by its REV lane (n = 0: no)
  double* sslot;       // [draw*nrootch + ch][C][8]
  double* sroot;       // [draw][nroot] w/L of each root class
  double* sitecls;     // [draw][nroot] log L of each root class
  int C, nmat, R, nslots, nstage, ntiles, ngs, nroot, nrootch, root, nspans;
  int rootr;           // rounds of ROOT_CHUNK classes per root workgroup (nrootch workgroups per draw)
  int first, count;    // this launch's chunk / tile range
  int rootoff;         // slot of the root's first class (its classes follow the other nodes')
  int sfirst;          // RED launches: the staging tile of the range's first tile (staging position 64 (sfirst + i))
  int sord;            // RED launches: the level's staging was written in parent class order (read through stperm)
  unsigned long long extra;
};

__device__ __forceinline__ V4 ldv(const double* p) {
  const double2 lo = *reinterpret_cast<const double2*>(p);
  const double2 hi = *reinterpret_cast<const double2*>(p + 2);
  return {lo.x, lo.y, hi.x, hi.y};
}
__device__ __forceinline__ void stv(double* p, const V4& v) {
  *reinterpret_cast<double2*>(p) = make_double2(v.x, v.y);
  *reinterpret_cast<double2*>(p + 2) = make_double2(v.z, v.w);
}
// P v and P^T v from a matrix record's four columns
__device__ __forceinline__ V4 rec_pv(const double* M, const V4& x) {
  const V4 a = ldv(M), b = ldv(M + 4), c = ldv(M + 8), d = ldv(M + 12);
  return {fma(d.x, x.w, fma(c.x, x.z, fma(b.x, x.y, a.x * x.x))),
          fma(d.y, x.w, fma(c.y, x.z, fma(b.y, x.y, a.y * x.x))),
          fma(d.z, x.w, fma(c.z, x.z, fma(b.z, x.y, a.z * x.x))),
          fma(d.w, x.w, fma(c.w, x.z, fma(b.w, x.y, a.w * x.x)))};
}
__device__ __forceinline__ V4 cols_pv(const V4& a, const V4& b, const V4& c, const V4& d, const V4& x) {
  return {fma(d.x, x.w, fma(c.x, x.z, fma(b.x, x.y, a.x * x.x))),
          fma(d.y, x.w, fma(c.y, x.z, fma(b.y, x.y, a.y * x.x))),
          fma(d.z, x.w, fma(c.z, x.z, fma(b.z, x.y, a.z * x.x))),
          fma(d.w, x.w, fma(c.w, x.z, fma(b.w, x.y, a.w * x.x)))};
}
// the identity in place of loaded columns (selects, not a branch: the loads
// stay ahead of their first use)
__device__ __forceinline__ void ident_if(bool id, V4& a, V4& b, V4& c, V4& d) {
  a = {id ? 1.0 : a.x, id ? 0.0 : a.y, id ? 0.0 : a.z, id ? 0.0 : a.w};
  b = {id ? 0.0 : b.x, id ? 1.0 : b.y, id ? 0.0 : b.z, id ? 0.0 : b.w};
  c = {id ? 0.0 : c.x, id ? 0.0 : c.y, id ? 1.0 : c.z, id ? 0.0 : c.w};
  d = {id ? 0.0 : d.x, id ? 0.0 : d.y, id ? 0.0 : d.z, id ? 1.0 : d.w};
}
__device__ __forceinline__ V4 cols_ptv(const V4& a, const V4& b, const V4& c, const V4& d, const V4& x) {
  return {vdot(a, x), vdot(b, x), vdot(c, x), vdot(d, x)};
}
__device__ __forceinline__ V4 rec_ptv(const double* M, const V4& x) {
  const V4 a = ldv(M), b = ldv(M + 4), c = ldv(M + 8), d = ldv(M + 12);
  return {vdot(a, x), vdot(b, x), vdot(c, x), vdot(d, x)};
}
// 16 outer-product accumulators, reduced over the wave once per chunk
struct G16 {
  double v[16];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int e = 0; e < 16; ++e) v[e] = 0.0;
  }
  __device__ __forceinline__ void add(const V4& r, const V4& p) {
    const double rr[4] = {r.x, r.y, r.z, r.w}, pp[4] = {p.x, p.y, p.z, p.w};
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int k = 0; k < 4; ++k) v[i * 4 + k] = fma(rr[i], pp[k], v[i * 4 + k]);
  }
  // wave sum of entry e -> GPART row (lanes with (lane & 3) == 0 own an entry)
  __device__ __forceinline__ void flush(double* row, int lane) {
    const double s = reduce16(v, lane);
    if ((lane & 3) == 0) row[reduce16_entry(lane)] = s;
  }
};

__device__ __forceinline__ size_t dcoff(int dc, int n) { return (size_t)dc * n; }

// ---- the class arrays one evaluation writes and reads (A, RR, STAGE, PART0,
// PART1): plain loads and stores -- the kernel boundaries order them.
// slot / position k of one dc's array
#define CLS_LD(arr, n, k) ldv(a.arr + (dcoff(dc, a.n) + (k)) * 4)
#define CLS_ST(arr, n, k, v) stv(a.arr + (dcoff(dc, a.n) + (k)) * 4, v)

// a child's moved partial of class k: a tip's record vector or A
// (level launches: one load from a wave-uniform base -- no branch for the
// compiler to sink the class load into)
__device__ __forceinline__ V4 child_a(const ClassArgs& a, int dc, int off, int m, int k) {
  const uint64_t pt = reinterpret_cast<uint64_t>(a.pmat + (dcoff(dc, a.nmat) + max(m, 0)) * a.R * 4);
  const uint64_t pa = reinterpret_cast<uint64_t>(a.A + (dcoff(dc, a.nslots) + max(off, 0)) * 4);
  return ldv(reinterpret_cast<const double*>(off < 0 ? pt : pa) + (size_t)k * 4);
}

// ---- forward: one wave per chunk ------------------------------------------
// Slots are chunk-major (every node's classes padded to a multiple of 64, in
// chunk order: build_class_engine checks it), so lane l of chunk ci owns slot
// 64 ci + l -- its per-slot loads issue with the chunk record's scalar load,
// not behind it (one dependent round trip fewer per level launch).
__device__ __forceinline__ void fwd_chunk(const ClassArgs& a, int dc, int ci, int lane) {
  const int sl = ci * WAVE + lane;
  const int2 kk = reinterpret_cast<const int2*>(a.cls)[sl];  // (padding slots: classes 0, 0)
  const CChunkN cc = a.chunks[ci];
  const CNode& nd = cc.nd;
  // v's matrix columns, loaded unconditionally (record 0 stands in for the
  // identity branch) so they issue with the child gathers, not after them
  const double* Mv = a.pmat + (dcoff(dc, a.nmat) + max(nd.mv, 0)) * a.R * 4;
  V4 m0 = ldv(Mv), m1 = ldv(Mv + 4), m2 = ldv(Mv + 8), m3 = ldv(Mv + 12);
  ident_if(nd.mv < 0, m0, m1, m2, m3);
  // every lane gathers, computes and stores: a padding lane (past the node's
  // classes) reads classes 0, 0 and writes its own padding slot, which nothing
  // reads -- no lane branch for the compiler to hoist ahead of the loads
  const V4 p = vmul(child_a(a, dc, nd.offx, nd.mx, kk.x), child_a(a, dc, nd.offy, nd.my, kk.y));
  const V4 av = cols_pv(m0, m1, m2, m3, p);  // (the identity's product is p, bit for bit: p >= 0, finite)
  CLS_ST(A, nslots, sl, av);
}
// one level, one wave per chunk
__global__ void __launch_bounds__(CLS_THREADS) cls_fwd_kernel(ClassArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  // (no early exit -- its kernel-argument wait would come first: the grid's
  // spare wave repeats the last chunk, storing the same bits)
  const int ck = min((int)blockIdx.x * CLS_WPG + wave, a.count - 1);
  fwd_chunk(a, blockIdx.y, a.first + ck, lane);
}

// Two forward levels in one launch (level pairs, build_class_engine): the
// lower level's chunks run as in cls_fwd_kernel; an upper-level chunk
// recomputes each lower-level child's moved partial from its grandchildren
// (their classes per upper class from a host table, gc) instead of reading
// the A its sibling chunks are still writing -- the lower level's arithmetic
// exactly, so the values are bitwise the two-launch ones.
__device__ __forceinline__ V4 fwd_node_value(const ClassArgs& a, int dc, const CNode& n, int kx, int ky) {
  const V4 p = vmul(child_a(a, dc, n.offx, n.mx, kx), child_a(a, dc, n.offy, n.my, ky));
  const double* M = a.pmat + (dcoff(dc, a.nmat) + max(n.mv, 0)) * a.R * 4;
  V4 m0 = ldv(M), m1 = ldv(M + 4), m2 = ldv(M + 8), m3 = ldv(M + 12);
  ident_if(n.mv < 0, m0, m1, m2, m3);
  return cols_pv(m0, m1, m2, m3, p);
}
__global__ void __launch_bounds__(CLS_THREADS) cls_fwd2_kernel(ClassArgs a, const int2* __restrict__ pair,
                                                               const int4* __restrict__ gc) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ck = min((int)blockIdx.x * CLS_WPG + wave, a.count - 1);  // (spare wave: cls_fwd_kernel)
  const int ci = a.first + ck, dc = blockIdx.y;
  const int sl = ci * WAVE + lane;
  const int2 kk = reinterpret_cast<const int2*>(a.cls)[sl];
  const int4 g = gc[sl];  // grandchildren's classes (upper-level chunks with a recomputed child)
  const CChunkN cc = a.chunks[ci];
  const int2 pr = pair[ci];
  const CNode& nd = cc.nd;
  V4 ax, ay;
  if (pr.x >= 0) ax = fwd_node_value(a, dc, a.nodes[pr.x], g.x, g.y);  // (wave-uniform)
  else ax = child_a(a, dc, nd.offx, nd.mx, kk.x);
  if (pr.y >= 0) ay = fwd_node_value(a, dc, a.nodes[pr.y], g.z, g.w);
  else ay = child_a(a, dc, nd.offy, nd.my, kk.y);
  const double* Mv = a.pmat + (dcoff(dc, a.nmat) + max(nd.mv, 0)) * a.R * 4;
  V4 m0 = ldv(Mv), m1 = ldv(Mv + 4), m2 = ldv(Mv + 8), m3 = ldv(Mv + 12);
  ident_if(nd.mv < 0, m0, m1, m2, m3);
  stv(a.A + (dcoff(dc, a.nslots) + sl) * 4, cols_pv(m0, m1, m2, m3, vmul(ax, ay)));  // (padding lanes: own padding slot)
}

// A segment crossing tiles: R[k] = PART1[t0] + sum PART0[t0+1..t1]; lanes
// stride over the tiles (two loads in flight each), then a fixed-order wave
// sum (every lane gets it): deterministic.
__device__ __forceinline__ V4 span_sum(const ClassArgs& a, int dc, const CSpan& sp, int lane) {
  V4 s = {0.0, 0.0, 0.0, 0.0}, s2 = {0.0, 0.0, 0.0, 0.0};
  if (sp.t1 - sp.t0 <= SPAN_LANE_MAX) {  // a short span: lane 0, in tile order -- the REV lanes' sum, bit for bit
    if (lane == 0) {
      s = CLS_LD(PART1, ntiles, sp.t0);
      for (int t = sp.t0 + 1; t <= sp.t1; ++t) {
        const V4 u = CLS_LD(PART0, ntiles, t);
        s.x += u.x;
        s.y += u.y;
        s.z += u.z;
        s.w += u.w;
      }
    }
    return s;
  }
  if (lane == 0) s = CLS_LD(PART1, ntiles, sp.t0);
  for (int t = sp.t0 + 1 + lane; t <= sp.t1; t += 2 * WAVE) {
    const V4 u = CLS_LD(PART0, ntiles, t);
    const V4 u2 = t + WAVE <= sp.t1 ? CLS_LD(PART0, ntiles, t + WAVE) : V4(0.0, 0.0, 0.0, 0.0);
    s.x += u.x;
    s.y += u.y;
    s.z += u.z;
    s.w += u.w;
    s2.x += u2.x;
    s2.y += u2.y;
    s2.z += u2.z;
    s2.w += u2.w;
  }
  s.x = wave_sum(s.x + s2.x);
  s.y = wave_sum(s.y + s2.y);
  s.z = wave_sum(s.z + s2.z);
  s.w = wave_sum(s.w + s2.w);
  return s;
}

// ---- segmented sums of one 64-position reduction tile -----------------------
// v: this lane's contribution at staging position 64 t + lane of the tile's
// node (ignored past the staging length).  Segments wholly inside the tile go
// straight to RR; the open ones leave tile partials (PART0: the first
// segment, begun in an earlier tile; PART1: the last one, continuing) for the
// REV lane of their class or a FIX wave.  All 64 lanes must call it
// (cross-lane scan).
__device__ __forceinline__ void tile_reduce(const ClassArgs& a, int dc, int g, const CTile& tl, V4 v,
                                            int lane) {
  const int pos = tl.t * WAVE + lane;
  const bool live = pos < tl.m;
  if (!live) v = V4(0.0, 0.0, 0.0, 0.0);
  const unsigned long long hm = ((unsigned long long)tl.hi << 32) | tl.lo;
  bool f = ((hm >> lane) & 1ull) || lane == 0;
  // segmented inclusive scan (Hillis-Steele; (f_a, v_a) + (f_b, v_b) =
  // (f_a | f_b, f_b ? v_b : v_a + v_b)) -- a fixed order: deterministic
#pragma unroll
  for (int d = 1; d < WAVE; d <<= 1) {
    const double ux = __shfl_up(v.x, d, WAVE), uy = __shfl_up(v.y, d, WAVE);
    const double uz = __shfl_up(v.z, d, WAVE), uw = __shfl_up(v.w, d, WAVE);
    const int uf = __shfl_up((int)f, d, WAVE);
    if (lane >= d && !f) {
      v.x = ux + v.x;
      v.y = uy + v.y;
      v.z = uz + v.z;
      v.w = uw + v.w;
      f = uf != 0;
    }
  }
  if (!live) return;
  const bool next_head = lane == WAVE - 1 ? true : ((hm >> (lane + 1)) & 1ull) != 0;
  const bool last = next_head || pos == tl.m - 1;
  if (!last) return;
  const unsigned long long below = lane == WAVE - 1 ? ~0ull : ((2ull << lane) - 1ull);
  const int k = tl.kfirst + __popcll(hm & below & ~1ull);
  const bool open_start = (k == tl.kfirst) && (tl.flags & 1);
  const bool continues = (lane == WAVE - 1) && (tl.flags & 2) && pos != tl.m - 1;
  if (!open_start && !continues)
    CLS_ST(RR, nslots, a.nodes[tl.node].off + k, v);
  else if (open_start)
    CLS_ST(PART0, ntiles, g, v);
  else
    CLS_ST(PART1, ntiles, g, v);
}

// ---- FIX: one wave per long tile-crossing segment ---------------------------
__device__ __forceinline__ void fix_span(const ClassArgs& a, int dc, int si, int lane) {
  const CSpan sp = a.spans[si];
  const V4 s = span_sum(a, dc, sp, lane);
  if (lane == 0) CLS_ST(RR, nslots, a.nodes[sp.node].off + sp.k, s);
}

// A parent class's contributions to its internal children: the primary
// child's reduction tile (scanned right here, in registers: no staging round
// trip), the secondary child's staging entry (its tiles are reduced by
// cls_red_kernel).  All lanes call it.
// Staging order.  A secondary child's staging is reduced in ITS class order
// (RED tiles); the writer is the parent, whose classes run in the primary
// child's order.  Small levels (and the clade levels) write each class's
// contribution straight to its reduction position (a.secpos: a random 32-B
// store) so the RED wave reads one contiguous run.  The levels with the most
// staged classes (nd.sord, ClassLevel::sord) write in the parent's class
// order instead -- entry stx + j for parent class j, a wave's 64 classes one
// contiguous 2 KB run -- and the RED wave gathers through a.stperm: the
// random access becomes a 32-B read instead of a partial-line write, at the
// price of one dependent index load in RED (which the small levels' latency
// chains cannot afford: shard of 8, 5,196 against 5,330 evals/s with every
// level so; one GPU 1,967 against 1,910).  Same values, same reduction
// order: the same bits either way.
__device__ __forceinline__ void contribute_inner(const ClassArgs& a, int dc, const CNode& nd, int sp,
                                                 bool live, const V4& cx, const V4& cy, int ptile, const CTile& ptl,
                                                 int lane) {
  // sp: the class's staging entry for its secondary child (its reduction position, or its index j when nd.sord)
  if (nd.offx >= 0 && !nd.secy) {  // x secondary
    if (live) CLS_ST(STAGE, nstage, nd.stx + sp, cx);
  }
  if (nd.offy >= 0 && nd.secy) {  // y secondary
    if (live) CLS_ST(STAGE, nstage, nd.sty + sp, cy);
  }
  if (ptile >= 0) tile_reduce(a, dc, ptile, ptl, nd.secy ? cx : cy, lane);  // primary internal child
}
// ... and to its tip children: their dL/dP accumulators
__device__ __forceinline__ void contribute_tips(const ClassArgs& a, const CNode& nd, int2 kk, const V4& cx,
                                                const V4& cy, G16& gx, G16& gy) {
  if (nd.offx < 0) gx.add(cx, tipvec_b((unsigned)kk.x, a.extra));
  if (nd.offy < 0) gy.add(cy, tipvec_b((unsigned)kk.y, a.extra));
}
// one outer product reduced over the wave into a dL/dP partial row at once
// (the REV waves' form: a chunk is one class per lane, so each accumulator
// takes one product; flushing it right away keeps one 16-entry set live
// instead of three)
__device__ __forceinline__ void outer_flush(double* row, const V4& r, const V4& p, int lane) {
  G16 g;
  g.zero();
  g.add(r, p);
  g.flush(row, lane);
}

// ---- RED: the staging tiles of secondary children --------------------------
// (staging is tile-major too: a secondary child's staging is padded to a
// multiple of 64 and laid out in RED-tile order, so a level launch knows the
// tile's staging position without its record: sb >= 0; else tl.sb)
__device__ __forceinline__ void red_tile(const ClassArgs& a, int dc, int g, int lane, int sb = -1) {
  V4 v = {0.0, 0.0, 0.0, 0.0};
  // (a.sord: position sb + lane holds the contribution written at entry
  // stperm[.]; padding positions: a valid entry, masked by tile_reduce)
  if (sb >= 0) v = CLS_LD(STAGE, nstage, a.sord ? a.stperm[sb + lane] : sb + lane);
  const CTile tl = a.tiles[g];
  if (sb < 0) v = CLS_LD(STAGE, nstage, tl.sb + lane);  // (clade levels: never sord)
  tile_reduce(a, dc, g, tl, v, lane);
}
// one level's tiles
__global__ void __launch_bounds__(CLS_THREADS) cls_red_kernel(ClassArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tk = min((int)blockIdx.x * CLS_WPG + wave, a.count - 1);  // (spare wave: cls_fwd_kernel)
  red_tile(a, blockIdx.y, a.first + tk, lane, (a.sfirst + tk) * WAVE);
}

// ---- the top chain's records (cls_chain_* below; the root recomputes the chain top; CLink: class_plan.h)
struct ChainArgs {
  const CLink* link;  // [m]
  const int* tab;     // [5][m][ntp]: class of c_i, of its x child, of its y child, staging position of x, of y
  const int* rep;     // [ntp]: bit i set: this top class is the representative of its class of c_i
  int m, ntop, ntp, toff;  // chain length, top classes (padded to ntp), the top's slot offset
};
#define CHT(w, i, kt) ch.tab[((size_t)(w) * ch.m + (i)) * ch.ntp + (kt)]

// the external child of chain node i (for i > 0 the one that is not c_{i-1};
// the bottom's y is gathered separately): its class row and its partial
template <int MC>
__device__ __forceinline__ void chain_gather(const ClassArgs& a, const ChainArgs& ch, int dc, int kt, V4 (&e)[MC],
                                             V4& ey0, int (&ke)[MC], int& ky0) {
  const int m = ch.m;
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int ii = min(i, m - 1);
    const CLink lk = ch.link[ii];
    const bool xe = lk.spine != 0;  // x is external (always at the bottom)
    ke[i] = CHT(xe ? 1 : 2, ii, kt);
    e[i] = child_a(a, dc, xe ? lk.offx : lk.offy, xe ? lk.mx : lk.my, ke[i]);
  }
  const CLink l0 = ch.link[0];
  ky0 = CHT(2, 0, kt);
  ey0 = child_a(a, dc, l0.offy, l0.my, ky0);
}
// a_i = P_i (a_{i-1} * e_i) from the bottom (a_0 = P_0 (e_0 * ey0)): the
// level launches' arithmetic (the product commutes exactly)
__device__ __forceinline__ V4 chain_step(const ClassArgs& a, int dc, const CLink& lk, const V4& u, const V4& w) {
  const V4 p = vmul(u, w);
  const double* Mv = a.pmat + (dcoff(dc, a.nmat) + max(lk.mv, 0)) * a.R * 4;
  V4 m0 = ldv(Mv), m1 = ldv(Mv + 4), m2 = ldv(Mv + 8), m3 = ldv(Mv + 12);
  ident_if(lk.mv < 0, m0, m1, m2, m3);
  return cols_pv(m0, m1, m2, m3, p);
}

// ---- root: one workgroup of C category waves per rootr x ROOT_CHUNK root
// classes.  Per round, wave c forms ps_c pi.p_c of its lane's class, the
// workgroup sums the categories through LDS in category order (L, log L,
// w / L), then each wave runs its category's reverse seeds R = (w/L) ps_c pi
// (identity root branch: Q = R), the contributions to the root's children
// and the scalar partials; the workgroup's partials are flushed once.
// MAXT: the register budget (C = 4 launches 256 threads: 256 VGPRs, no spill).
// TIPS: a child of the root is a tip (else its 32 dL/dP accumulators, live
// across the rounds, are compiled out: 191 -> fewer VGPRs at C = 4).
// (root_chunk: one root workgroup's work; every wave of the workgroup calls
// it -- it holds barriers)
// MC > 0 (level launches with a top chain of m <= MC levels, C <= 4): the
// root's child that is the chain's top is recomputed here from the chain's
// tables (chain_gather / chain_step: the chain forward's arithmetic, so the
// same bits as the A that cls_chain_fwd_kernel would store) -- and nothing
// else reads the chain's A, so that launch is dropped
template <bool TIPS, int MC = 0>
__device__ __forceinline__ void root_chunk(const ClassArgs& a, int ch, int draw,
                                           double (&fcat)[2][16][WAVE], const ChainArgs* cha = nullptr) {
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int C = a.C, dc = draw * C + c;
  const CNode nd = a.nodes[a.root];
  const double* mdl = a.model + (size_t)draw * (10 + 2 * C);
  const V4 pi = {mdl[0], mdl[1], mdl[2], mdl[3]};
  const double ps = mdl[10 + C + c];
  G16 gx, gy;
  gx.zero();
  gy.zero();
  double acc_ll = 0.0, acc_dps = 0.0;
  V4 acc_f = {0.0, 0.0, 0.0, 0.0};
  for (int r = 0; r < a.rootr; ++r) {
    const int ci = ch * a.rootr + r;  // 64-class chunk: its reduction tile of the primary child
    const int j0 = ci * ROOT_CHUNK, j = j0 + lane;
    if (j0 >= a.nroot) break;  // workgroup-uniform (nroot = nd.n: known without the node record)
    const bool live = j < a.nroot;
    const int jj = live ? j : j0;
    const int2 kk = reinterpret_cast<const int2*>(a.cls)[a.rootoff + jj];
    const int spj = nd.sord ? jj : a.secpos[a.rootoff + jj];
    const int ptile = nd.ptile >= 0 ? nd.ptile + ci : -1;
    const CTile ptl = a.tiles[max(ptile, 0)];  // (loaded ahead of its use, unconditionally)
    V4 ax, ay;
    if constexpr (MC > 0) {
      const ChainArgs& cg = *cha;
      const bool topx = nd.offx == cg.toff;  // (uniform) which root child is the chain's top
      const int kt = topx ? kk.x : kk.y;
      V4 e[MC], ey0;
      int ke[MC], ky0;
      chain_gather<MC>(a, cg, dc, kt, e, ey0, ke, ky0);
      const V4 ao = topx ? child_a(a, dc, nd.offy, nd.my, kk.y) : child_a(a, dc, nd.offx, nd.mx, kk.x);
      V4 av = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int i = 0; i < MC; ++i) {
        if (i >= cg.m) break;  // uniform
        av = chain_step(a, dc, cg.link[i], i == 0 ? ey0 : av, e[i]);
      }
      ax = topx ? av : ao;
      ay = topx ? ao : av;
    } else {
      ax = child_a(a, dc, nd.offx, nd.mx, kk.x);
      ay = child_a(a, dc, nd.offy, nd.my, kk.y);
    }
    const V4 p = vmul(ax, ay);
    const double fp = vdot(pi, p);
    fcat[r & 1][c][lane] = ps * fp;
    __syncthreads();
    double L = 0.0;
    for (int q = 0; q < C; ++q) L += fcat[r & 1][q][lane];
    const double w = live ? a.wroot[j] : 0.0;
    const double s = live ? w / L : 0.0;
    if (c == 0 && live) {
      const double lnL = log(L);
      a.sitecls[(size_t)draw * a.nroot + j] = lnL;
      acc_ll = fma(w, lnL, acc_ll);
    }
    const double sc = s * ps;
    acc_dps = fma(s, fp, acc_dps);
    acc_f.x = fma(sc, p.x, acc_f.x);
    acc_f.y = fma(sc, p.y, acc_f.y);
    acc_f.z = fma(sc, p.z, acc_f.z);
    acc_f.w = fma(sc, p.w, acc_f.w);
    const V4 R = vscale(pi, sc);
    const V4 cx = vmul(R, ay), cy = vmul(R, ax);
    if constexpr (TIPS) contribute_tips(a, nd, kk, cx, cy, gx, gy);
    contribute_inner(a, dc, nd, spj, live, cx, cy, ptile, ptl, lane);
  }
  if constexpr (TIPS) {
    if (nd.gx >= 0) gx.flush(a.gpart + (dcoff(dc, a.ngs) + nd.gx + ch) * 16, lane);
    if (nd.gy >= 0) gy.flush(a.gpart + (dcoff(dc, a.ngs) + nd.gy + ch) * 16, lane);
  }
  acc_ll = wave_sum(acc_ll);
  acc_dps = wave_sum(acc_dps);
  acc_f.x = wave_sum(acc_f.x);
  acc_f.y = wave_sum(acc_f.y);
  acc_f.z = wave_sum(acc_f.z);
  acc_f.w = wave_sum(acc_f.w);
  if (lane == 0) {
    double* ss = a.sslot + (((size_t)draw * a.nrootch + ch) * C + c) * 8;
    ss[0] = acc_ll;  // 0 for c > 0
    ss[1] = acc_dps;
    ss[2] = acc_f.x;
    ss[3] = acc_f.y;
    ss[4] = acc_f.z;
    ss[5] = acc_f.w;
  }
}
template <int MAXT, bool TIPS, int MC = 0>
__global__ void __launch_bounds__(MAXT) cls_root_kernel(ClassArgs a, ChainArgs cha) {
  __shared__ double fcat[2][16][WAVE];  // C <= 16 (phy_create); double-buffered over rounds
  root_chunk<TIPS, MC>(a, blockIdx.x, blockIdx.y, fcat, &cha);
}

// ---- REV: one wave per chunk ----------------------------------------------
// LS (level launches, build_class_engine's PHY_REVFIX plan): the chunk's
// long segments (beyond SPAN_LANE_MAX tiles) are summed here by the whole
// wave, fix_span's arithmetic (so R is bitwise the FIX launch's RR), instead
// of by a FIX launch before the level's REV: clf[ci] = (first, count) into
// clong (span indices).
template <bool LS = false>
__device__ __forceinline__ void rev_chunk(const ClassArgs& a, int dc, int ci, int lane,
                                          const int2* clf = nullptr, const int* clong = nullptr) {
  const int sl = ci * WAVE + lane;  // this lane's slot (chunk-major, fwd_chunk): loaded beside the chunk record
  const int2 kk0 = reinterpret_cast<const int2*>(a.cls)[sl];
  int2 lf = make_int2(0, 0);
  if constexpr (LS) lf = clf[ci];
  const V4 R0 = CLS_LD(RR, nslots, sl);
  const int2 ls0 = a.sspan[sl];
  const int sp0 = a.secpos[sl];
  const CChunkN cc = a.chunks[ci];
  const CNode& nd = cc.nd;
  const int jn = cc.jn, chi = cc.ci;
  const bool hasm = nd.mv >= 0;  // (else the identity: root / merged branch)
  const double* Mv = a.pmat + (dcoff(dc, a.nmat) + max(nd.mv, 0)) * a.R * 4;  // loaded up front (fwd_chunk)
  const V4 m0 = ldv(Mv), m1 = ldv(Mv + 4), m2 = ldv(Mv + 8), m3 = ldv(Mv + 12);
  const bool live = lane < jn;
  // a padding lane reads classes (0, 0) (valid children's classes): with R = 0
  // every product it forms is zero and it stores nothing
  const int2 kk = kk0;
  // the child gathers and the primary child's tile record, issued before the
  // span sums (they need only the classes and the chunk record)
  const V4 ax = child_a(a, dc, nd.offx, nd.mx, kk.x), ay = child_a(a, dc, nd.offy, nd.my, kk.y);
  const int ptile = nd.ptile >= 0 ? nd.ptile + chi : -1;
  const CTile ptl = a.tiles[max(ptile, 0)];
  V4 R = live ? R0 : V4(0.0, 0.0, 0.0, 0.0);
  const int2 ls = live ? ls0 : make_int2(0, 0);
  if (live && ls.y > 0) {  // R = PART1[t0] + PART0[t0+1] + ... + PART0[t0+n], in tile order
    V4 u[SPAN_BATCH];
#pragma unroll
    for (int q = 0; q < SPAN_BATCH; ++q) u[q] = q < ls.y ? CLS_LD(PART0, ntiles, ls.x + q + 1) : V4(0.0, 0.0, 0.0, 0.0);
    R = CLS_LD(PART1, ntiles, ls.x);
    for (int q0 = 0;; q0 += SPAN_BATCH) {  // batches in tile order (the sum stays sequential)
      if constexpr (SPAN_LANE_MAX <= SPAN_BATCH) {  // one batch: no loop (registers)
#pragma unroll
        for (int q = 0; q < SPAN_BATCH; ++q)
          if (q < ls.y) {
            R.x += u[q].x;
            R.y += u[q].y;
            R.z += u[q].z;
            R.w += u[q].w;
          }
        break;
      }
#pragma unroll
      for (int q = 0; q < SPAN_BATCH; ++q)
        if (q0 + q < ls.y) {
          R.x += u[q].x;
          R.y += u[q].y;
          R.z += u[q].z;
          R.w += u[q].w;
        }
      if (q0 + SPAN_BATCH >= ls.y) break;
#pragma unroll
      for (int q = 0; q < SPAN_BATCH; ++q)
        u[q] = q0 + SPAN_BATCH + q < ls.y ? CLS_LD(PART0, ntiles, ls.x + q0 + SPAN_BATCH + q + 1)
                                          : V4(0.0, 0.0, 0.0, 0.0);
    }
  }
  if constexpr (LS) {
    for (int i = 0; i < lf.y; ++i) {  // (wave-uniform; rare)
      const CSpan sp = a.spans[clong[lf.x + i]];
      const V4 s = span_sum(a, dc, sp, lane);  // every lane gets the sum
      if (lane == sp.k - cc.j0) R = s;
    }
  }
  const V4 zero = {0.0, 0.0, 0.0, 0.0};  // a slot without a product gets zeros, as before
  if (nd.gv >= 0) outer_flush(a.gpart + (dcoff(dc, a.ngs) + nd.gv + chi) * 16, hasm ? R : zero, vmul(ax, ay), lane);
  const V4 Q = hasm ? cols_ptv(m0, m1, m2, m3, R) : R;
  const V4 cx = vmul(Q, ay), cy = vmul(Q, ax);
  if (nd.gx >= 0)
    outer_flush(a.gpart + (dcoff(dc, a.ngs) + nd.gx + chi) * 16, nd.offx < 0 ? cx : zero,
                tipvec_b((unsigned)kk.x, a.extra), lane);
  if (nd.gy >= 0)
    outer_flush(a.gpart + (dcoff(dc, a.ngs) + nd.gy + chi) * 16, nd.offy < 0 ? cy : zero,
                tipvec_b((unsigned)kk.y, a.extra), lane);
  contribute_inner(a, dc, nd, nd.sord ? cc.j0 + lane : sp0, live, cx, cy, ptile, ptl, lane);
}
// one level, one wave per chunk
__global__ void __launch_bounds__(CLS_THREADS) cls_rev_kernel(ClassArgs a) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ck = min((int)blockIdx.x * CLS_WPG + wave, a.count - 1);  // (spare wave: cls_fwd_kernel)
  rev_chunk(a, blockIdx.y, a.first + ck, lane);
}
// ... whose chunks also sum their long segments (no FIX launch for the level)
__global__ void __launch_bounds__(CLS_THREADS) cls_rev_ls_kernel(ClassArgs a, const int2* __restrict__ clf,
                                                                 const int* __restrict__ clong) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int ck = min((int)blockIdx.x * CLS_WPG + wave, a.count - 1);
  rev_chunk<true>(a, blockIdx.y, a.first + ck, lane, clf, clong);
}

// ---- the top chain: single-node levels fused --------------------------------
// Near the root of a caterpillar-like tree every level L-1, L-2, ..., lo holds
// ONE node (the synthetic 128-taxon tree: levels 12..16): each level-wide
// launch there is a few waves and pure latency.  The chain c_0 (level lo) ..
// c_{m-1} (level L-1, the "top") runs in one launch per pass, one lane per
// class kt of the top:
//   forward  a_0 = P_0 (a_x0 * a_y0), a_i = P_i (a_{i-1} * e_i): the classes
//            of every chain node and child under kt come from host tables, so
//            all m + 1 child gathers issue at once; a_i is stored by the one
//            top class chosen as its class's representative -- bitwise the
//            level launches' values;
//   reverse  the reverse is linear, so top class kt carries its own share
//            down the chain: c_{m-1} = R_top[kt]; dL/dP_i += c_i (x) p_i;
//            q = P_i^T c_i; the external children's shares q * a_spine (or
//            q * e_i) go to their staging at their position in kt order
//            (segmented sums by the level's RED as for any staged child), and
//            c_{i-1} = q * e_i continues down.  R of the chain nodes below
//            the top is never formed: their dL/dP sums run over top classes.

template <int MC>
__global__ void __launch_bounds__(CLS_THREADS) cls_chain_fwd_kernel(ClassArgs a, ChainArgs ch) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tc = min((int)blockIdx.x * CLS_WPG + wave, (ch.ntop + WAVE - 1) / WAVE - 1);
  const int dc = blockIdx.y, kt = tc * WAVE + lane, m = ch.m;
  // every class index, then every gather (padding top classes read valid zeros)
  int kc[MC], ke[MC], ky0;
#pragma unroll
  for (int i = 0; i < MC; ++i) kc[i] = CHT(0, min(i, m - 1), kt);
  const int rp = ch.rep[kt];
  V4 e[MC], ey0;
  chain_gather<MC>(a, ch, dc, kt, e, ey0, ke, ky0);
  V4 av = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    if (i >= m) break;  // uniform
    const CLink lk = ch.link[i];
    av = chain_step(a, dc, lk, i == 0 ? ey0 : av, e[i]);
    if (((rp >> i) & 1) && kt < ch.ntop) stv(a.A + (dcoff(dc, a.nslots) + lk.off + kc[i]) * 4, av);
  }
}

template <int MC>
__global__ void __launch_bounds__(CLS_THREADS) cls_chain_rev_kernel(ClassArgs a, ChainArgs ch) {
  // the chain's recomputed forward values wait in LDS (wave-private), not in
  // registers: 4 waves per SIMD instead of 2 at m = 5
  __shared__ double acs[CLS_WPG * MC * 4 * WAVE];
  // the chain's matrix columns for this workgroup's dc (both waves share it),
  // staged once: the forward recompute and the reverse read them from LDS
  // instead of one dependent global round trip per level
  __shared__ __attribute__((aligned(16))) double cms[MC * 16];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int tc = min((int)blockIdx.x * CLS_WPG + wave, (ch.ntop + WAVE - 1) / WAVE - 1);
  const int dc = blockIdx.y, kt = tc * WAVE + lane, m = ch.m;
  if (threadIdx.x < MC * 16) {
    const int li = min((int)threadIdx.x >> 4, m - 1);
    const int mv = ch.link[li].mv;
    const double v = a.pmat[(dcoff(dc, a.nmat) + max(mv, 0)) * a.R * 4 + (threadIdx.x & 15)];
    const int r = (threadIdx.x & 15) >> 2, cc = threadIdx.x & 3;  // column r, entry cc
    cms[threadIdx.x] = mv < 0 ? (r == cc ? 1.0 : 0.0) : v;        // (ident_if's identity)
  }
  const bool live = kt < ch.ntop;
  const int sl = ch.toff + kt;  // the top's slot (RR, lane-summed span)
  const V4 R0 = ldv(a.RR + (dcoff(dc, a.nslots) + sl) * 4);
  const int2 ls = live ? a.sspan[sl] : make_int2(0, 0);
  int ke[MC], pe[MC], ky0;
  V4 e[MC], ey0;
  chain_gather<MC>(a, ch, dc, kt, e, ey0, ke, ky0);
#pragma unroll
  for (int i = 0; i < MC; ++i) {
    const int ii = min(i, m - 1);
    pe[i] = CHT(ch.link[ii].spine != 0 ? 3 : 4, ii, kt);
  }
  const int py0 = CHT(4, 0, kt);
  // the chain's forward values again (bitwise the stored ones), a_0 .. a_{m-2} parked in LDS
  double* acw = acs + (size_t)wave * MC * 4 * WAVE + lane;
  __syncthreads();  // cms staged
  V4 av = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < MC - 1; ++i) {
    if (i >= m - 1) break;  // uniform
    {
      const double* Ms = cms + i * 16;
      av = cols_pv(ldv(Ms), ldv(Ms + 4), ldv(Ms + 8), ldv(Ms + 12), vmul(i == 0 ? ey0 : av, e[i]));
    }
    acw[(i * 4 + 0) * WAVE] = av.x;
    acw[(i * 4 + 1) * WAVE] = av.y;
    acw[(i * 4 + 2) * WAVE] = av.z;
    acw[(i * 4 + 3) * WAVE] = av.w;
  }
  V4 c = live ? R0 : V4(0.0, 0.0, 0.0, 0.0);
  if (live && ls.y > 0) {  // the top class's segment crossed tiles: R = PART1[t0] + PART0[t0+1..], in tile order
    c = ldv(a.PART1 + (dcoff(dc, a.ntiles) + ls.x) * 4);
    for (int q = 1; q <= ls.y; ++q) {
      const V4 u = ldv(a.PART0 + (dcoff(dc, a.ntiles) + ls.x + q) * 4);
      c.x += u.x;
      c.y += u.y;
      c.z += u.z;
      c.w += u.w;
    }
  }
#pragma unroll
  for (int j = MC - 1; j >= 0; --j) {
    if (j >= m) continue;  // uniform
    const CLink lk = ch.link[j];
    // children: (x, y) = (a_{j-1}, e_j) or (e_j, a_{j-1}); the bottom (e_0, ey0)
    const V4 sp = j > 0 ? V4(acw[((j - 1) * 4 + 0) * WAVE], acw[((j - 1) * 4 + 1) * WAVE], acw[((j - 1) * 4 + 2) * WAVE],
                             acw[((j - 1) * 4 + 3) * WAVE])
                        : ey0;
    const V4 ax = lk.spine == 0 ? sp : e[j], ay = lk.spine == 0 ? e[j] : sp;
    const double* Ms = cms + j * 16;
    const V4 m0 = ldv(Ms), m1 = ldv(Ms + 4), m2 = ldv(Ms + 8), m3 = ldv(Ms + 12);
    if (lk.gv >= 0) outer_flush(a.gpart + (dcoff(dc, a.ngs) + lk.gv + tc) * 16, c, vmul(ax, ay), lane);
    const V4 q = cols_ptv(m0, m1, m2, m3, c);
    const V4 cx = vmul(q, ay), cy = vmul(q, ax);
    const bool xe = lk.spine != 0, ye = lk.spine != 1;  // external children (both at the bottom)
    if (xe) {
      const int kx = ke[j];
      if (lk.offx < 0) {
        if (lk.gx >= 0) outer_flush(a.gpart + (dcoff(dc, a.ngs) + lk.gx + tc) * 16, cx, tipvec_b((unsigned)kx, a.extra), lane);
      } else if (live) {
        stv(a.STAGE + (dcoff(dc, a.nstage) + lk.stx + pe[j]) * 4, cx);
      }
    }
    if (ye) {
      const int ky = j == 0 ? ky0 : ke[j], py = j == 0 ? py0 : pe[j];
      if (lk.offy < 0) {
        if (lk.gy >= 0) outer_flush(a.gpart + (dcoff(dc, a.ngs) + lk.gy + tc) * 16, cy, tipvec_b((unsigned)ky, a.extra), lane);
      } else if (live) {
        stv(a.STAGE + (dcoff(dc, a.nstage) + lk.sty + py) * 4, cy);
      }
    }
    c = lk.spine == 0 ? cx : cy;  // the spine child's share (unused below the bottom)
  }
}
#undef CHT

// ---- bottom clades: the small levels fused ------------------------------
// A clade is a maximal subtree of the nodes at levels <= Lc (its root's
// parent sits higher).  Its nodes depend only on each other and on work the
// level-synchronous launches above finish first, so one workgroup per
// (clade, dc) runs all of its levels with a barrier between them (and
// between the reverse's RED / REV phases) instead of one launch per level
// and phase.  Same chunks, tiles and spans, same operations in the
// same order: results are bitwise those of the per-level launches.
constexpr int CLADE_THREADS = 512;
// The clade roots' own RED tiles are sized by their parents (levels above
// Lc: often large), so they run before the clade kernels as one flat launch
// over an index list, not inside one workgroup.
__global__ void __launch_bounds__(CLS_THREADS) cls_red_list_kernel(ClassArgs a, const int* list, int n) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int i = blockIdx.x * CLS_WPG + wave;
  if (i >= n) return;
  red_tile(a, blockIdx.y, list[i], lane);
}
__global__ void __launch_bounds__(CLS_THREADS) cls_fix_list_kernel(ClassArgs a, const int* list, int n) {
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int i = blockIdx.x * CLS_WPG + wave;
  if (i >= n) return;
  fix_span(a, blockIdx.y, list[i], lane);
}
__global__ void __launch_bounds__(CLADE_THREADS) cls_clade_fwd_kernel(ClassArgs a, const CladeLevel* cl, int Lc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int dc = blockIdx.y;
  for (int l = 0; l < Lc; ++l) {
    const CladeLevel c = cl[(size_t)blockIdx.x * Lc + l];
    for (int i = wave; i < c.nchunk; i += nw) fwd_chunk(a, dc, c.chunk0 + i, lane);
    __syncthreads();  // this level's A before the next level gathers it
  }
}
__global__ void __launch_bounds__(CLADE_THREADS) cls_clade_rev_kernel(ClassArgs a, const CladeLevel* cl, int Lc) {
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, nw = blockDim.x >> 6;
  const int dc = blockIdx.y;
  for (int l = Lc - 1; l >= 0; --l) {
    const CladeLevel c = cl[(size_t)blockIdx.x * Lc + l];
    for (int i = wave; i < c.ntile; i += nw) red_tile(a, dc, c.tile0 + i, lane);
    __syncthreads();  // tile partials before the spans
    for (int i = wave; i < c.nspan; i += nw) fix_span(a, dc, c.span0 + i, lane);
    __syncthreads();  // R complete before the reverse reads it
    for (int i = wave; i < c.nchunk; i += nw) rev_chunk(a, dc, c.chunk0 + i, lane);
    __syncthreads();  // contributions to the children before their level
  }
}

// ---- the epilogue: a per-item launch, then a closing launch per draw --------
// Per-item launch (cls_epi_kernel<EPI_WIDE_THREADS, 1>): workgroup
// (c*B + b, draw) sums the chunk partials of branch b, category c into its
// dL/dP row (EPI_WIDE_THREADS / 16 groups of 16 entries, 16 loads in flight,
// fixed order), forms <G_cb, Q P_cb> and its share of the Q-parameter chain
// rule's M = sum_cb (V^T G_cb V^-T) .* Phi_cb (the algebra of qgrad_body),
// and a slice of the root workgroups' scalar partials, and stores them.
// Closing launch (cls_epi_kernel<EPI_THREADS, 2>, one workgroup per draw):
// sums the C*B hand-offs in a fixed order -- log L, dlogL/dblens, /drs,
// /dps, the root frequency term, the exchangeability and frequency
// gradients.  Until round 6 both ran in ONE launch, the last workgroup to
// take a per-draw ticket closing it; a timestamped build (tools/epitime.py)
// showed its C*B 512-thread workgroups (170 VGPRs for the closing code) ran
// one per CU, in four dispatch rounds of ~4 us each.  Split, the per-item
// workgroups (256 threads, 81 VGPRs) are all resident at once: shard of 8
// 5,282 -> 5,578 evals/s, one GPU unchanged (profiles/r06_epi_split_ab.txt).
// A long branch's dL/dP partial rows (thousands on the one-GPU synthetic
// plan: one per 64-class chunk of a node of 10^5 classes) would make its
// epilogue workgroup a chain of a dozen dependent rounds of loads (one CU's
// loads in flight); they are summed first in sub-ranges of GSUB_ROWS rows,
// one workgroup each with every load in flight, then the epilogue sums the
// sub-range sums in order -- a fixed order: deterministic (GSUB_ROWS, GSUB_MIN: class_plan.h).
__global__ void __launch_bounds__(256) cls_gsum_kernel(const double* __restrict__ gpart, const int2* __restrict__ gsub,
                                                      double* __restrict__ gpsum, int ngs, int nsub) {
  __shared__ double part[16][17];
  const int j = blockIdx.x, dc = blockIdx.y, g = threadIdx.x >> 4, e = threadIdx.x & 15;
  const int2 sb = gsub[j];
  const double* src = gpart + ((size_t)dc * ngs + sb.x) * 16 + e;
  double u[GSUB_ROWS / 16];
#pragma unroll
  for (int v = 0; v < GSUB_ROWS / 16; ++v) {
    const int k = g + 16 * v;
    u[v] = k < sb.y ? src[(size_t)k * 16] : 0.0;
  }
#pragma unroll
  for (int w = GSUB_ROWS / 32; w >= 1; w >>= 1)  // a fixed pairwise tree
#pragma unroll
    for (int v = 0; v < w; ++v) u[v] = u[2 * v] + u[2 * v + 1];
  part[g][e] = u[0];
  __syncthreads();
  if (threadIdx.x < 16) {
    double t = part[0][threadIdx.x];
    for (int q = 1; q < 16; ++q) t += part[q][threadIdx.x];
    gpsum[((size_t)dc * nsub + j) * 16 + threadIdx.x] = t;
  }
}

struct EpiArgs {
  const double* gpart;  // [dc][ngs][16]
  const int* gbase;     // [B]
  const int* gcount;    // [B]
  const double* sslot;  // [draw][nrootch][C][8]
  const double* pmat;   // [draw][C][nmat][R][4] (columns of P first)
  const double* eig;    // [draw][EIG_LEN]
  const double* blens;  // [draw][B]
  const double* model;  // [draw][10+2C]
  const int* gpos;      // [B] matrix of branch b
  double* grows;        // dL/dP rows of draw d at grows + d * grows_stride
  long long grows_stride;
  double* out;          // [draw][outlen]
  double* inner;        // [draw][C*B]      hand-off: <G_cb, Q P_cb>
  double* mpart;        // [draw][C*B][16]  hand-off: (c, b)'s part of M
  double* spart;        // [draw][C*B][8C]  hand-off: scalar partial sums of a slice of root workgroups
  int C, B, nmat, R, ngs, nrootch, outlen, kind;
  const double* gpsum;  // [dc][nsub][16] sub-range sums of the long branches (cls_gsum_kernel)
  const int* pbase;     // [B] their first sub-range (-1: the branch's rows are summed here)
  int nsub;
};
constexpr int EPI_THREADS = 512;        // the closing launch's workgroup
constexpr int EPI_WIDE_THREADS = 256;   // the per-item launch's workgroups
constexpr int EPI_GROUPS = EPI_THREADS / 16;
constexpr int EPI_CMAX = 16;   // categories the closing workgroup's registers cover (phy_create: C <= 16)
constexpr int EPI_SLICES = 64;  // items that sum a slice of the root workgroups' scalar partials
static_assert(EPI_SLICES <= 2 * EPI_GROUPS, "the closing workgroup sums two slices per group");

#ifdef PHY_EPITIME
// Diagnostic build only (tools/epitime.py): the real-time clock (100 MHz) of
// wave 0 of each epilogue workgroup of draw 0 at its phase boundaries (the
// closing workgroup in the last row).
constexpr int ET_ITEMS = 4096, ET_EV = 8;
__device__ unsigned long long g_et[ET_ITEMS][ET_EV];
#define ET_MARK(i)                                                                         \
  do {                                                                                     \
    if (draw == 0 && item < ET_ITEMS - 1 && tid == 0)                                      \
      g_et[MODE == 2 ? ET_ITEMS - 1 : item][(i)] = __builtin_amdgcn_s_memrealtime();       \
  } while (0)
#else
#define ET_MARK(i) do {} while (0)
#endif
// MODE 1: the per-item launch (grid (C*B, draws)); MODE 2: the closing
// launch (grid (draws)), after it -- the kernel boundary orders the
// hand-offs.  NT threads.
template <int NT, int MODE>
__global__ void __launch_bounds__(NT) cls_epi_kernel(EpiArgs a) {
  constexpr int EPI_GROUPS_T = NT / 16;
  __shared__ double sV[16], sVi[16], sQ[16], srinv[16], slam[4];
  __shared__ double part[EPI_GROUPS_T][17];
  __shared__ double sG[16], sterm[16];
  __shared__ double red[EPI_GROUPS_T][129];  // the last workgroup's group partials (8C <= 128 entries)
  __shared__ double sroot[4], sM[16], sW[16];
  __shared__ double csum[8][16];
  const int tid = threadIdx.x, g = tid >> 4, e = tid & 15;
  const int item = MODE == 2 ? 0 : blockIdx.x, draw = MODE == 2 ? blockIdx.x : blockIdx.y;  // item = c * B + b
  const int C = a.C, B = a.B, E = 8 * C, NI = C * B;
  const int c = item / B, b = item - c * B;
  const bool qp = a.kind != PHY_JC69;
  ET_MARK(0);
  const double* eg = a.eig + (size_t)draw * EIG_LEN;
  const double* mdl = a.model + (size_t)draw * (10 + 2 * C);
  // this thread's column of P (tid < 16: (Q P)[kk][ll] needs P[.][ll]), loaded
  // with the eigensystem, ahead of the G sums it does not depend on
  double pcol[4] = {0.0, 0.0, 0.0, 0.0};
  if (MODE != 2 && tid < 16) {
    const double* P = a.pmat + (((size_t)draw * C + c) * a.nmat + a.gpos[b]) * a.R * 4;  // column-major
#pragma unroll
    for (int j = 0; j < 4; ++j) pcol[j] = P[(tid & 3) * 4 + j];
  }
  if (tid < 16) {
    sV[tid] = eg[EIG_M1 + tid];
    sVi[tid] = eg[EIG_M2 + tid];
    sQ[tid] = eg[EIG_Q + tid];
    srinv[tid] = phi_rinv(eg[EIG_LAM + (tid >> 2)], eg[EIG_LAM + (tid & 3)], PHI_NEAR);  // 0: tie or near tie
    if (tid < 4) slam[tid] = eg[EIG_LAM + tid];
  }
  // the first NS items: a slice of the root workgroups' scalar partials, in slot order
  const int NS = min(NI, EPI_SLICES);
  if constexpr (MODE == 1) {
  if (item < NS && tid >= NT - E) {
    const int en = tid - (NT - E);
    const int k0 = (int)((long long)item * a.nrootch / NS), k1 = (int)((long long)(item + 1) * a.nrootch / NS);
    const double* ss = a.sslot + (size_t)draw * a.nrootch * E + en;
    double acc = 0.0;  // in slot order, 8 loads in flight
    for (int k = k0; k < k1; k += 8) {
      double v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = k + u < k1 ? ss[(size_t)(k + u) * E] : 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u)
        if (k + u < k1) acc += v[u];
    }
    a.spart[((size_t)draw * NI + item) * E + en] = acc;
  }
  // G_cb: group q sums the partials q, q + EPI_GROUPS_T, ... (16 in flight)
  {
    const int pb = a.pbase[b];
    const int cntb = pb < 0 ? a.gcount[b] : (a.gcount[b] + GSUB_ROWS - 1) / GSUB_ROWS;
    const double* src = pb < 0 ? a.gpart + ((size_t)(draw * C + c) * a.ngs + a.gbase[b]) * 16 + e
                               : a.gpsum + ((size_t)(draw * C + c) * a.nsub + pb) * 16 + e;
    double u[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) u[v] = 0.0;
    for (int k0 = g; k0 < cntb; k0 += 16 * EPI_GROUPS_T) {
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int k = k0 + v * EPI_GROUPS_T;
        u[v] += (k < cntb) ? src[(size_t)k * 16] : 0.0;
      }
    }
    part[g][e] = (((u[0] + u[1]) + (u[2] + u[3])) + ((u[4] + u[5]) + (u[6] + u[7]))) +
                 (((u[8] + u[9]) + (u[10] + u[11])) + ((u[12] + u[13]) + (u[14] + u[15])));
  }
  __syncthreads();
  ET_MARK(1);
  if (tid < 16) {
    double gv = part[0][tid];
    for (int q = 1; q < EPI_GROUPS_T; ++q) gv += part[q][tid];
    sG[tid] = gv;
    a.grows[(size_t)draw * a.grows_stride + (size_t)item * 16 + tid] = gv;
  }
  __syncthreads();
  if (tid < 16) {
    const int kk = tid >> 2, ll = tid & 3;
    double qpv = 0.0;  // (Q P)[kk][ll] = sum_j Q[kk][j] P[j][ll]
#pragma unroll
    for (int j = 0; j < 4; ++j) qpv = fma(sQ[kk * 4 + j], pcol[j], qpv);
    sterm[tid] = sG[tid] * qpv;
    double m = 0.0;
    if (qp) {
      const double t = mdl[10 + c] * a.blens[(size_t)draw * B + b];
      double T[4];  // row kk of V^T G
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        double acc = 0.0;
#pragma unroll
        for (int i = 0; i < 4; ++i) acc = fma(sV[i * 4 + kk], sG[i * 4 + j], acc);
        T[j] = acc;
      }
      double hh = 0.0;  // (V^T G V^-T)[kk][ll]
#pragma unroll
      for (int j = 0; j < 4; ++j) hh = fma(T[j], sVi[ll * 4 + j], hh);
      const double Ek = exp(slam[kk] * t);
      const double ri = srinv[tid];
      const double El = exp(slam[ll] * t);
      const double phi = ri == 0.0 ? phi_close(slam[kk], slam[ll], t, Ek, El) : (Ek - El) * ri;
      m = hh * phi;
    }
    a.mpart[((size_t)draw * NI + item) * 16 + tid] = m;
  }
  __syncthreads();
  if (tid == 0) {
    double sv = 0.0;
    for (int q = 0; q < 16; ++q) sv += sterm[q];
    a.inner[(size_t)draw * NI + item] = sv;
  }
  ET_MARK(2);
  return;
  }  // (MODE 1)
  // ---- the closing workgroup of the draw (MODE 2): every hand-off load is
  // issued up front (scalars, M, this thread's branches' <G, QP> for every
  // category): one round trip instead of one per category
  auto ld1 = [](const double* q) { return *q; };
  double* out = a.out + (size_t)draw * a.outlen;
  const double* sp = a.spart + (size_t)draw * NI * E;
  const double* mp = a.mpart + (size_t)draw * NI * 16;
  const double* inr = a.inner + (size_t)draw * NI;
  const double* rs = mdl + 10;
  const double* blv = a.blens + (size_t)draw * B;
  double iv[EPI_CMAX];  // <G_cb, Q P_cb> of this thread's first branch (bb = tid), every category
#pragma unroll
  for (int cc = 0; cc < EPI_CMAX; ++cc) iv[cc] = (cc < C && tid < B) ? ld1(inr + (size_t)cc * B + tid) : 0.0;
  for (int idx = tid; idx < EPI_GROUPS_T * E; idx += NT) {  // scalars: group q sums slices q, q + G
    const int q = idx / E, en = idx - q * E;
    const double u0 = q < NS ? ld1(sp + (size_t)q * E + en) : 0.0;
    const double u1 = q + EPI_GROUPS_T < NS ? ld1(sp + (size_t)(q + EPI_GROUPS_T) * E + en) : 0.0;
    red[q][en] = u0 + u1;
  }
  {  // M: group g sums items g, g + G, ... (32 in flight: one round trip up to C*B = 1,024)
    double u[32];
#pragma unroll
    for (int v = 0; v < 32; ++v) u[v] = 0.0;
    for (int k0 = g; k0 < NI; k0 += 32 * EPI_GROUPS_T) {
#pragma unroll
      for (int v = 0; v < 32; ++v) {
        const int k = k0 + v * EPI_GROUPS_T;
        u[v] += (k < NI) ? ld1(mp + (size_t)k * 16 + e) : 0.0;
      }
    }
#pragma unroll
    for (int w = 16; w >= 1; w >>= 1)  // a fixed pairwise tree
#pragma unroll
      for (int v = 0; v < w; ++v) u[v] = u[2 * v] + u[2 * v + 1];
    part[g][e] = u[0];
    ET_MARK(3);
  }
  // dlogL/db = sum_c r_c <G_cb, Q P_cb> (this thread's branches); the
  // partials of dlogL/dr_c = sum_b b <G_cb, Q P_cb> in branch order
  double acc[EPI_CMAX];
#pragma unroll
  for (int cc = 0; cc < EPI_CMAX; ++cc) acc[cc] = 0.0;
  for (int bb = tid; bb < B; bb += NT) {
    if (bb != tid) {
#pragma unroll
      for (int cc = 0; cc < EPI_CMAX; ++cc) iv[cc] = cc < C ? ld1(inr + (size_t)cc * B + bb) : 0.0;
    }
    const double blb = blv[bb];
    double sv = 0.0;
#pragma unroll
    for (int cc = 0; cc < EPI_CMAX; ++cc)
      if (cc < C) {
        sv = fma(rs[cc], iv[cc], sv);
        acc[cc] = fma(blb, iv[cc], acc[cc]);
      }
    out[1 + bb] = sv;
  }
  ET_MARK(7);
  __syncthreads();
  ET_MARK(4);
  if (tid < E) {
    double tot = red[0][tid];
    for (int q = 1; q < EPI_GROUPS_T; ++q) tot += red[q][tid];
    red[0][tid] = tot;
  }
  if (tid >= 128 && tid < 144) {
    const int t = tid - 128;
    double tot = part[0][t];
    for (int q = 1; q < EPI_GROUPS_T; ++q) tot += part[q][t];
    sM[t] = tot;
  }
  __syncthreads();
  const int o = 1 + B + 2 * C;
  if (tid == 0) {
    const double ll = red[0][0];
    out[0] = isfinite(ll) ? ll : -INFINITY;
    for (int cc = 0; cc < C; ++cc) out[1 + B + C + cc] = red[0][cc * 8 + 1];
    for (int f = 0; f < 4; ++f) {
      double t = 0.0;
      for (int cc = 0; cc < C; ++cc) t += red[0][cc * 8 + 2 + f];
      out[o + f] = t;
      sroot[f] = t;
    }
  }
  // W = V^-T M V^T, one entry per thread (beside thread 0's sums; the
  // barriers below publish it to thread 0's q_tail)
  if (qp && tid >= 64 && tid < 80) sW[tid - 64] = w_entry(sM, sV, sVi, tid - 64);
  __syncthreads();  // thread 0 is done with red[0][.] before it is reused below
  // dlogL/dr_c: NT partials per category in a fixed tree, up to 8
  // categories per pass (group sums, then the 16 entries in order)
  for (int c0 = 0; c0 < C; c0 += 8) {
    const int nc = min(8, C - c0);
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j < nc) red[tid >> 4][j * 16 + (tid & 15)] = acc[c0 + j];
    __syncthreads();
    if (tid < 16 * nc) {
      double t = red[0][tid];
      for (int q = 1; q < EPI_GROUPS_T; ++q) t += red[q][tid];
      csum[tid >> 4][tid & 15] = t;
    }
    __syncthreads();
    if (tid < nc) {
      double t = csum[tid][0];
      for (int q = 1; q < 16; ++q) t += csum[tid][q];
      out[1 + B + c0 + tid] = t;
    }
    __syncthreads();
  }
  ET_MARK(5);
  if (tid != 0) return;
  if (!qp) {
    for (int k = 0; k < 10; ++k) out[o + 4 + k] = 0.0;
    return;
  }
  // the exchangeability / frequency gradients
  double W[16];
  for (int t = 0; t < 16; ++t) W[t] = sW[t];
  q_tail(W, sQ, eg[EIG_S], mdl, sroot, out + o);
  ET_MARK(6);
}

// ---- site log-likelihoods: pattern i <- its root class --------------------
__global__ void __launch_bounds__(256) cls_site_kernel(const double* sitecls, const int* pat_root, double* site,
                                                      int P, int nroot) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int draw = blockIdx.y;
  if (i < P) site[(size_t)draw * P + i] = sitecls[(size_t)draw * nroot + pat_root[i]];
}

// ===========================================================================
// host: the class plan (class_plan.h) on the device
// ===========================================================================
static_assert(sizeof(CPair) == sizeof(int2) && alignof(CPair) == alignof(int2), "CPair is the kernels' int2");
static_assert(sizeof(CQuad) == sizeof(int4) && alignof(CQuad) == alignof(int4), "CQuad is the kernels' int4");

struct ClassEngine : ClassSizes {
  int max_draws = 0;        // work buffers sized for this many draws
  // device plan (ClassPlan's tables)
  CNode* d_nodes = nullptr;
  CChunkN* d_chunks = nullptr;
  int* d_cls = nullptr;
  int* d_secpos = nullptr;
  int* d_stperm = nullptr;
  CTile* d_tiles = nullptr;
  CSpan* d_spans = nullptr;
  double* d_wroot = nullptr;
  int* d_pat_root = nullptr;
  int* d_gbase = nullptr;
  int* d_gcount = nullptr;
  int2* d_gsub = nullptr;
  int* d_pbase = nullptr;
  CladeLevel* d_clade = nullptr;
  int* d_rtile = nullptr;
  int* d_rspan = nullptr;
  int* d_lfix = nullptr;
  int2* d_sspan = nullptr;
  int2* d_pair = nullptr;
  int4* d_gc = nullptr;
  int2* d_clf = nullptr;
  int* d_clong = nullptr;
  CLink* d_link = nullptr;
  int* d_ctab = nullptr;
  int* d_crep = nullptr;
  // device work buffers (per draw)
  double* d_gpsum = nullptr;  // [dc][nsub][16] sub-range sums
  double* d_A = nullptr;
  double* d_RR = nullptr;
  double* d_STAGE = nullptr;
  double* d_PART0 = nullptr;
  double* d_PART1 = nullptr;
  double* d_gpart = nullptr;
  double* d_epi = nullptr;  // [draw][C*B (1 + 16 + 8C)]: the epilogue's hand-offs (inner, mpart, spart)
  double* d_sslot = nullptr;
  double* d_sroot = nullptr;
  double* d_sitecls = nullptr;
};

void free_class_engine(ClassEngine* e) {
  if (!e) return;
  void* ptrs[] = {e->d_nodes, e->d_chunks, e->d_cls,   e->d_secpos, e->d_stperm, e->d_clade, e->d_rtile, e->d_rspan, e->d_sspan,
                  e->d_tiles, e->d_spans,      e->d_wroot,    e->d_pat_root, e->d_gbase, e->d_gcount, e->d_gsub, e->d_pbase, e->d_gpsum,
                  e->d_A,     e->d_RR,         e->d_STAGE,    e->d_PART0,    e->d_PART1, e->d_gpart,
                  e->d_lfix,  e->d_sslot,      e->d_sroot,    e->d_sitecls, e->d_epi,
                  e->d_link,  e->d_ctab,  e->d_crep, e->d_pair, e->d_gc,
                  e->d_clf, e->d_clong};
  for (void* p : ptrs)
    if (p) (void)hipFree(p);
  delete e;
}

// Plan the class sweep (class_plan) and put its tables on the device, each
// host table released once it is uploaded (the synthetic plan's run to
// hundreds of MB, one plan per shard of a multi-device context).
int build_class_engine(int S, int P, int C, int rooted, const uint8_t* tipcodes, const double* weights,
                       const int32_t* peel, const std::vector<int>& vec_of, int R, int nmat,
                       const std::vector<int>& gpos, const ClassPrefs& prefs, ClassEngine** out) {
  ClassPlan p;
  int rc = class_plan(S, P, C, rooted, tipcodes, weights, peel, vec_of, R, nmat, gpos, prefs, p);
  if (rc) return rc;
  std::unique_ptr<ClassEngine, void (*)(ClassEngine*)> e(new ClassEngine(), free_class_engine);
  static_cast<ClassSizes&>(*e) = p;
  auto up = [](auto*& dptr, auto& vec) -> int {
    using T = typename std::remove_reference<decltype(vec)>::type::value_type;
    static_assert(sizeof(*dptr) == sizeof(T), "element sizes differ");
    int rc = dalloc(&dptr, std::max<size_t>(vec.size(), 1));
    if (rc) return rc;
    if (!vec.empty() && hipMemcpy(dptr, vec.data(), vec.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess)
      return fail(PHY_EHIP, "hipMemcpy (class plan)");
    std::vector<T>().swap(vec);
    return PHY_OK;
  };
  if (p.chain_m && ((rc = up(e->d_link, p.links)) || (rc = up(e->d_ctab, p.ctab)) || (rc = up(e->d_crep, p.crep))))
    return rc;
  if ((rc = up(e->d_nodes, p.nodes)) || (rc = up(e->d_chunks, p.chunks)) || (rc = up(e->d_cls, p.cls)) ||
      (rc = up(e->d_secpos, p.secpos)) || (rc = up(e->d_stperm, p.stperm)) || (rc = up(e->d_tiles, p.tiles)) ||
      (rc = up(e->d_spans, p.spans)) || (rc = up(e->d_wroot, p.wroot)) || (rc = up(e->d_pat_root, p.pat_root)) ||
      (rc = up(e->d_gbase, p.gbase)) || (rc = up(e->d_gcount, p.gcount)) || (rc = up(e->d_gsub, p.gsub)) ||
      (rc = up(e->d_pbase, p.pbase)) || (rc = up(e->d_clade, p.clade)) || (rc = up(e->d_rtile, p.rtile)) ||
      (rc = up(e->d_rspan, p.rspan)) || (rc = up(e->d_lfix, p.lfix)) || (rc = up(e->d_sspan, p.sspan)) ||
      (rc = up(e->d_pair, p.pair)) || (rc = up(e->d_clf, p.clf)) || (rc = up(e->d_clong, p.clong)) ||
      (rc = up(e->d_gc, p.gc)))
    return rc;
  *out = e.release();
  return PHY_OK;
}

// Work buffers for n draws (grown on demand).
// The ticket counters are zeroed on the stream the evaluation runs on
// (hipMemsetAsync): a plain hipMemset goes to the null stream, which the
// contexts' non-blocking streams do not wait for -- concurrent shards' first
// kernels could then add to counters the memset clears afterwards.
int class_engine_reserve(ClassEngine* e, int n, hipStream_t st) {
  if (n <= e->max_draws) return PHY_OK;
  double** bufs[] = {&e->d_A, &e->d_RR, &e->d_STAGE, &e->d_PART0, &e->d_PART1, &e->d_gpart, &e->d_sslot, &e->d_sroot,
                     &e->d_sitecls, &e->d_gpsum};
  for (double** b : bufs)
    if (*b) {
      (void)hipFree(*b);
      *b = nullptr;
    }
  if (e->d_epi) {
    (void)hipFree(e->d_epi);
    e->d_epi = nullptr;
  }
  e->max_draws = 0;
  const size_t dcn = (size_t)n * e->C;
  int rc;
  if ((rc = dalloc(&e->d_A, dcn * std::max(e->nslots, 1) * 4))) return rc;
  if ((rc = dalloc(&e->d_RR, dcn * std::max(e->nslots, 1) * 4))) return rc;
  if ((rc = dalloc(&e->d_STAGE, dcn * e->nstage * 4))) return rc;
  if ((rc = dalloc(&e->d_PART0, dcn * e->ntiles * 4))) return rc;
  if ((rc = dalloc(&e->d_PART1, dcn * e->ntiles * 4))) return rc;
  if ((rc = dalloc(&e->d_gpart, dcn * std::max(e->ngs, 1) * 16))) return rc;
  if ((rc = dalloc(&e->d_gpsum, dcn * std::max(e->nsub, 1) * 16))) return rc;
  if ((rc = dalloc(&e->d_epi, (size_t)n * e->C * e->B * (1 + 16 + 8 * (size_t)e->C)))) return rc;
  if ((rc = dalloc(&e->d_sslot, (size_t)n * e->nrootch * e->C * 8))) return rc;
  if ((rc = dalloc(&e->d_sroot, (size_t)n * e->nroot))) return rc;
  if ((rc = dalloc(&e->d_sitecls, (size_t)n * e->nroot))) return rc;
  e->max_draws = n;
  return PHY_OK;
}

ClassArgs class_args(const ClassEngine* e, const double* d_pmat, const double* d_model, unsigned long long extra) {
  ClassArgs a;
  a.nodes = e->d_nodes;
  a.chunks = e->d_chunks;
  a.cls = e->d_cls;
  a.secpos = e->d_secpos;
  a.stperm = e->d_stperm;
  a.tiles = e->d_tiles;
  a.spans = e->d_spans;
  a.pmat = d_pmat;
  a.model = d_model;
  a.wroot = e->d_wroot;
  a.A = e->d_A;
  a.RR = e->d_RR;
  a.STAGE = e->d_STAGE;
  a.PART0 = e->d_PART0;
  a.PART1 = e->d_PART1;
  a.gpart = e->d_gpart;
  a.sspan = e->d_sspan;
  a.nspans = std::max(e->nspans, 1);
  a.sslot = e->d_sslot;
  a.sroot = e->d_sroot;
  a.sitecls = e->d_sitecls;
  a.C = e->C;
  a.nmat = e->nmat;
  a.R = e->R;
  a.nslots = std::max(e->nslots, 1);
  a.nstage = e->nstage;
  a.ntiles = e->ntiles;
  a.ngs = std::max(e->ngs, 1);
  a.nroot = e->nroot;
  a.nrootch = e->nrootch;
  a.rootr = e->rootr;

  a.root = e->root;
  a.rootoff = e->rootoff;
  a.first = a.count = 0;
  a.sfirst = 0;
  a.sord = 0;
  a.extra = extra;
  return a;
}
