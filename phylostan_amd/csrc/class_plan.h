// class_plan.h -- the host planner of the class sweep (class_engine.inc): the
// subtree classes of every node, the level / clade / chain layout of their
// slots, the staging tiles and tile-crossing segments of the reverse, and every
// table the cls_* kernels read.
//
// Plain C++17 like sweep_plan.h, which it builds on (WAVE, fail, g_err, the
// PHY_* codes): no HIP header, no device memory.  class_engine.inc uploads what
// class_plan leaves in a ClassPlan; tests/class_plan_check.cpp compiles this
// file with a host compiler alone.  The records the kernels share (CNode,
// CChunkN, CTile, CSpan, CLink, CladeLevel) are laid out here.
#ifndef PHYLO_CLASS_PLAN_H
#define PHYLO_CLASS_PLAN_H

#include <cstring>

#include "sweep_plan.h"

namespace {

constexpr int ROOT_CHUNK = 64;   // root classes per round of a root workgroup (one per lane of each category wave)
#ifndef PHY_SPAN_LANE_MAX
#define PHY_SPAN_LANE_MAX 32
#endif
constexpr int SPAN_LANE_MAX = PHY_SPAN_LANE_MAX;  // segments crossing at most this many tiles past their first: summed by their REV lane
constexpr long long STAGE_PORDER_MIN = 100000;  // staged classes of a level from which its staging is written in
                                                // parent class order (contribute_inner; synthetic: the one-GPU
                                                // plan's levels 4, 9, 11, 12, none of the shard-of-8 plan's;
                                                // 60,000 -- level 10 too -- measured the same)
constexpr int ROOT_WGS = 8192;   // root workgroups wanted: a workgroup runs ceil(chunks / ROOT_WGS) rounds, so
                                 // its scalar / dL/dP partials (what the epilogue sums) stay ~4k per draw
                                 // (one GPU, synthetic: 2,048 / 4,096 / 8,192 / 16,384 -> 1,869-1,886 /
                                 // 1,902-1,906 / 1,915-1,918 / 1,909-1,912 evals/s; PHY_ROOT_WGS overrides)
constexpr int CHAIN_MAX = 8;     // levels of the top chain (cls_chain_*)
constexpr int GSUB_ROWS = 512;   // rows per sub-range (16 groups x 32 rows in flight)
constexpr int GSUB_MIN = 1024;   // branches with more rows than this are pre-summed (none in a shard of 8)
// Bottom clades: the deepest Lc <= L-2 whose largest clade (a maximal
// subtree of nodes at levels <= Lc) has at most CLADE_CAP classes, so one
// workgroup runs each fused level in about one round; PHY_CLADE sets Lc
// (0: off).  Measured on the synthetic workload (one GPU / one 8-way shard,
// step ms): Lc 0 0.734 / 0.329, 3 (largest clade 816 / 455 classes) 0.722 /
// 0.314, 4 (3781 / 1600) 0.757 / 0.317 -- past about one round per level
// the single workgroup is slower than the level-wide launches.
constexpr long long CLADE_CAP = 1024;

// int2 / int4 of the device tables (class_engine.inc asserts the layouts equal)
struct alignas(8) CPair {
  int x, y;
};
struct alignas(16) CQuad {
  int x, y, z, w;
};

struct CChunk {  // one wave's work: classes [j0, j0+jn) of a node
  int node, j0, jn;
  int ci;        // chunk index inside the node (its GPART slot offset)
  int pad0, pad1, pad2, pad3;
};

struct CNode {  // 16 ints, device copy of a node's class plan
  int off;     // slot offset (A / RR / cls arrays) of this node's classes
  int n;       // classes
  int offx;    // slot offset of child x (internal) or -1 (tip)
  int offy;
  int mv;      // matrix record of v's branch, -1 (root / merged branch: identity)
  int mx;      // matrix record of a tip x (its branch), -1 if internal
  int my;
  int stx;     // staging offset of internal x's incoming contributions (-1 tip)
  int sty;
  int secy;    // 1: y is the secondary child, 0: x is
  int gv;      // GPART base slot of v's branch (-1 none)
  int gx;      // GPART base slot of tip x's branch (-1: x internal)
  int gy;
  int sin;     // staging offset of v's own incoming contributions (-1: root, or v is its parent's primary child)
  int ptile;   // reduction tile of v's primary internal child for v's first 64 classes (-1: the primary is a tip)
  int sord;    // 1: the secondary child's staging is written in v's class order (contribute_inner)
};

// A chunk with its node's plan inlined (the device copy the FWD / REV waves
// read): one 80-byte scalar load pair instead of the chunk, then (dependent)
// its node.
struct CChunkN {
  CNode nd;
  int j0, jn, ci, node;
};

struct CTile {  // one 64-position tile of a node's staging array
  int node;
  int t;         // tile index inside the node's staging array
  unsigned lo, hi;  // head mask: bit l = position 64t+l starts a segment
  int kfirst;    // child class (segment id) of position 64t
  int flags;     // bit0: lane-0 segment started before the tile; bit1: lane-63 segment continues after
  int m;         // staging length (= the parent's class count)
  int sb;        // staging position of the tile's lane 0 (secondary children; -1: a primary child's tile)
};

struct CSpan {  // a segment crossing tiles: R[k] = PART1[t0] + sum PART0[t0+1..t1]
  int node, k, t0, t1;
};

struct CLink {     // chain node i (0: bottom, m-1: top)
  int off;         // slot offset of its classes
  int mv;          // its matrix record (-1: identity: a merged root branch)
  int spine;       // 0: child x is c_{i-1}, 1: child y is; -1: the bottom (both children external)
  int offx, offy;  // external children: slot offsets (-1: a tip)
  int mx, my;      // external tips: matrix records
  int gv;          // GPART base slot of its branch (-1: none), one row per top chunk
  int gx, gy;      // GPART base slots of external tip children (-1: none)
  int stx, sty;    // staging base of external internal children (-1: none)
  int pad0, pad1, pad2, pad3;
};

struct CladeLevel {  // one clade's work at one level: ranges into chunks / RED tiles / spans
  int chunk0, nchunk, tile0, ntile, span0, nspan, pad0, pad1;
};

struct ClassLevel {
  int chunk0, nchunk;  // chunks of this level's nodes (forward / reverse)
  int tile0, ntile;    // RED tiles of this level's secondary children (their primary siblings' tiles follow,
                       // reduced inside the parents' reverse)
  int span0, nspan;    // tile-crossing segments of this level's nodes
  int lfix0, nlfix;    // the long ones among them (a FIX launch over an index list; the rest summed by REV lanes)
  int sec0;            // staging tile of the RED range's first tile (ClassArgs::sfirst)
  int pair;            // 1: this level and the next run as one forward launch (cls_fwd2_kernel); 2: the next's
  int revfix;          // 1: the long spans are summed by the REV chunks (cls_rev_ls_kernel), no FIX launch
  int sord;            // 1: its secondary children's staging is written in parent class order (contribute_inner)
};

// open-addressing map uint64 key -> int (reused across nodes)
struct KeyMap {
  std::vector<unsigned long long> key;
  std::vector<int> val;
  unsigned long long mask = 0;
  static constexpr unsigned long long EMPTY = ~0ull;
  void init(size_t n) {
    size_t cap = 16;
    while (cap < 2 * n) cap <<= 1;
    key.assign(cap, EMPTY);
    val.assign(cap, -1);
    mask = cap - 1;
  }
  static unsigned long long hash(unsigned long long k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdull;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ull;
    k ^= k >> 33;
    return k;
  }
  // slot of k (inserted if new; `fresh` tells)
  size_t find(unsigned long long k, bool& fresh) {
    size_t h = hash(k) & mask;
    while (key[h] != EMPTY && key[h] != k) h = (h + 1) & mask;
    fresh = key[h] == EMPTY;
    if (fresh) key[h] = k;
    return h;
  }
  void clear(const std::vector<unsigned long long>& used) {
    for (unsigned long long k : used) {
      size_t h = hash(k) & mask;
      while (key[h] != k) h = (h + 1) & mask;
      key[h] = EMPTY;  // tombstone-free: every key of this round is cleared, so probe chains vanish together
      val[h] = -1;
    }
  }
};

// The class plan's preferences: the environment's when the engine is built
// (class_prefs_from_env, from select_engine).
struct ClassPrefs {
  int clade = -1;          // PHY_CLADE: bottom-clade levels (0: off; < 0: the deepest within CLADE_CAP)
  bool chain = true;       // PHY_CHAIN=0: no top chain
  int root_wgs = ROOT_WGS; // PHY_ROOT_WGS (A/B: root workgroups wanted)
  long long stage_order = STAGE_PORDER_MIN;  // PHY_STAGE_ORDER (tests: the threshold in staged classes; 0: every level)
  bool pair = true;        // PHY_PAIR=0: no forward level pairs
  long long pair_max = LLONG_MAX;  // PHY_PAIR_MAX: only upper levels of at most this many classes
  bool revfix = true;      // PHY_REVFIX=0: the long spans by FIX launches
  bool root_chain = true;  // PHY_ROOT_CHAIN=0: the chain's own forward launch
};

ClassPrefs class_prefs_from_env() {
  auto flag = [](const char* name) {
    const char* v = getenv(name);
    return !(v && atoi(v) == 0);
  };
  ClassPrefs p;
  if (const char* v = getenv("PHY_CLADE")) p.clade = atoi(v);
  p.chain = flag("PHY_CHAIN");
  if (const char* v = getenv("PHY_ROOT_WGS")) p.root_wgs = std::max(1, atoi(v));
  if (const char* v = getenv("PHY_STAGE_ORDER")) p.stage_order = atoll(v);
  p.pair = flag("PHY_PAIR");
  if (const char* v = getenv("PHY_PAIR_MAX")) p.pair_max = atoll(v);
  p.revfix = flag("PHY_REVFIX");
  p.root_chain = flag("PHY_ROOT_CHAIN");
  return p;
}

// What the launches and the fact calls read of a plan (ClassEngine keeps these).
struct ClassSizes {
  int S = 0, P = 0, C = 0, R = 0, nmat = 0, B = 0;
  int nslots = 0, nstage = 0, ntiles = 0, ngs = 0, nroot = 0, nrootch = 0, root = 0;
  int rootoff = 0;          // slot of the root's first class
  int rootr = 1;            // rounds of ROOT_CHUNK classes per root workgroup
  int root_tips = 1;        // a child of the root is a tip (cls_root_kernel's dL/dP accumulators)
  int levels = 0;           // L: the root's level
  int max_gcount = 0;       // most dL/dP chunk partials of one branch
  long long classes = 0;    // non-root internal classes (the forward's work)
  long long stage_elems = 0;  // sum over internal nodes of classes x internal children (the reverse's scatter)
  long long stage_sec = 0;    // the part of it that goes through staging (secondary children)
  std::vector<ClassLevel> lv;  // index = level (1..L-1)
  int Lc = 0;               // levels 1..Lc run as bottom clades (0: none)
  int nclade = 0;
  long long clade_max = 0;  // classes of the largest clade
  int nrtile = 0, nrspan = 0;  // the clade roots' RED tiles / long FIX spans (run before the clade kernel)
  long long lane_spans = 0, long_spans = 0;
  int nspans = 0;           // tile-crossing segments (all levels)
  int nsub = 0;             // long branches' dL/dP partial rows pre-summed in GSUB_ROWS sub-ranges (cls_gsum_kernel)
  // the top chain (cls_chain_fwd / cls_chain_rev): levels lo..hi, one node each
  int chain_m = 0, chain_lo = 0, chain_hi = 0, chain_ntop = 0, chain_ntp = 0, chain_toff = 0;
  int npairs = 0;           // forward level pairs (cls_fwd2_kernel)
  int nsord = 0;            // levels whose staging is written in parent class order (ClassLevel::sord)
  int nclong = 0;           // long spans summed by the REV chunks (cls_rev_ls_kernel)
  int root_chain_pref = 1;  // the root recomputes the chain's top (no chain forward launch; PHY_ROOT_CHAIN=0: off)
};

// The sizes and the host tables the engine uploads.
struct ClassPlan : ClassSizes {
  std::vector<CNode> nodes;
  std::vector<CChunkN> chunks;
  std::vector<int> cls;      // [slot][2]: child classes (x, y); tips: record index
  std::vector<int> secpos;   // [slot] staging position for the secondary child (sord = 0)
  std::vector<int> stperm;   // [nstage] staging position -> the STAGE entry its contribution was written to
  std::vector<CTile> tiles;
  std::vector<CSpan> spans;
  std::vector<double> wroot;  // [nroot] pattern weight of each root class
  std::vector<int> pat_root;  // [P] root class of each pattern
  std::vector<int> gbase, gcount;  // [B] GPART rows of branch b
  std::vector<CPair> gsub;   // [nsub] (first GPART row, rows)
  std::vector<int> pbase;    // [B] first sub-range of branch b (-1: summed by cls_epi_kernel directly)
  std::vector<CladeLevel> clade;  // [nclade][Lc]
  std::vector<int> rtile, rspan;
  std::vector<int> lfix;     // long spans of the level-wide levels, per level (ClassLevel::lfix0 / nlfix)
  std::vector<CPair> sspan;  // [slot] lane-summed span of the class, or (0, 0)
  std::vector<CPair> pair;   // per chunk of a pair's upper level: the recomputed children
  std::vector<CQuad> gc;     // per slot of those chunks: the children's children's classes
  std::vector<CPair> clf;    // per chunk (first, count) into clong
  std::vector<int> clong;
  std::vector<CLink> links;  // [chain_m]
  std::vector<int> ctab;     // [5][chain_m][chain_ntp] (ChainArgs::tab)
  std::vector<int> crep;     // [chain_ntp]
};

// The working arrays the phases of class_plan share (node-indexed unless said).
struct ClassWork {
  int S, P, N, root, merged, L;
  const int32_t* peel;
  std::vector<int> ch1, ch2, par, level;
  std::vector<int> ncls;
  std::vector<std::vector<CPair>> kids;  // per class: (class of x, class of y)
  std::vector<std::vector<int>> secp;    // per class: staging position for the secondary child
  std::vector<int> prim_is_y;
  std::vector<int> cid;                  // bottom clade of a node (-1: none)
  std::vector<int> chn;                  // chn[i]: the chain's node of level lo + i
  std::vector<int> in_chain;             // chain index of a node
  std::vector<char> chain_ext;           // an internal node whose parent is a chain node, not itself in the chain
  int cm = 0, ctop = -1, ntop = 0, ntp = 0;
  std::vector<int> order;                // non-root internal nodes by (level, clade, id)
  std::vector<int> off, sin;
  int cls_slots = 0;
  std::vector<std::vector<CSpan>> node_spans;
  std::vector<CChunk> chunks;

  // staging: only a node that is its parent's *secondary* child receives its
  // contributions through HBM (the primary child's are reduced in registers)
  // (the chain: its externals receive the top classes' shares through staging
  // -- ntop positions each; the chain nodes below the top receive nothing)
  bool is_primary(int u) const {
    if (chain_ext[u]) return false;
    const int v = par[u];
    return (ch2[v] == u) == (prim_is_y[v] != 0);
  }
  bool chained(int u) const { return in_chain[u] >= 0 && u != ctop; }
  int stage_len(int u) const { return chain_ext[u] ? ntop : ncls[par[u]]; }
  bool sord_of(const ClassPlan& p, int u) const {
    return u >= S && sin[u] >= 0 && !chain_ext[u] && p.lv[level[u]].sord;
  }
  int& CT(ClassPlan& p, int w, int i, int kt) const { return p.ctab[((size_t)w * cm + i) * ntp + kt]; }
};

// ---- classes, bottom-up (peel order is a post-order)
void plan_classes(ClassPlan& p, ClassWork& w, const uint8_t* tipcodes, const std::vector<int>& vec_of) {
  const int S = w.S, P = w.P, N = w.N;
  std::vector<std::vector<int>> cls(N);  // per pattern class id (freed once the parent is built)
  w.ncls.assign(N, 0);
  for (int t = 0; t < S; ++t) {
    cls[t].resize(P);
    for (int i = 0; i < P; ++i) cls[t][i] = vec_of[tipcodes[(size_t)t * P + i]];
    w.ncls[t] = p.R;
  }
  w.kids.resize(N);
  w.secp.resize(N);
  w.prim_is_y.assign(N, 0);
  KeyMap km;
  km.init((size_t)P);
  std::vector<unsigned long long> uniq;
  for (int r = 0; r < S - 1; ++r) {
    const int x = w.peel[3 * r], y = w.peel[3 * r + 1], v = w.peel[3 * r + 2];
    // primary child: internal, the one with more classes
    bool py;
    if (x >= S && y >= S) py = w.ncls[y] > w.ncls[x];
    else py = (y >= S && x < S);
    const int pc = py ? y : x, sc = py ? x : y;
    w.prim_is_y[v] = py;
    const unsigned long long nsec = (unsigned long long)w.ncls[sc];
    uniq.clear();
    for (int i = 0; i < P; ++i) {
      const unsigned long long k = (unsigned long long)cls[pc][i] * nsec + (unsigned long long)cls[sc][i];
      bool fresh;
      km.find(k, fresh);
      if (fresh) uniq.push_back(k);
    }
    std::vector<unsigned long long> sorted = uniq;
    std::sort(sorted.begin(), sorted.end());  // primary-major class order
    for (size_t q = 0; q < sorted.size(); ++q) {
      bool fresh;
      km.val[km.find(sorted[q], fresh)] = (int)q;
    }
    std::vector<int> cv(P);
    for (int i = 0; i < P; ++i) {
      const unsigned long long k = (unsigned long long)cls[pc][i] * nsec + (unsigned long long)cls[sc][i];
      bool fresh;
      cv[i] = km.val[km.find(k, fresh)];
    }
    km.clear(uniq);
    const int n = (int)sorted.size();
    w.ncls[v] = n;
    w.kids[v].resize(n);
    for (int q = 0; q < n; ++q) {
      const int kp = (int)(sorted[q] / nsec), ks = (int)(sorted[q] % nsec);
      w.kids[v][q] = py ? CPair{ks, kp} : CPair{kp, ks};
    }
    // staging positions for the secondary child: classes ordered by its class (stable)
    {
      std::vector<int> cnt(w.ncls[sc] + 1, 0);
      for (int q = 0; q < n; ++q) cnt[1 + (int)(sorted[q] % nsec)]++;
      for (int k = 0; k < w.ncls[sc]; ++k) cnt[k + 1] += cnt[k];
      w.secp[v].resize(n);
      for (int q = 0; q < n; ++q) w.secp[v][q] = cnt[(int)(sorted[q] % nsec)]++;
    }
    cls[v].swap(cv);
    if (x >= S) std::vector<int>().swap(cls[x]);
    if (y >= S) std::vector<int>().swap(cls[y]);
  }
  p.pat_root.swap(cls[w.root]);
}

// ---- bottom clades (CLADE_CAP above)
void plan_clades(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs) {
  const int S = w.S, N = w.N, L = w.L;
  w.cid.assign(N, -1);
  auto clades_at = [&](int lc, std::vector<int>& id, int& n, long long& mx) {
    std::fill(id.begin(), id.end(), -1);
    std::vector<long long> sz;
    n = 0;
    mx = 0;
    for (int v = S; v < N; ++v) {  // clade roots in id order
      if (v == w.root || w.level[v] > lc || w.level[w.par[v]] <= lc) continue;
      id[v] = n++;
      sz.push_back(0);
    }
    // every other node at level <= lc joins its parent's clade (parents
    // have larger ids in a post-order numbering, so walk ids downwards)
    for (int v = N - 1; v >= S; --v)
      if (v != w.root && w.level[v] <= lc && id[v] < 0) id[v] = id[w.par[v]];
    for (int v = S; v < N; ++v)
      if (id[v] >= 0) sz[id[v]] += w.ncls[v];
    for (long long z : sz) mx = std::max(mx, z);
  };
  const int want = prefs.clade;
  std::vector<int> id(N, -1);
  int n;
  long long mx;
  if (want >= 0) {
    p.Lc = std::min(want, L - 2);
  } else {
    for (int lc = L - 2; lc >= 2; --lc) {
      clades_at(lc, id, n, mx);
      if (mx <= CLADE_CAP) {
        p.Lc = lc;
        break;
      }
    }
  }
  if (p.Lc < 1) p.Lc = 0;
  if (p.Lc > 0) clades_at(p.Lc, w.cid, p.nclade, p.clade_max);
}

// ---- the top chain: the run of single-node levels below the root (at
// least 2, above the clade levels, the top CHAIN_MAX of them); PHY_CHAIN=0:
// none.  Then its tables: per top class kt the class of every chain node and of
// its children, by walking down the chain through kids (tab[0..2]);
// representatives
void plan_chain(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs) {
  const int S = w.S, N = w.N, L = w.L;
  w.in_chain.assign(N, -1);
  w.chain_ext.assign(N, 0);
  if (prefs.chain) {
    std::vector<int> cnt(L + 1, 0), one(L + 1, -1);
    for (int v = S; v < N; ++v)
      if (v != w.root) {
        cnt[w.level[v]]++;
        one[w.level[v]] = v;
      }
    // A chained node's externals receive one share per TOP class (staged,
    // segment-reduced), more than per own class; a floor on the chained
    // levels' classes measured slower (shard of 8, top 47k classes: no chain
    // 4,501 evals/s, chain of 4 stopped at a quarter 4,541, chain of 5 4,630).
    // A big top (more than 131,072 classes) takes no chain: its levels are
    // bandwidth-bound, not latency-bound (one GPU, top 350k: 1,800 -> 1,643
    // with the chain).
    constexpr long long maxtop = 131072;
    const int top = cnt[L - 1] == 1 ? one[L - 1] : -1;
    int lo = L;
    if (top >= 0 && w.ncls[top] <= maxtop)
      for (int l = L - 1; l > std::max(p.Lc, 0) && cnt[l] == 1 && L - l <= CHAIN_MAX; --l) lo = l;
    if (L - lo >= 2)
      for (int l = lo; l < L; ++l) w.chn.push_back(one[l]);
  }
  for (size_t i = 0; i < w.chn.size(); ++i) w.in_chain[w.chn[i]] = (int)i;
  for (size_t i = 0; i < w.chn.size(); ++i)
    for (int u : {w.ch1[w.chn[i]], w.ch2[w.chn[i]]})
      if (u >= S && w.in_chain[u] < 0) w.chain_ext[u] = 1;
  const int cm = w.cm = (int)w.chn.size();
  w.ctop = cm ? w.chn[cm - 1] : -1;
  const int ntop = w.ntop = cm ? w.ncls[w.ctop] : 0;
  w.ntp = (ntop + WAVE - 1) / WAVE * WAVE;
  p.ctab.assign((size_t)5 * std::max(cm, 1) * std::max(w.ntp, 1), 0);
  p.crep.assign(std::max(w.ntp, 1), 0);
  for (int i = cm - 1; i >= 0; --i) {
    const int v = w.chn[i];
    std::vector<char> seen(w.ncls[v], 0);
    for (int kt = 0; kt < ntop; ++kt) {
      const int k = i == cm - 1 ? kt : (w.ch1[w.chn[i + 1]] == v ? w.CT(p, 1, i + 1, kt) : w.CT(p, 2, i + 1, kt));
      w.CT(p, 0, i, kt) = k;
      w.CT(p, 1, i, kt) = w.kids[v][k].x;
      w.CT(p, 2, i, kt) = w.kids[v][k].y;
      if (!seen[k]) {
        seen[k] = 1;
        p.crep[kt] |= 1 << i;
      }
    }
  }
}

// ---- layout: non-root internal nodes by (level, clade, id), then the root;
// the staging ranges, and the staging order per level
void plan_layout(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs) {
  const int S = w.S, N = w.N, L = w.L;
  for (int l = 1; l < L; ++l) {
    const size_t o0 = w.order.size();
    for (int v = S; v < N; ++v)
      if (v != w.root && w.level[v] == l) w.order.push_back(v);
    if (l <= p.Lc)  // clade roots first, then by clade: each clade's chunks / tiles / spans of a level form
                    // one range (a clade root is the only node of its clade at its level)
      std::stable_sort(w.order.begin() + o0, w.order.end(), [&](int u, int x) {
        const bool ru = w.level[w.par[u]] > p.Lc, rx = w.level[w.par[x]] > p.Lc;
        if (ru != rx) return ru;
        return w.cid[u] < w.cid[x];
      });
  }
  w.off.assign(N, -1);
  int slot = 0;
  for (int v : w.order) {  // chunk-major: a node's classes padded to whole 64-class chunks (fwd_chunk)
    w.off[v] = slot;
    slot += (w.ncls[v] + WAVE - 1) / WAVE * WAVE;
    p.classes += w.ncls[v];
  }
  p.nslots = slot;  // A / RR cover the non-root nodes only
  w.off[w.root] = slot;
  p.rootoff = slot;
  w.cls_slots = slot + w.ncls[w.root];
  // staging ranges: each internal non-root node receives its parent's class count (ClassWork::is_primary)
  w.sin.assign(N, -1);
  int st = 0;
  for (int v : w.order) {
    if (w.chained(v)) continue;
    p.stage_elems += w.stage_len(v);
    if (w.is_primary(v)) continue;
    w.sin[v] = st;  // tile-major: whole 64-position tiles, in RED-tile order (red_tile)
    st += (w.stage_len(v) + WAVE - 1) / WAVE * WAVE;
    p.stage_sec += w.stage_len(v);
  }
  p.nstage = std::max(st, 8);
  p.lv.assign(L + 1, ClassLevel{0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0});
  // staging order per level (contribute_inner): the parent's class order where
  // the level's secondary children stage the most classes
  std::vector<long long> stl(L + 1, 0);
  for (int u = S; u < N; ++u)
    if (w.sin[u] >= 0 && !w.chain_ext[u]) stl[w.level[u]] += w.stage_len(u);
  const long long thr = prefs.stage_order;
  for (int l = p.Lc + 1; l < L; ++l) {
    p.lv[l].sord = stl[l] > 0 && stl[l] >= thr ? 1 : 0;
    p.nsord += p.lv[l].sord;
  }
}

// ---- nodes and dL/dP slots.  GPART slots: one per chunk (64 classes; the
// root's: one per root workgroup) of the contributing node
int plan_nodes(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs, const std::vector<int>& gpos) {
  const int S = w.S, N = w.N, root = w.root;
  p.nodes.resize(N);
  p.gbase.assign(p.B, -1);
  p.gcount.assign(p.B, 0);
  int ngs = 0;
  {
    const int rch = (w.ncls[root] + ROOT_CHUNK - 1) / ROOT_CHUNK;
    p.rootr = std::max(1, (rch + prefs.root_wgs - 1) / prefs.root_wgs);
  }
  auto nchunks = [&](int v) {
    return v == root ? ((w.ncls[v] + ROOT_CHUNK - 1) / ROOT_CHUNK + p.rootr - 1) / p.rootr : (w.ncls[v] + WAVE - 1) / WAVE;
  };
  // dL/dP partial rows: a chain node contributes one per top chunk
  auto gchunks = [&](int v) { return w.in_chain[v] >= 0 ? w.ntp / WAVE : nchunks(v); };
  for (int v = S; v < N; ++v) {
    CNode& nd = p.nodes[v];
    std::memset(&nd, 0xff, sizeof(nd));  // -1 everywhere
    const int x = w.ch1[v], y = w.ch2[v];
    nd.off = w.off[v];
    nd.n = w.ncls[v];
    nd.offx = x >= S ? w.off[x] : -1;
    nd.offy = y >= S ? w.off[y] : -1;
    nd.mv = (v != root && v != w.merged) ? gpos[v] : -1;
    nd.mx = x < S ? gpos[x] : -1;
    nd.my = y < S ? gpos[y] : -1;
    nd.stx = x >= S ? w.sin[x] : -1;
    nd.sty = y >= S ? w.sin[y] : -1;
    nd.secy = w.prim_is_y[v] ? 0 : 1;
    nd.sin = w.sin[v];
    nd.ptile = -1;
    const int nch = gchunks(v);
    if (nd.mv >= 0) {
      nd.gv = ngs;
      p.gbase[v] = ngs;
      p.gcount[v] = nch;
      ngs += nch;
    }
    if (x < S) {
      nd.gx = ngs;
      p.gbase[x] = ngs;
      p.gcount[x] = nch;
      ngs += nch;
    }
    if (y < S) {
      nd.gy = ngs;
      p.gbase[y] = ngs;
      p.gcount[y] = nch;
      ngs += nch;
    }
    nd.sord = w.sord_of(p, w.prim_is_y[v] ? x : y) ? 1 : 0;  // (the secondary child)
  }
  for (int b = 0; b < p.B; ++b)
    if (p.gbase[b] < 0)
      return fail(PHY_EINVAL, "internal: class plan has no dL/dP contributor for branch " + std::to_string(b));
  p.ngs = ngs;
  for (int b = 0; b < p.B; ++b) p.max_gcount = std::max(p.max_gcount, p.gcount[b]);
  p.nroot = w.ncls[root];
  p.nrootch = nchunks(root);
  p.root_tips = (p.nodes[root].offx < 0 || p.nodes[root].offy < 0) ? 1 : 0;
  return PHY_OK;
}

// ---- RED tiles per level (a node's staging is reduced at its own level)
// and the tile-crossing segments of every node (finished by its REV chunks)
int plan_tiles(ClassPlan& p, ClassWork& w) {
  const int S = w.S, N = w.N, L = w.L, cm = w.cm, ntop = w.ntop;
  std::vector<CTile>& tiles = p.tiles;
  w.node_spans.resize(N);
  std::vector<int> tile_first(N, -1);
  // the chain externals' staging order: the top classes, stably by the external's class
  // (tab[3] / tab[4]: a top class's position in its x / y external's staging)
  for (int i = 0; i < cm; ++i)
    for (int c = 1; c <= 2; ++c) {
      const int u = c == 1 ? w.ch1[w.chn[i]] : w.ch2[w.chn[i]];
      if (u < S || !w.chain_ext[u]) continue;
      std::vector<int> cnt(w.ncls[u] + 1, 0);
      for (int kt = 0; kt < ntop; ++kt) cnt[1 + w.CT(p, c, i, kt)]++;
      for (int k = 0; k < w.ncls[u]; ++k) cnt[k + 1] += cnt[k];
      for (int kt = 0; kt < ntop; ++kt) w.CT(p, 2 + c, i, kt) = cnt[w.CT(p, c, i, kt)]++;
    }
  for (int l = 1; l < L; ++l) {
    p.lv[l].tile0 = (int)tiles.size();
    // secondary children first (the RED launch range), then the primary ones
    std::vector<int> lorder;
    for (int u : w.order)
      if (w.level[u] == l && !w.chained(u) && !w.is_primary(u)) lorder.push_back(u);
    const size_t nsec = lorder.size();
    for (int u : w.order)
      if (w.level[u] == l && !w.chained(u) && w.is_primary(u)) lorder.push_back(u);
    for (size_t q = 0; q < lorder.size(); ++q) {
      const int u = lorder[q];
      if (q == nsec) p.lv[l].ntile = (int)tiles.size() - p.lv[l].tile0;
      const int v = w.par[u];
      const int m = w.stage_len(u);
      // child class of each staging position: non-decreasing by construction
      std::vector<int> kpos(m);
      const bool u_is_y = w.ch2[v] == u;
      const bool u_primary = w.is_primary(u);
      if (w.chain_ext[u]) {  // the top classes in the chain's staging order
        const int i = w.in_chain[v], c = u_is_y ? 2 : 1;
        for (int kt = 0; kt < ntop; ++kt) kpos[w.CT(p, 2 + c, i, kt)] = w.CT(p, c, i, kt);
      } else {
        for (int q = 0; q < m; ++q) {
          const int k = u_is_y ? w.kids[v][q].y : w.kids[v][q].x;
          const int pos = u_primary ? q : w.secp[v][q];
          kpos[pos] = k;
        }
      }
      const int nt = (m + WAVE - 1) / WAVE;
      const int gt0 = (int)tiles.size();
      tile_first[u] = gt0;
      for (int t = 0; t < nt; ++t) {
        CTile tl;
        tl.node = u;
        tl.t = t;
        unsigned long long hm = 0;
        for (int l2 = 0; l2 < WAVE; ++l2) {
          const int pos = t * WAVE + l2;
          if (pos < m && (pos == 0 || kpos[pos] != kpos[pos - 1])) hm |= 1ull << l2;
        }
        tl.lo = (unsigned)(hm & 0xffffffffu);
        tl.hi = (unsigned)(hm >> 32);
        tl.kfirst = kpos[t * WAVE];
        tl.flags = 0;
        if (t > 0 && kpos[t * WAVE] == kpos[t * WAVE - 1]) tl.flags |= 1;
        const int lastpos = std::min(m, (t + 1) * WAVE) - 1;
        if (lastpos + 1 < m && kpos[lastpos + 1] == kpos[lastpos]) tl.flags |= 2;
        tl.m = m;
        tl.sb = u_primary ? -1 : w.sin[u] + t * WAVE;
        tiles.push_back(tl);
      }
      // spans: segments whose first and last positions lie in different tiles
      int q0 = 0;
      while (q0 < m) {
        int q1 = q0;
        while (q1 + 1 < m && kpos[q1 + 1] == kpos[q0]) ++q1;
        const int t0 = q0 / WAVE, t1 = q1 / WAVE;
        if (t0 != t1) w.node_spans[u].push_back(CSpan{u, kpos[q0], gt0 + t0, gt0 + t1});
        q0 = q1 + 1;
      }
      // every child class must own exactly one segment
      int segs = 0;
      for (int q = 0; q < m; ++q) segs += (q == 0 || kpos[q] != kpos[q - 1]);
      if (segs != w.ncls[u] || kpos[m - 1] != w.ncls[u] - 1)
        return fail(PHY_EINVAL, "internal: class segments of node " + std::to_string(u) + " do not cover it");
    }
    if (nsec == lorder.size()) p.lv[l].ntile = (int)tiles.size() - p.lv[l].tile0;  // no primary child here
  }
  p.ntiles = std::max((int)tiles.size(), 1);
  for (int v = S; v < N; ++v) {  // the parent's reverse reduces its primary child's tiles
    const int pc = w.prim_is_y[v] ? w.ch2[v] : w.ch1[v];
    if (pc >= S) p.nodes[v].ptile = tile_first[pc];
  }
  return PHY_OK;
}

// ---- chunks per level: 64 classes of one node each; the level's spans.  Then
// the index identities the level launches rely on: chunk i's lane l owns slot
// 64 i + l, and a RED range's tiles are consecutive staging tiles
int plan_chunks_spans(ClassPlan& p, ClassWork& w) {
  const int L = w.L;
  for (int l = 1; l < L; ++l) {
    p.lv[l].chunk0 = (int)w.chunks.size();
    p.lv[l].span0 = (int)p.spans.size();
    for (int v : w.order) {
      if (w.level[v] != l) continue;
      for (const CSpan& sp : w.node_spans[v]) p.spans.push_back(sp);
      for (int j0 = 0, ci = 0; j0 < w.ncls[v]; j0 += WAVE, ++ci) {
        CChunk cc;
        cc.node = v;
        cc.j0 = j0;
        cc.jn = std::min(WAVE, w.ncls[v] - j0);
        cc.ci = ci;
        cc.pad0 = cc.pad1 = cc.pad2 = cc.pad3 = 0;
        w.chunks.push_back(cc);
      }
    }
    p.lv[l].nchunk = (int)w.chunks.size() - p.lv[l].chunk0;
    p.lv[l].nspan = (int)p.spans.size() - p.lv[l].span0;
  }
  p.nspans = (int)p.spans.size();
  for (size_t i = 0; i < w.chunks.size(); ++i)
    if ((long long)w.off[w.chunks[i].node] + w.chunks[i].j0 != (long long)WAVE * (long long)i)
      return fail(PHY_EINVAL, "internal: class slots are not chunk-major");
  for (int l = 1; l < L; ++l) {
    ClassLevel& L1 = p.lv[l];
    L1.sec0 = L1.ntile ? p.tiles[L1.tile0].sb / WAVE : 0;
    for (int g = L1.tile0; g < L1.tile0 + L1.ntile; ++g)
      if (p.tiles[g].sb != (L1.sec0 + g - L1.tile0) * WAVE) return fail(PHY_EINVAL, "internal: staging is not tile-major");
  }
  return PHY_OK;
}

// ---- clade table: each clade's ranges at each fused level
int plan_clade_table(ClassPlan& p, ClassWork& w) {
  const int Lc = p.Lc, nclade = p.nclade;
  p.clade.assign((size_t)std::max(nclade, 1) * std::max(Lc, 1), CladeLevel{0, 0, 0, 0, 0, 0, 0, 0});
  if (Lc <= 0) return PHY_OK;
  std::vector<char> seen((size_t)nclade * Lc * 3, 0);
  auto note = [&](int k, int l, int which, int idx) {  // which: 0 chunk, 1 tile, 2 span
    CladeLevel& c = p.clade[(size_t)k * Lc + (l - 1)];
    char& f = seen[((size_t)k * Lc + (l - 1)) * 3 + which];
    int* first = which == 0 ? &c.chunk0 : which == 1 ? &c.tile0 : &c.span0;
    int* cnt = which == 0 ? &c.nchunk : which == 1 ? &c.ntile : &c.nspan;
    if (!f) {
      f = 1;
      *first = idx;
    }
    if (*first + *cnt != idx) return false;  // not contiguous
    ++*cnt;
    return true;
  };
  bool ok = true;
  auto croot = [&](int u) { return w.level[w.par[u]] > Lc; };
  for (int l = 1; l <= Lc && ok; ++l) {
    const ClassLevel& L1 = p.lv[l];
    for (int i = L1.chunk0; i < L1.chunk0 + L1.nchunk && ok; ++i) ok = note(w.cid[w.chunks[i].node], l, 0, i);
    for (int i = L1.tile0; i < L1.tile0 + L1.ntile && ok; ++i) {
      if (croot(p.tiles[i].node)) p.rtile.push_back(i);
      else ok = note(w.cid[p.tiles[i].node], l, 1, i);
    }
    for (int i = L1.span0; i < L1.span0 + L1.nspan && ok; ++i) {
      if (croot(p.spans[i].node)) p.rspan.push_back(i);
      else ok = note(w.cid[p.spans[i].node], l, 2, i);
    }
  }
  if (!ok) return fail(PHY_EINVAL, "internal: clade work is not contiguous");
  return PHY_OK;
}

// ---- tile-crossing segments: short ones (<= SPAN_LANE_MAX tiles past the
// first) of nodes the level-wide REV launches or the clade kernels' REV
// phase reverse -- not clade-internal nodes, whose spans the clade kernel's
// FIX phase sums -- are summed by their class's REV lane; the long ones by
// a FIX launch per level (index list) or the clade roots' FIX list
void plan_short_long_spans(ClassPlan& p, ClassWork& w) {
  const int Lc = p.Lc;
  p.sspan.assign((size_t)w.cls_slots, CPair{0, 0});
  auto lane_ok = [&](int u) { return w.level[u] > Lc || w.level[w.par[u]] > Lc; };  // not clade-internal
  auto is_short = [&](const CSpan& sp) { return sp.t1 - sp.t0 <= SPAN_LANE_MAX; };
  for (const CSpan& sp : p.spans)
    if (lane_ok(sp.node) && is_short(sp)) {
      p.sspan[(size_t)w.off[sp.node] + sp.k] = CPair{sp.t0, sp.t1 - sp.t0};
      ++p.lane_spans;
    }
  for (int l = Lc + 1; l < w.L; ++l) {
    ClassLevel& L1 = p.lv[l];
    L1.lfix0 = (int)p.lfix.size();
    for (int i = L1.span0; i < L1.span0 + L1.nspan; ++i)
      if (!is_short(p.spans[i])) p.lfix.push_back(i);
    L1.nlfix = (int)p.lfix.size() - L1.lfix0;
  }
  std::vector<int> rlong;
  for (int i : p.rspan)
    if (!is_short(p.spans[i])) rlong.push_back(i);
  p.rspan.swap(rlong);
  p.long_spans = (long long)p.lfix.size() + (long long)p.rspan.size();
}

// ---- forward level pairs (cls_fwd2_kernel): levels l and l + 1 -- above
// the clades, below the chain -- as one launch, the upper level recomputing
// its level-l children from their children (classes per slot in gc).
// Measured on one box (synthetic 200k, 100 evaluations): shard of 8 4,773
// evals/s unpaired, 4,965 paired; one GPU 1,794 -> 1,825 -- a pair saves a
// launch and its drain, the recomputed children cost one more gather per
// upper slot; a cap on the upper level's classes (PHY_PAIR_MAX, default
// none) measured no better at 65,536.  PHY_PAIR=0: none.
void plan_pairs(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs) {
  const int S = w.S, N = w.N, L = w.L, Lc = p.Lc;
  const long long pmax = prefs.pair_max;
  const int ltop = w.cm ? w.level[w.chn[0]] : L;  // the first level the FWD level loop does not launch
  std::vector<long long> lcls(L + 1, 0);
  for (int v = S; v < N; ++v)
    if (v != w.root) lcls[w.level[v]] += w.ncls[v];
  if (prefs.pair)
    for (int l = Lc + 1; l + 1 < ltop;) {
      if (p.lv[l].nchunk && p.lv[l + 1].nchunk && lcls[l + 1] <= pmax) {
        p.lv[l].pair = 1;
        p.lv[l + 1].pair = 2;
        ++p.npairs;
        l += 2;
      } else {
        ++l;
      }
    }
  if (!p.npairs) return;
  p.pair.assign(w.chunks.size(), CPair{-1, -1});
  p.gc.assign(w.chunks.size() * WAVE, CQuad{0, 0, 0, 0});
  for (int l = Lc + 2; l < L; ++l) {
    if (p.lv[l].pair != 2) continue;
    for (int ci = p.lv[l].chunk0; ci < p.lv[l].chunk0 + p.lv[l].nchunk; ++ci) {
      const int v = w.chunks[ci].node, x = w.ch1[v], y = w.ch2[v];
      const int rx = x >= S && w.level[x] == l - 1 ? x : -1, ry = y >= S && w.level[y] == l - 1 ? y : -1;
      p.pair[ci] = CPair{rx, ry};
      for (int j = 0; j < w.chunks[ci].jn; ++j) {
        const int q = w.chunks[ci].j0 + j;
        CQuad& g = p.gc[(size_t)ci * WAVE + j];
        if (rx >= 0) {
          const CPair kc = w.kids[rx][w.kids[v][q].x];
          g.x = kc.x;
          g.y = kc.y;
        }
        if (ry >= 0) {
          const CPair kc = w.kids[ry][w.kids[v][q].y];
          g.z = kc.x;
          g.w = kc.y;
        }
      }
    }
  }
}

// ---- long spans summed by their REV chunk (PHY_REVFIX, default on): the
// levels between the clades and the chain, whose FIX launch then goes
void plan_revfix(ClassPlan& p, ClassWork& w, const ClassPrefs& prefs) {
  const int ltop = w.cm ? w.level[w.chn[0]] : w.L;
  if (!prefs.revfix) return;
  std::vector<std::pair<int, int>> cs;  // (chunk, span)
  for (int l = p.Lc + 1; l < ltop; ++l) {
    ClassLevel& L1 = p.lv[l];
    if (!L1.nlfix) continue;
    L1.revfix = 1;
    for (int i = L1.lfix0; i < L1.lfix0 + L1.nlfix; ++i) {
      const CSpan& sp = p.spans[p.lfix[i]];
      cs.emplace_back((w.off[sp.node] + sp.k) / WAVE, p.lfix[i]);  // chunk-major slots
    }
  }
  if (cs.empty()) return;
  std::stable_sort(cs.begin(), cs.end(), [](const std::pair<int, int>& u, const std::pair<int, int>& x) {
    return u.first < x.first;
  });
  p.clf.assign(w.chunks.size(), CPair{0, 0});
  for (const auto& q : cs) {
    if (p.clf[q.first].y == 0) p.clf[q.first].x = (int)p.clong.size();
    p.clong.push_back(q.second);
    p.clf[q.first].y++;
  }
  p.nclong = (int)p.clong.size();
}

// ---- flat per-slot arrays, the staging permutation, the root weights, the
// chunks with their nodes inlined
void plan_flat(ClassPlan& p, ClassWork& w, const double* weights) {
  const int S = w.S, N = w.N;
  p.cls.assign((size_t)w.cls_slots * 2, 0);
  p.secpos.assign((size_t)w.cls_slots, 0);
  for (int v = S; v < N; ++v) {
    for (int q = 0; q < w.ncls[v]; ++q) {
      p.cls[2 * ((size_t)w.off[v] + q)] = w.kids[v][q].x;
      p.cls[2 * ((size_t)w.off[v] + q) + 1] = w.kids[v][q].y;
      p.secpos[(size_t)w.off[v] + q] = w.secp[v][q];
    }
  }
  // staging permutation of the sord levels (red_tile): position p of a
  // secondary child written in its parent's class order reads entry stperm[p];
  // the identity elsewhere (the other nodes of such a level, padding)
  p.stperm.assign((size_t)p.nstage, 0);
  for (size_t q = 0; q < p.stperm.size(); ++q) p.stperm[q] = (int)q;
  for (int u = S; u < N; ++u) {
    if (!w.sord_of(p, u)) continue;
    const int v = w.par[u], m = w.stage_len(u);
    for (int q = 0; q < m; ++q) p.stperm[(size_t)w.sin[u] + w.secp[v][q]] = w.sin[u] + q;
  }
  p.wroot.assign(w.ncls[w.root], 0.0);
  for (int i = 0; i < w.P; ++i) p.wroot[p.pat_root[i]] += weights[i];
  p.chunks.resize(w.chunks.size());
  for (size_t i = 0; i < w.chunks.size(); ++i) {
    p.chunks[i].nd = p.nodes[w.chunks[i].node];
    p.chunks[i].j0 = w.chunks[i].j0;
    p.chunks[i].jn = w.chunks[i].jn;
    p.chunks[i].ci = w.chunks[i].ci;
    p.chunks[i].node = w.chunks[i].node;
  }
}

// ---- the chain's links (its tables: plan_chain, plan_tiles)
void plan_chain_links(ClassPlan& p, ClassWork& w) {
  const int S = w.S, cm = w.cm;
  if (!cm) return;
  p.links.resize(cm);
  for (int i = 0; i < cm; ++i) {
    const int v = w.chn[i];
    const CNode& nd = p.nodes[v];
    CLink& lk = p.links[i];
    std::memset(&lk, 0xff, sizeof(lk));
    lk.off = w.off[v];
    lk.mv = nd.mv;
    lk.spine = i == 0 ? -1 : (w.ch1[v] == w.chn[i - 1] ? 0 : 1);
    lk.offx = nd.offx;
    lk.offy = nd.offy;
    lk.mx = nd.mx;
    lk.my = nd.my;
    lk.gv = nd.gv;
    lk.gx = nd.gx;
    lk.gy = nd.gy;
    lk.stx = (w.ch1[v] >= S && w.chain_ext[w.ch1[v]]) ? w.sin[w.ch1[v]] : -1;
    lk.sty = (w.ch2[v] >= S && w.chain_ext[w.ch2[v]]) ? w.sin[w.ch2[v]] : -1;
  }
  p.chain_m = cm;
  p.chain_lo = w.level[w.chn[0]];
  p.chain_hi = w.level[w.ctop];
  p.chain_ntop = w.ntop;
  p.chain_ntp = w.ntp;
  p.chain_toff = w.off[w.ctop];
}

// ---- branches whose partial rows take cls_epi_kernel more than GSUB_MIN / 512 rounds of loads
void plan_gsub(ClassPlan& p) {
  p.pbase.assign(p.B, -1);
  for (int b = 0; b < p.B; ++b) {
    if (p.gcount[b] <= GSUB_MIN) continue;
    p.pbase[b] = (int)p.gsub.size();
    for (int r = 0; r < p.gcount[b]; r += GSUB_ROWS)
      p.gsub.push_back(CPair{p.gbase[b] + r, std::min(GSUB_ROWS, p.gcount[b] - r)});
  }
  p.nsub = (int)p.gsub.size();
}

// Build the class plan.  vec_of: tip code -> record index; gpos: branch ->
// matrix record index (make_problem's).  Returns PHY_OK or a PHY_E* code.
int class_plan(int S, int P, int C, int rooted, const uint8_t* tipcodes, const double* weights, const int32_t* peel,
               const std::vector<int>& vec_of, int R, int nmat, const std::vector<int>& gpos, const ClassPrefs& prefs,
               ClassPlan& p) {
  p = ClassPlan();
  ClassWork w;
  const int N = w.N = 2 * S - 1;
  w.S = S;
  w.P = P;
  w.peel = peel;
  w.root = peel[3 * (S - 2) + 2];
  w.merged = rooted ? -1 : peel[3 * (S - 2) + 1];
  w.ch1.assign(N, -1);
  w.ch2.assign(N, -1);
  w.par.assign(N, -1);
  w.level.assign(N, 0);
  for (int r = 0; r < S - 1; ++r) {
    const int x = peel[3 * r], y = peel[3 * r + 1], v = peel[3 * r + 2];
    w.ch1[v] = x;
    w.ch2[v] = y;
    w.par[x] = w.par[y] = v;
    w.level[v] = 1 + std::max(w.level[x], w.level[y]);
  }
  w.L = w.level[w.root];
  p.S = S;
  p.P = P;
  p.C = C;
  p.R = R;
  p.nmat = nmat;
  p.B = rooted ? 2 * S - 2 : 2 * S - 3;
  p.root = w.root;
  p.levels = w.L;
  p.root_chain_pref = prefs.root_chain ? 1 : 0;
  int rc;
  plan_classes(p, w, tipcodes, vec_of);
  plan_clades(p, w, prefs);
  plan_chain(p, w, prefs);
  plan_layout(p, w, prefs);
  if ((rc = plan_nodes(p, w, prefs, gpos))) return rc;
  if ((rc = plan_tiles(p, w))) return rc;
  if ((rc = plan_chunks_spans(p, w))) return rc;
  if ((rc = plan_clade_table(p, w))) return rc;
  plan_short_long_spans(p, w);
  plan_pairs(p, w, prefs);
  plan_revfix(p, w, prefs);
  plan_flat(p, w, weights);
  plan_chain_links(p, w);
  plan_gsub(p);
  p.nrtile = (int)p.rtile.size();
  p.nrspan = (int)p.rspan.size();
  return PHY_OK;
}

// The uploaded tables, in upload order (phy_plan_class's digests; a chain-free
// plan uploads no chain table)
struct ClassTable {
  const char* name;
  const void* data;
  size_t bytes;
};
std::vector<ClassTable> class_plan_tables(const ClassPlan& p) {
  auto t = [](const char* name, const auto& v, bool on = true) {
    return ClassTable{name, v.data(), on ? v.size() * sizeof(v[0]) : 0};
  };
  const bool ch = p.chain_m > 0;
  return {t("links", p.links, ch), t("ctab", p.ctab, ch), t("crep", p.crep, ch), t("nodes", p.nodes),
          t("chunks", p.chunks), t("cls", p.cls), t("secpos", p.secpos), t("stperm", p.stperm), t("tiles", p.tiles),
          t("spans", p.spans), t("wroot", p.wroot), t("pat_root", p.pat_root), t("gbase", p.gbase),
          t("gcount", p.gcount), t("gsub", p.gsub), t("pbase", p.pbase), t("clade", p.clade), t("rtile", p.rtile),
          t("rspan", p.rspan), t("lfix", p.lfix), t("sspan", p.sspan), t("pair", p.pair), t("clf", p.clf),
          t("clong", p.clong), t("gc", p.gc)};
}

}  // namespace
#endif  // PHYLO_CLASS_PLAN_H
