// sweep_plan.h -- the host planner of the pattern sweep: everything that
// turns a tree, its tip data and the tuning preferences into the programs,
// records, LDS plan and launch choice the kernels of phylo_hip.hip run.
//
// Plain C++17: no HIP header, no device code, no device memory.  phylo_hip.hip
// includes it (one translation unit, hence the anonymous namespace) and
// uploads what it plans; tests/plan_host_check.cpp compiles it with a host
// compiler alone.  PHY_HD marks the few layout helpers the kernels share.
#ifndef PHYLO_SWEEP_PLAN_H
#define PHYLO_SWEEP_PLAN_H

#include <algorithm>
#include <climits>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "phylo_hip_diag.h"

#if defined(__HIPCC__)
#define PHY_HD __host__ __device__
#else
#define PHY_HD
#endif

namespace {

constexpr int WAVE = 64;
// Program step (STEP_INTS ints, host-built by build_program).
constexpr int STEP_INTS = 16;
enum {
  ST_X = 0,  // child x: tip index >= 0, or -1 (internal)
  ST_Y,      // child y: same
  ST_MX,     // matrix of a tip x (its branch), -1 otherwise
  ST_MY,     // matrix of a tip y
  ST_MV,     // matrix of the step's own branch (-1: root / merged branch)
  ST_VSLOT,  // scratch slot of a_v (-1 at the root)
  ST_FLAGS,  // F_* below
  ST_XSLOT,  // scratch slot of an internal x
  ST_YSLOT,  // scratch slot of an internal y
  ST_XDPOS,  // deep-stack entry of x when both children are internal
  ST_VDPOS,  // deep-stack entry of v when F_VDEEP
  ST_CHUNK,  // LDS chunk holding the step's matrices
  ST_M0,     // first matrix of that chunk
  ST_MN,     // matrices in that chunk
  ST_NODE,   // node id
  ST_RD,     // rebuild depth of the previous-step child (F_PREVREC): 1 cherry, 2.. chain
};
constexpr int F_MV = 1;     // the step's branch has a matrix (else identity)
constexpr int F_XDEEP = 2;  // both children internal: x's operand is on the deep stack
constexpr int F_VDEEP = 4;  // v is the x child of a both-internal parent
// Recomputed cherries (set per LDS plan, plan_lds): a node whose children
// are both tips is not stored when it is the previous step of its parent and
// shares the parent's LDS chunk -- the parent's reverse step rebuilds it from
// the tips and matrices already in LDS (its step record is the one the
// reverse loaded a step ahead).
constexpr int F_NOSTORE = 8;   // this step's a_v is not written to scratch
constexpr int F_PREVREC = 16;  // the child computed at the previous step is rebuilt, not loaded
#ifndef PHY_RD_MAX
#define PHY_RD_MAX 4
#endif
constexpr int RD_MAX = PHY_RD_MAX;  // deepest rebuild chain: a cherry plus up to RD_MAX-1 one-tip nodes above it
// Rescaled sweep: largest power of two by which a category whose root term is
// exactly zero may pre-scale its upper partials (sweep_kernel's root)
constexpr int RS_DMAX = 900;
// Clade compression of the batched sweep (plan_clades below): limits and the host plan.
constexpr int CC_MAXCL = 8;    // clades per context (they share the class block)
constexpr int CC_COLS = 128;   // columns of the class block: one K = 2 block
constexpr int CC_MININT = 3;   // internal nodes of the smallest clade taken
constexpr int CC_ROUNDS_U = 8; // aggregation rounds in flight
constexpr int CC_HDR = 4 * CC_MAXCL;  // ints of the device table's header (lo, hi per clade)

// The device copy of the program packs a step into 8 ints (pack_program):
//   w0 x | y<<16   w1 mx | my<<16   w2 mv | vslot<<16   w3 xslot | yslot<<16
//   w4 flags | xdpos<<8 | vdpos<<16 (8-bit fields)      w5 chunk | m0<<16
//   w6 mn | node<<16                                    w7 unused
// 16-bit fields are signed (-1 = none).  One s_load_dwordx8 per step, issued
// a step ahead, replaces a chain of dependent scalar loads.
constexpr int PSTEP = 8;
// The two-column kernel (K = 2, the batched throughput plan) reads 16-int
// steps (one s_load_dwordx16, no field extraction): measured 6.07-6.09
// against 6.14 ms per fluA launch; the one-column latency kernel keeps the
// packed form (64-draw calls 181 against 191 us with unpacked records) and
// derives the fields below when it loads a step.
//
// The 16 ints are the batched record (batched_records, built per plan from
// the 16-int program): every index the kernel would scale is stored as the
// byte offset it adds, and "operand not loaded" is decided on the host
// (fluA 6.07 -> 5.94 ms per launch with the slot masks and the nibble
// extract below).
enum {
  BR_X = 0,  // tip x: byte offset of its nibble row in the block's tips (x * K * 32); -1 internal
  BR_Y,      // tip y: same
  BR_MXO,    // LDS byte offset of x's matrix record inside the wave's chunk ((mx - m0) * R * 32)
  BR_MYO,    // of y's
  BR_MVO,    // of the step's own
  BR_VSO,    // scratch byte offset of a_v (vslot * entry stride); -1 at the root
  BR_FLRD,   // F_* flags | rebuild depth << 8
  BR_XSO,    // scratch byte offset the reverse loads a_x from; OOB when it loads none
  BR_YSO,    // the same for a_y
  BR_XDPOS,  // deep-stack entries, as in the program
  BR_VDPOS,
  BR_GX,     // dL/dP slot byte offsets (m * 128) of mx, my, mv
  BR_M0,     // first matrix and matrix count of the step's chunk (staging)
  BR_MN,
  BR_GY,
  BR_GV,
};
constexpr int USTEP = STEP_INTS;
constexpr uint32_t OOB = 0x40000000u;  // out-of-range offset part (regions are < 2^30 bytes, checked at plan time)
// Per-draw eigensystem record: P(t) = m1 diag(exp(lam t)) m2, plus Q.
constexpr int EIG_LEN = 56;  // m1[16] lam[4] m2[16] Q[16] s (+pad)
constexpr int EIG_M1 = 0, EIG_LAM = 16, EIG_M2 = 20, EIG_Q = 36, EIG_S = 52;

// LDS doubles of the Q-parameter chain rule (qgrad_body) and the split
// epilogue's shape (qfin_kernel): the launch choice tests their room.
constexpr int QG_THREADS = 1024;  // 256 (c, b) quads per pass (the synthetic config: 1016 in 4 passes, not 16)
constexpr int QG_SHARED = 16 * 3 + 4 + (QG_THREADS / 64) * 16 + 16 * 2;  // V, V^-1, 1/(lam_k - lam_l), lam,
                                                                          // wave partials, M, W
constexpr int QFIN_THREADS = 256;
constexpr int QFIN_ITEMS = QFIN_THREADS / 4;  // (c, b) items per workgroup
constexpr int QFIN_SLOTS = 16;                // workgroup slots per draw it takes

constexpr size_t LDS_CAP = 160 * 1024;
constexpr int MIN_CAP = 24;  // an occupancy level is taken only if chunks stay this large
#ifndef PHY_WPE2
#define PHY_WPE2 2  // waves per SIMD the K=2 kernel is register-budgeted for
#endif

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// LDS carve (16-B aligned pieces), K columns per lane:
//   tips   S x 64K nibbles            record indices, shared by the C category waves
//   mats   C x cap_m x R x 4 doubles  wave c's chunk of matrix records
//   tail   per wave: ndl deep entries of K x 2 x 64 double2 (the deep
//          entries [0, ndl) kept in LDS), or K x 64 doubles when ndl = 0;
//          wave c's root-exchange slice (K x 64 doubles) sits at the start
//          of its own tail, whose deep entries are all free at the root
// tips: the block's nibbles, then the 0/1 state vectors of the 16 record
// indices (the t of dL/dP += r (x) t for a tip child: two LDS reads instead
// of unpacking and converting its mask bits per column)
PHY_HD inline size_t tip_nib_bytes(int S, int K) { return ((size_t)S * WAVE * K / 2 + 15) / 16 * 16; }
PHY_HD inline size_t tip_lds_bytes(int S, int K) { return tip_nib_bytes(S, K) + 16 * 4 * sizeof(double); }
PHY_HD inline size_t tail_doubles(int K, int ndl) {  // per wave
  return ndl > 0 ? (size_t)ndl * K * 2 * WAVE * 2 : (size_t)K * WAVE;
}
PHY_HD inline size_t lds_bytes(int S, int C, int R, int cap_m, int K, int ndl) {
  return tip_nib_bytes(S, K) + 16 * 4 * sizeof(double) + (size_t)C * cap_m * R * 32 +
         (size_t)C * tail_doubles(K, ndl) * 8;
}

inline int nblk_for(int P, int K) { return (P + WAVE * K - 1) / (WAVE * K); }
// The sweep's register budget per plan: K = 1 has two, four waves per SIMD
// (1,024-thread workgroups, 128 VGPRs: spills) for wide launches with C > 8,
// and the sampler's latency plan (a few draws: at most one wave per SIMD is
// busy) at 256 VGPRs without spills (lat).
inline int waves_per_simd(int K, bool lat) { return (K == 2 || lat) ? PHY_WPE2 : 4; }

// Build the traversal program (DESIGN.md "Traversal program"): post-order
// with the child needing the deeper stack first (Strahler order), every
// stored moved partial in a slot (its step index), every branch matrix
// numbered in order of use, and the deep-stack entries.
//
// In this post-order the node computed just before v is v's second child y
// when y is internal, else its first child x when x is internal.  So a step
// pops `top` (the previous step's result) for y, and for x when y is a tip;
// only the first child x of a node whose children are both internal waits
// while y's subtree runs.  Those waits nest, so they live on a stack whose
// entry per wait is fixed here (ST_XDPOS / ST_VDPOS), used by both passes.
// Device layout of the program (see Step / ld_step): 8 packed ints per step.
std::vector<int> pack_program(const std::vector<int>& prog) {
  const size_t n = prog.size() / STEP_INTS;
  std::vector<int> out(n * PSTEP, 0);
  auto h = [](int lo, int hi) { return (int)(((unsigned)(lo & 0xFFFF)) | ((unsigned)hi << 16)); };
  for (size_t s = 0; s < n; ++s) {
    const int* p = &prog[s * STEP_INTS];
    int* q = &out[s * PSTEP];
    q[0] = h(p[ST_X], p[ST_Y]);
    q[1] = h(p[ST_MX], p[ST_MY]);
    q[2] = h(p[ST_MV], p[ST_VSLOT]);
    q[3] = h(p[ST_XSLOT], p[ST_YSLOT]);
    q[4] = (int)((unsigned)(p[ST_FLAGS] & 0xFF) | ((unsigned)(p[ST_XDPOS] & 0xFF) << 8) |
                 ((unsigned)(p[ST_VDPOS] & 0xFF) << 16));
    q[5] = h(p[ST_CHUNK], p[ST_M0]);
    q[6] = h(p[ST_MN], p[ST_NODE]);
    q[7] = p[ST_RD];
  }
  return out;
}

// The batched (two-column) kernel's records (BR_*) of a planned program: the
// offsets depend on the column plan (K, C: the scratch entry stride), on R
// and on the chunk plan (ST_M0) and its rebuilt chains (F_PREVREC), so they
// are rebuilt with every plan.  ld_step's packed branch derives the same
// values on the device for the one-column kernel.
// plane0 >= 0 (a compressed plan, plan_clades): the first r-plane entry;
// a gathered child (ST_X / ST_Y <= -2) keeps its clade code and carries its r
// plane's offset where a tip child has its dL/dP slot.
std::vector<int> batched_records(const std::vector<int>& prog, int K, int C, int R, int plane0 = -1, int nblk = 0) {
  const size_t n = prog.size() / STEP_INTS;
  std::vector<int> out(n * USTEP, 0);
  const uint32_t estr = (uint32_t)(K * 2 * C * WAVE * 16);
  const int rec8 = R * 32;
  for (size_t s = 0; s < n; ++s) {
    const int* p = &prog[s * STEP_INTS];
    int* q = &out[s * USTEP];
    const int x = p[ST_X], y = p[ST_Y], fl = p[ST_FLAGS];
    const bool rec = fl & F_PREVREC;
    q[BR_X] = x >= 0 ? x * K * (WAVE / 2) : x;
    q[BR_Y] = y >= 0 ? y * K * (WAVE / 2) : y;
    q[BR_MXO] = (p[ST_MX] - p[ST_M0]) * rec8;
    q[BR_MYO] = (p[ST_MY] - p[ST_M0]) * rec8;
    q[BR_MVO] = (p[ST_MV] - p[ST_M0]) * rec8;
    q[BR_VSO] = p[ST_VSLOT] >= 0 ? (int)((uint32_t)p[ST_VSLOT] * estr) : -1;
    q[BR_FLRD] = fl | (p[ST_RD] << 8);
    q[BR_XSO] = (int)((x < 0 && !(rec && y >= 0)) ? (uint32_t)p[ST_XSLOT] * estr : OOB);
    q[BR_YSO] = (int)((y < 0 && !rec) ? (uint32_t)p[ST_YSLOT] * estr : OOB);
    q[BR_XDPOS] = p[ST_XDPOS];
    q[BR_VDPOS] = p[ST_VDPOS];
    q[BR_GX] = p[ST_MX] * 128;
    q[BR_GY] = p[ST_MY] * 128;
    q[BR_GV] = p[ST_MV] * 128;
    q[BR_M0] = p[ST_M0];
    q[BR_MN] = p[ST_MN];
    if (plane0 >= 0 && x <= -2) q[BR_GX] = (int)((uint32_t)(plane0 + (-2 - x) * nblk) * estr);
    if (plane0 >= 0 && y <= -2) q[BR_GY] = (int)((uint32_t)(plane0 + (-2 - y) * nblk) * estr);
  }
  return out;
}

// A validated tree: children of every internal node, the root, and the
// node whose branch is merged into the root's (unrooted trees; -1 rooted).
struct PeelTree {
  int S = 0, root = -1, merged = -1;
  std::vector<int> ch1, ch2;
};

int parse_peel(int S, const int32_t* peel, int rooted, PeelTree& t) {
  const int N = 2 * S - 1;
  std::vector<int>&ch1 = t.ch1, &ch2 = t.ch2;
  ch1.assign(N, -1);
  ch2.assign(N, -1);
  std::vector<int> seen(N, 0);
  for (int r = 0; r < S - 1; ++r) {
    const int a = peel[3 * r], b = peel[3 * r + 1], v = peel[3 * r + 2];
    if (a < 0 || a >= N || b < 0 || b >= N || v < S || v >= N || a == b)
      return fail(PHY_EINVAL, "peel row " + std::to_string(r) + " out of range");
    if (ch1[v] != -1) return fail(PHY_EINVAL, "node " + std::to_string(v) + " peeled twice");
    ch1[v] = a;
    ch2[v] = b;
    seen[a]++;
    seen[b]++;
  }
  const int root = peel[3 * (S - 2) + 2];
  for (int n = 0; n < N; ++n) {
    if (n != root && seen[n] != 1)
      return fail(PHY_EINVAL, "node " + std::to_string(n) + " is not a child exactly once");
    if (n >= S && ch1[n] < 0) return fail(PHY_EINVAL, "internal node without children");
  }
  if (seen[root] != 0) return fail(PHY_EINVAL, "root listed as a child");
  int merged = -1;
  if (!rooted) {
    merged = peel[3 * (S - 2) + 1];
    if (merged != 2 * S - 3)
      return fail(PHY_EINVAL,
                  "unrooted peel: last row child2 must be node 2S-3 (phylostan.py:264-267)");
    if (merged < S) return fail(PHY_EINVAL, "unrooted peel: node 2S-3 must be internal");
  }
  t.S = S;
  t.root = root;
  t.merged = merged;
  return PHY_OK;
}

// Append the steps of the subtree under `sub` to prog (and its matrices, in
// order of use, to mat_branch).  gath[n] >= 0 marks an internal node that is
// a leaf of this program: the root of compressed clade gath[n], whose moved
// partial was stored by its own program (slot[n]) and is gathered per pattern
// column (ST_X / ST_Y = -2 - clade; no matrix here: its branch belongs to
// the clade's program).  A node's slot is its step index in prog.  A sub-root
// other than the tree's root is stored like any other node and takes its
// upper partial from `top`.
int emit_steps(const PeelTree& t, int sub, const std::vector<int>& gath, std::vector<int>& prog,
               std::vector<int>& mat_branch, std::vector<int>& slot, int& ndeep) {
  const int S = t.S, N = 2 * S - 1, root = t.root, merged = t.merged;
  const std::vector<int>&ch1 = t.ch1, &ch2 = t.ch2;
  auto leaf = [&](int n) { return n < S || (n != sub && gath[n] >= 0); };
  // deep-stack need per subtree; larger-need child first (Strahler order)
  std::vector<int> need(N, 0), first(N, -1), second(N, -1);
  {
    std::vector<int> order;  // post-order of the rooted tree
    std::vector<std::pair<int, int>> st{{sub, 0}};
    while (!st.empty()) {
      auto& [n, k] = st.back();
      if (leaf(n) || k == 2) {
        order.push_back(n);
        st.pop_back();
        continue;
      }
      const int child = (k == 0) ? ch1[n] : ch2[n];
      ++k;
      st.push_back({child, 0});
    }
    for (int n : order) {
      if (leaf(n)) continue;
      const int a = ch1[n], b = ch2[n];
      auto hold = [&](int m) { return !leaf(m) ? 1 : 0; };
      const int ab = std::max({need[a], hold(a) + need[b], 1});
      const int ba = std::max({need[b], hold(b) + need[a], 1});
      if (ba < ab) {
        first[n] = b;
        second[n] = a;
        need[n] = ba;
      } else {
        first[n] = a;
        second[n] = b;
        need[n] = ab;
      }
    }
  }
  std::vector<int> steps;
  {
    std::vector<std::pair<int, int>> st{{sub, 0}};
    while (!st.empty()) {
      auto& [n, k] = st.back();
      if (leaf(n)) {
        st.pop_back();
        continue;
      }
      if (k == 2) {
        steps.push_back(n);
        st.pop_back();
        continue;
      }
      const int child = (k == 0) ? first[n] : second[n];
      ++k;
      st.push_back({child, 0});
    }
  }
  const int ns = (int)steps.size();
  const int s0 = (int)(prog.size() / STEP_INTS);
  std::vector<int> parent(N, -1);
  for (int s = 0; s < ns; ++s) {
    if (steps[s] != root) slot[steps[s]] = s0 + s;
    parent[first[steps[s]]] = parent[second[steps[s]]] = steps[s];
  }
  prog.resize((size_t)(s0 + ns) * STEP_INTS, -1);
  std::vector<int> vdpos(N, -1);
  int cur = 0;
  for (int s = 0; s < ns; ++s) {
    const int v = steps[s];
    const int x = first[v], y = second[v];
    int* p = &prog[(size_t)(s0 + s) * STEP_INTS];
    p[ST_X] = x < S ? x : leaf(x) ? -2 - gath[x] : -1;
    p[ST_Y] = y < S ? y : leaf(y) ? -2 - gath[y] : -1;
    p[ST_MX] = p[ST_MY] = p[ST_MV] = -1;
    if (x < S) {  // tip children: their matrices are used at this step
      p[ST_MX] = (int)mat_branch.size();
      mat_branch.push_back(x);
    }
    if (y < S) {
      p[ST_MY] = (int)mat_branch.size();
      mat_branch.push_back(y);
    }
    int fl = 0;
    if (v != root && v != merged) {  // the step's own branch
      p[ST_MV] = (int)mat_branch.size();
      mat_branch.push_back(v);
      fl |= F_MV;
    }
    p[ST_VSLOT] = (v == root) ? -1 : slot[v];
    p[ST_XSLOT] = x >= S ? slot[x] : -1;
    p[ST_YSLOT] = y >= S ? slot[y] : -1;
    // operand sources (see the comment above), checked here
    if (!leaf(y) && (s == 0 || steps[s - 1] != y)) return fail(PHY_EINVAL, "internal: y is not the previous step");
    if (!leaf(x) && leaf(y) && (s == 0 || steps[s - 1] != x))
      return fail(PHY_EINVAL, "internal: x is not the previous step");
    if (!leaf(x) && !leaf(y)) {
      fl |= F_XDEEP;
      if (vdpos[x] != cur - 1) return fail(PHY_EINVAL, "internal: deep stack out of order");
      p[ST_XDPOS] = vdpos[x];
      --cur;
    }
    if (v != sub) {
      const int u = parent[v];
      if (first[u] == v && !leaf(second[u])) {  // waits for its sibling's subtree
        fl |= F_VDEEP;
        vdpos[v] = cur++;
        ndeep = std::max(ndeep, cur);
        p[ST_VDPOS] = vdpos[v];
      }
    }
    p[ST_FLAGS] = fl;
    p[ST_NODE] = v;
  }
  if (cur != 0) return fail(PHY_EINVAL, "internal: deep stack not empty");
  return PHY_OK;
}

int build_program(int S, const int32_t* peel, int rooted, std::vector<int>& prog,
                  std::vector<int>& mat_branch, int& nslots, int& ndeep) {
  PeelTree t;
  int rc = parse_peel(S, peel, rooted, t);
  if (rc) return rc;
  const int N = 2 * S - 1;
  std::vector<int> slot(N, -1);
  const std::vector<int> gath(N, -1);
  prog.clear();
  mat_branch.clear();
  ndeep = 0;
  rc = emit_steps(t, t.root, gath, prog, mat_branch, slot, ndeep);
  if (rc) return rc;
  if ((int)(prog.size() / STEP_INTS) != S - 1) return fail(PHY_EINVAL, "tree is not binary / connected");
  nslots = S - 2;
  return PHY_OK;
}

// The chunk plan over the program for chunks of at most `cap` matrices
// (ST_CHUNK / ST_M0 / ST_MN) and the rebuilt chains it allows.
// brk > 0: a chunk boundary is forced before step brk (a compressed plan's
// first U step), and a step with a gathered child rebuilds nothing.
int assign_chunks(std::vector<int>& prog, int nsteps, int nmat, int cap, bool recompute, int& nchunks, int& nrec,
                  int brk = -1) {
  // chunk boundaries: matrices are numbered in step order, so a chunk is a
  // run of steps whose matrices fit
  int used = 0, ch = 0, lo = 0;
  std::vector<int> first_step{0};
  for (int s = 0; s < nsteps; ++s) {
    const int* p = &prog[(size_t)s * STEP_INTS];
    const int n = (p[ST_MX] >= 0) + (p[ST_MY] >= 0) + (p[ST_MV] >= 0);
    if (used + n > cap || (s == brk && s > 0)) {
      first_step.push_back(s);
      lo += used;
      used = 0;
      ++ch;
    }
    int* q = &prog[(size_t)s * STEP_INTS];
    q[ST_CHUNK] = ch;
    q[ST_M0] = lo;
    used += n;
  }
  if (lo + used != nmat) return fail(PHY_EINVAL, "internal: chunk plan does not cover the matrices");
  first_step.push_back(nsteps);
  for (int k = 0; k <= ch; ++k) {
    const int m0 = prog[(size_t)first_step[k] * STEP_INTS + ST_M0];
    const int m1 = (k < ch) ? prog[(size_t)first_step[k + 1] * STEP_INTS + ST_M0] : nmat;
    for (int s = first_step[k]; s < first_step[k + 1]; ++s) prog[(size_t)s * STEP_INTS + ST_MN] = m1 - m0;
  }
  // rebuilt chains (F_NOSTORE / F_PREVREC / ST_RD), valid for this chunk plan:
  // step s's previous-step child q is rebuilt at depth d when q is a cherry
  // (d = 1) or has one tip child and itself rebuilds its previous-step child
  // at depth d-1, and steps s-d..s share one LDS chunk
  nrec = 0;
  for (int s = 0; s < nsteps; ++s) {
    prog[(size_t)s * STEP_INTS + ST_FLAGS] &= ~(F_NOSTORE | F_PREVREC);
    prog[(size_t)s * STEP_INTS + ST_RD] = 0;
  }
  if (recompute) {
    for (int s = 1; s < nsteps; ++s) {
      int* p = &prog[(size_t)s * STEP_INTS];
      int* q = &prog[(size_t)(s - 1) * STEP_INTS];
      const bool has_internal = p[ST_X] < 0 || p[ST_Y] < 0;  // then step s-1 is its top child
      const bool eligible = (q[ST_FLAGS] & F_MV) && q[ST_VSLOT] >= 0 && !(q[ST_FLAGS] & F_VDEEP);
      if (!has_internal || !eligible || p[ST_X] <= -2 || p[ST_Y] <= -2) continue;
      int d = 0;
      if (q[ST_X] >= 0 && q[ST_Y] >= 0) d = 1;
      else if ((q[ST_X] >= 0) != (q[ST_Y] >= 0) && q[ST_RD] > 0) d = q[ST_RD] + 1;
      if (d == 0 || d > RD_MAX || s - d < 0) continue;
      bool same = true;
      for (int j = 1; j <= d; ++j) same = same && prog[(size_t)(s - j) * STEP_INTS + ST_CHUNK] == p[ST_CHUNK];
      if (!same) continue;
      q[ST_FLAGS] |= F_NOSTORE;
      p[ST_FLAGS] |= F_PREVREC;
      p[ST_RD] = d;
      ++nrec;
    }
  }
  nchunks = ch + 1;
  return PHY_OK;
}

// ---------------------------------------------------------------------------
// Clade compression of the batched pattern sweep ("Compressed
// clades"): host planning.
//
// A clade whose tips take at most CC_COLS distinct state tuples over the
// context's patterns runs once per draw on one column per tuple (class)
// instead of once per pattern block:
//   L  the selected clades' steps, each clade in its own post-order, run on
//      the class block (one more 128-column block of tip nibbles);
//   U  the rest of the tree on the pattern blocks, with every clade root a
//      gathered leaf: its moved partial is read from the root's slot at the
//      column of the pattern's class, and its upper partial is stored to the
//      root's r plane, class by class, and summed per class before L's reverse.
// Only whole maximal clades are taken, so indirection is paid at the clade
// boundaries alone.
// ---------------------------------------------------------------------------
struct CladePlan {
  int ncl = 0;
  int node[CC_MAXCL] = {}, ncls[CC_MAXCL] = {}, maxmult[CC_MAXCL] = {}, nint[CC_MAXCL] = {};
  int lo[CC_MAXCL] = {}, hi[CC_MAXCL] = {};  // the clade's steps in L, inclusive
  int nblk = 0;                    // pattern blocks (K = 2)
  int nL = 0, nU = 0, nmat = 0, nmatL = 0, ndeep = 0, maxcls = 0;
  int rounds = 0;                  // largest maxmult, rounded up to CC_ROUNDS_U
  std::vector<int> prog;           // raw steps [L | U] (STEP_INTS each), before the chunk plan
  std::vector<int> mat_branch;     // branch of matrix m, matrices in order of use over [L | U]
  std::vector<int> cls_of;         // [ncl][nblk * CC_COLS] class of each pattern column, -1 on padding
  std::vector<int> members;        // [ncl][rounds][CC_COLS] t-th pattern of class j (ascending), -1 past its size
  std::vector<int> rep;            // [ncl][CC_COLS] first pattern of class j, -1 past the class count
  std::vector<char> in_clade;      // [2S-1] node belongs to a selected clade (root included)
  std::vector<int> clade_of_tip;   // [S] clade of a tip, -1 outside
};

// selection is attempted only for alignments this small (the plan is
// quadratic-ish host work and only one-workgroup-per-draw launches use it)
constexpr size_t CC_MAX_CELLS = (size_t)1 << 22;

// Cost model, in cycles of one category wave per draw.
// A clade saves its steps on all pattern blocks but one: forward plus reverse
// step of the two-column kernel, about 1.2 k + 3.5 k cycles (DESIGN.md 7's
// step profile).  It costs its boundary, all of it latencies of dependent
// loads that nothing hides (about 2.5 k cycles each on a full MI355X):
//   per pattern block   the class-column load and the gathered a_x in the
//                       forward, the class-column load ahead of the reverse's
//                       operand prefetch (which drains the prefetch), the
//                       position load before the r store;
//   per aggregation batch  CC_ROUNDS_U rounds of r loads in flight;
//   per clade           the run starts and class sizes, and one restart of
//                       the reverse's step and operand prefetch.
// Calibrated on one MI355X from fluA at 8,192 draws (HKY, C = 4, two blocks):
// parent 921 k cycles per draw; clades 114 + 121 826 k; 76 added 865 k, so
// node 76 (8 batches) costs 53 k against 14 k saved and 114 + 121 + the
// fixed part 102 k; HCV's five clades then come out 10 k better than the
// model says.  A clade is kept when its saving exceeds its
// cost by a quarter.
constexpr long CC_STEP_CYCLES = 4700;      // forward + reverse step of one block
constexpr long CC_BOUNDARY_CYCLES = 13000; // per pattern block and clade
constexpr long CC_BATCH_CYCLES = 2500;     // per CC_ROUNDS_U aggregation rounds
constexpr long CC_CLADE_CYCLES = 7000;     // per clade
constexpr long CC_FIXED_CYCLES = 6000;     // the class block's two passes (tip staging, root barriers)

// The clades taken for a tree and its tip data; mode 1 skips the cost model's
// per-clade and overall tests (every qualifying maximal clade is taken).
int plan_clades(const PeelTree& t, int P, const uint8_t* tipcodes, int mode, CladePlan& cp) {
  const int S = t.S, N = 2 * S - 1;
  cp = CladePlan();
  cp.nblk = (P + CC_COLS - 1) / CC_COLS;
  if (cp.nblk < 2 || (size_t)N * P > CC_MAX_CELLS) return PHY_OK;
  // post-order of the internal nodes
  std::vector<int> order;
  {
    std::vector<std::pair<int, int>> st{{t.root, 0}};
    while (!st.empty()) {
      auto& [n, k] = st.back();
      if (n < S) {
        st.pop_back();
        continue;
      }
      if (k == 2) {
        order.push_back(n);
        st.pop_back();
        continue;
      }
      const int child = (k == 0) ? t.ch1[n] : t.ch2[n];
      ++k;
      st.push_back({child, 0});
    }
  }
  // classes of every subtree: the id of (class under ch1, class under ch2),
  // numbered by first occurrence in ascending pattern order; a subtree with
  // more than CC_COLS classes is not tracked further (-1)
  std::vector<std::vector<int>> cid(N);
  std::vector<int> count(N, 0), nint(N, 0);
  auto col = [&](int n, int p) -> long { return n < S ? (long)tipcodes[(size_t)n * P + p] : (long)cid[n][p]; };
  for (int v : order) {
    const int a = t.ch1[v], b = t.ch2[v];
    nint[v] = 1 + nint[a] + nint[b];
    if ((a >= S && count[a] < 0) || (b >= S && count[b] < 0)) {
      count[v] = -1;
      continue;
    }
    std::vector<std::pair<long, int>> keys(P);
    for (int p = 0; p < P; ++p) keys[p] = {col(a, p) * 65536 + col(b, p), p};
    std::vector<std::pair<long, int>> sorted = keys;
    std::sort(sorted.begin(), sorted.end());
    // first pattern of every distinct key, then ids in order of that pattern
    std::vector<int> firstp;
    for (int i = 0; i < P; ++i)
      if (i == 0 || sorted[i].first != sorted[i - 1].first) firstp.push_back(sorted[i].second);
    if ((int)firstp.size() > CC_COLS) {
      count[v] = -1;
      continue;
    }
    std::sort(firstp.begin(), firstp.end());
    std::vector<int> idof(P, -1);
    for (int j = 0; j < (int)firstp.size(); ++j) idof[firstp[j]] = j;
    cid[v].assign(P, -1);
    int run = -1;
    for (int i = 0; i < P; ++i) {
      if (i == 0 || sorted[i].first != sorted[i - 1].first) run = idof[sorted[i].second];
      cid[v][sorted[i].second] = run;
    }
    count[v] = (int)firstp.size();
  }
  auto mult_of = [&](int v) {
    std::vector<int> sz(count[v], 0);
    for (int p = 0; p < P; ++p) ++sz[cid[v][p]];
    return *std::max_element(sz.begin(), sz.end());
  };
  // maximal qualifying clades, in the order a walk from the root meets them
  long gain = 0;
  std::vector<int> walk{t.root};
  while (!walk.empty()) {
    const int v = walk.back();
    walk.pop_back();
    if (v < S) continue;
    bool take = v != t.root && count[v] > 0 && nint[v] >= CC_MININT && cp.ncl < CC_MAXCL;
    int mm = 0;
    if (take) {
      mm = mult_of(v);
      const long save = (long)(cp.nblk - 1) * nint[v] * CC_STEP_CYCLES;
      const long cost = (long)cp.nblk * CC_BOUNDARY_CYCLES +
                        (long)((mm + CC_ROUNDS_U - 1) / CC_ROUNDS_U) * CC_BATCH_CYCLES + CC_CLADE_CYCLES;
      if (mode != 1 && 4 * save <= 5 * cost) take = false;
      if (take) gain += save - cost;
    }
    if (!take) {
      walk.push_back(t.ch2[v]);
      walk.push_back(t.ch1[v]);
      continue;
    }
    const int ci = cp.ncl++;
    cp.node[ci] = v;
    cp.ncls[ci] = count[v];
    cp.maxmult[ci] = mm;
    cp.nint[ci] = nint[v];
  }
  if (cp.ncl > 0 && mode != 1 && gain <= CC_FIXED_CYCLES) cp.ncl = 0;
  if (cp.ncl == 0) return PHY_OK;
  // tables
  int mmx = 0;
  for (int ci = 0; ci < cp.ncl; ++ci) {
    mmx = std::max(mmx, cp.maxmult[ci]);
    cp.maxcls = std::max(cp.maxcls, cp.ncls[ci]);
  }
  cp.rounds = (mmx + CC_ROUNDS_U - 1) / CC_ROUNDS_U * CC_ROUNDS_U;
  const int pcols = cp.nblk * CC_COLS;
  cp.cls_of.assign((size_t)cp.ncl * pcols, -1);
  cp.members.assign((size_t)cp.ncl * cp.rounds * CC_COLS, -1);
  cp.rep.assign((size_t)cp.ncl * CC_COLS, -1);
  cp.in_clade.assign(N, 0);
  cp.clade_of_tip.assign(S, -1);
  std::vector<int> gath(N, -1);
  for (int ci = 0; ci < cp.ncl; ++ci) {
    const int v = cp.node[ci];
    gath[v] = ci;
    std::vector<int> fill(CC_COLS, 0);
    for (int p = 0; p < P; ++p) {
      const int j = cid[v][p];
      cp.cls_of[(size_t)ci * pcols + p] = j;
      if (fill[j] == 0) cp.rep[(size_t)ci * CC_COLS + j] = p;
      cp.members[((size_t)ci * cp.rounds + fill[j]++) * CC_COLS + j] = p;
    }
    std::vector<int> st{v};
    while (!st.empty()) {
      const int n = st.back();
      st.pop_back();
      cp.in_clade[n] = 1;
      if (n < S) {
        cp.clade_of_tip[n] = ci;
        continue;
      }
      st.push_back(t.ch1[n]);
      st.push_back(t.ch2[n]);
    }
  }
  // programs: L (each clade from its first step, a cherry), then U
  std::vector<int> slot(N, -1);
  const std::vector<int> none(N, -1);
  for (int ci = 0; ci < cp.ncl; ++ci) {
    cp.lo[ci] = (int)(cp.prog.size() / STEP_INTS);
    int rc = emit_steps(t, cp.node[ci], none, cp.prog, cp.mat_branch, slot, cp.ndeep);
    if (rc) return rc;
    cp.hi[ci] = (int)(cp.prog.size() / STEP_INTS) - 1;
  }
  cp.nL = (int)(cp.prog.size() / STEP_INTS);
  cp.nmatL = (int)cp.mat_branch.size();
  int rc = emit_steps(t, t.root, gath, cp.prog, cp.mat_branch, slot, cp.ndeep);
  if (rc) return rc;
  cp.nU = (int)(cp.prog.size() / STEP_INTS) - cp.nL;
  cp.nmat = (int)cp.mat_branch.size();
  if (cp.nL + cp.nU != S - 1) return fail(PHY_EINVAL, "internal: L and U do not cover the tree");
  return PHY_OK;
}

// The chunk plan and the batched records of [L | U]: chunks never straddle
// the L / U boundary (U's chunk stays resident across the pattern blocks when
// it is a single one), a gathered child's record carries its clade
// (BR_X / BR_Y = -2 - clade), the root's slot (BR_XSO / BR_YSO) and its r
// plane's scratch offset (BR_GX / BR_GY: the clade root's branch
// has no dL/dP slot in U).  The r planes follow the S - 1 step slots.
int clade_records(const CladePlan& cp, int S, int C, int R, int cap, bool recompute, std::vector<int>& raw,
                  std::vector<int>& recs, int& nchunks, int& nrec) {
  raw = cp.prog;
  int rc = assign_chunks(raw, S - 1, cp.nmat, cap, recompute, nchunks, nrec, cp.nL);
  if (rc) return rc;
  recs = batched_records(raw, 2, C, R, S - 1, cp.nblk);
  return PHY_OK;
}
inline int clade_nslots(const CladePlan& cp, int S) { return S - 1 + cp.ncl * cp.nblk; }

// The device table of a plan (ints): header (first and last L step, classes
// and largest class per clade), then
//   cls[ncl][nblk][CC_COLS]   the column part (wave 0) of the class column's
//                             scratch byte offset for every pattern column;
//   spos[ncl][nblk][CC_COLS]  the byte offset, inside a category's part of the
//                             clade's r plane, of the position the pattern's r
//                             is stored at: 16 x (the patterns of lower
//                             classes + its rank in its class);
//   pre[ncl][CC_COLS]         16 x the position class j's run starts at;
//   cnt[ncl][CC_COLS]         the size of class j (0 past the class count).
// cls and spos are OOB on padding columns.  The kernel adds its wave's part.
std::vector<int> clade_table(const CladePlan& cp, int S, int C) {
  const int ncolwg = C * WAVE;
  auto colpart = [&](int q) { return (uint32_t)(((q / WAVE) * 2 * ncolwg + (q % WAVE)) * 16); };
  const int pcols = cp.nblk * CC_COLS;
  const size_t o_cls = CC_HDR, o_spos = o_cls + (size_t)cp.ncl * pcols, o_pre = o_spos + (size_t)cp.ncl * pcols,
               o_cnt = o_pre + (size_t)cp.ncl * CC_COLS;
  std::vector<int> tab(o_cnt + (size_t)cp.ncl * CC_COLS, (int)OOB);
  for (int ci = 0; ci < cp.ncl; ++ci) {
    tab[4 * ci] = cp.lo[ci];
    tab[4 * ci + 1] = cp.hi[ci];
    tab[4 * ci + 2] = cp.ncls[ci];
    tab[4 * ci + 3] = cp.maxmult[ci];
    for (int p = 0; p < pcols; ++p) {
      const int j = cp.cls_of[(size_t)ci * pcols + p];
      if (j >= 0) tab[o_cls + (size_t)ci * pcols + p] = (int)colpart(j);
    }
    int run = 0;
    for (int j = 0; j < CC_COLS; ++j) {
      int n = 0;
      for (int r = 0; r < cp.rounds; ++r) {
        const int p = cp.members[((size_t)ci * cp.rounds + r) * CC_COLS + j];
        if (p < 0) break;
        tab[o_spos + (size_t)ci * pcols + p] = (run + n) * 16;
        ++n;
      }
      tab[o_pre + (size_t)ci * CC_COLS + j] = run * 16;
      tab[o_cnt + (size_t)ci * CC_COLS + j] = n;
      run += n;
    }
  }
  (void)S;
  return tab;
}

// facts[12] and clades[CC_MAXCL][6] of phy_clade_compression / phy_clade_plan
// (include/phylo_hip_diag.h) for a plan and its records' chunk plan; zeros
// when `on` is false.  Either output may be NULL.
void clade_facts(const CladePlan& cp, int S, int nchunks, int nrec, bool on, int* facts, int* clades) {
  if (facts) {
    const int fv[12] = {cp.ncl, cp.nL, cp.nU, cp.nmatL, cp.nmat - cp.nmatL, cp.rounds, cp.maxcls, cp.nblk,
                        cp.ncl ? clade_nslots(cp, S) : 0, cp.ndeep, nchunks, nrec};
    for (int k = 0; k < 12; ++k) facts[k] = on ? fv[k] : 0;
  }
  if (clades)
    for (int ci = 0; ci < CC_MAXCL; ++ci) {
      const bool have = on && ci < cp.ncl;
      const int cv[6] = {cp.node[ci], cp.nint[ci], cp.ncls[ci], cp.maxmult[ci], cp.lo[ci], cp.hi[ci]};
      for (int k = 0; k < 6; ++k) clades[6 * ci + k] = have ? cv[k] : 0;
    }
}

// The quad sweeps' host plans (kernels: quad_engine.inc) and the constants they share with the kernels.
constexpr int QCOLS = 16;           // pattern columns per wave
constexpr int QUAD_MAX_DRAWS = 32;  // calls of at most this many draws take the quad sweep: with the
                                    // multi-wave form (r06, profiles/r06_quad_max_draws_ab.txt) fluA
                                    // 24 / 32 draws 143 / 145 against 167-171 us on the column sweep,
                                    // HCV 117 / 116 against 152-156, DS1 82 / 86 against 77-84; at 40,
                                    // 48, 64 and 100 draws the column sweep is faster (device-formed
                                    // eigensystems, fewer workgroups per draw): 16 until round 5

// The quad sweep's step records (quad_program, host-built per context from
// the program): LDS byte offsets and scratch / deep / slot element offsets
// instead of indices, 14 ints read as one block whose fields are all
// materialised at the top of the step (the plain Step's fields were fetched
// by up to four dependent scalar loads sunk into the step's branches, each
// behind an lgkmcnt(0) that also waits for the step's LDS reads: r04 ISA).
enum {
  QS_XT = 0,  // tip x: its byte row in the tip nibbles (x * QCOLS / 2), -1: x internal
  QS_YT,      // tip y: same
  QS_MXB,     // tip x's matrix record: byte offset in the wave's records
  QS_MYB,
  QS_MVB,     // the step's own matrix (F_MV)
  QS_VSO,     // a_v's scratch element offset (slot * C * 64), -1 at the root
  QS_FL,      // F_* flags
  QS_XSO,     // internal x's scratch element offset
  QS_YSO,
  QS_XDO,     // deep-stack element offset of x (F_XDEEP: both children internal)
  QS_VDO,     // deep-stack element offset of v (F_VDEEP)
  QS_MXG,     // dL/dP slot element offsets (matrix * 16) of mx, my, mv
  QS_MYG,
  QS_MVG,
};

// the quad program from the context's (unpacked) program
std::vector<int> quad_program(const std::vector<int>& prog, int nsteps, int C, int R) {
  std::vector<int> q((size_t)nsteps * STEP_INTS, 0);
  const int recb = R * 4 * 8;
  for (int s = 0; s < nsteps; ++s) {
    const int* p = &prog[(size_t)s * STEP_INTS];
    int* o = &q[(size_t)s * STEP_INTS];
    o[QS_XT] = p[ST_X] >= 0 ? p[ST_X] * (QCOLS / 2) : -1;
    o[QS_YT] = p[ST_Y] >= 0 ? p[ST_Y] * (QCOLS / 2) : -1;
    o[QS_MXB] = p[ST_MX] >= 0 ? p[ST_MX] * recb : 0;
    o[QS_MYB] = p[ST_MY] >= 0 ? p[ST_MY] * recb : 0;
    o[QS_MVB] = p[ST_MV] >= 0 ? p[ST_MV] * recb : 0;
    o[QS_VSO] = p[ST_VSLOT] >= 0 ? p[ST_VSLOT] * C * WAVE : -1;
    o[QS_FL] = p[ST_FLAGS] & ~(F_NOSTORE | F_PREVREC);  // every moved partial stored
    o[QS_XSO] = p[ST_XSLOT] >= 0 ? p[ST_XSLOT] * C * WAVE : 0;
    o[QS_YSO] = p[ST_YSLOT] >= 0 ? p[ST_YSLOT] * C * WAVE : 0;
    o[QS_XDO] = p[ST_XDPOS] >= 0 ? p[ST_XDPOS] * WAVE : 0;
    o[QS_VDO] = p[ST_VDPOS] >= 0 ? p[ST_VDPOS] * WAVE : 0;
    o[QS_MXG] = p[ST_MX] >= 0 ? p[ST_MX] * 16 : 0;
    o[QS_MYG] = p[ST_MY] >= 0 ? p[ST_MY] * 16 : 0;
    o[QS_MVG] = p[ST_MV] >= 0 ? p[ST_MV] * 16 : 0;
  }
  return q;
}

// The quad sweeps' dynamic LDS: the regions' sizes in order, which the host sums and the kernels step their
// pointers by.  Doubles: matrix records [C][nmat][R * 4] | tip state vectors [16][4] | root exchange [C][16] |
// tail [C][ntail][64] (qsweep_kernel's deep stack, qmw_kernel's slots).  Bytes, padded to 16: qmw_kernel's
// slot flags [C][ntail] ints and the error word | the block's tip nibbles [S][8].
struct QuadLds {
  size_t recs, tvec, xch, tail, flags, nib;
  PHY_HD QuadLds(int S, int C, int nmat, int R, int ntail, bool mw)
      : recs((size_t)C * nmat * (R * 4)), tvec(64), xch((size_t)C * QCOLS), tail((size_t)C * ntail * WAVE),
        flags(mw ? ((size_t)C * ntail * 4 + 16 + 15) / 16 * 16 : 0), nib(((size_t)S * (QCOLS / 2) + 15) / 16 * 16) {}
  PHY_HD size_t bytes() const { return (recs + tvec + xch + tail) * 8 + flags + nib; }
};
size_t quad_lds_bytes(int S, int C, int nmat, int R, int ndeep) { return QuadLds(S, C, nmat, R, ndeep, false).bytes(); }
size_t qmw_lds_bytes(int S, int C, int nmat, int R, int nslot) { return QuadLds(S, C, nmat, R, nslot, true).bytes(); }

// The multi-wave quad sweep (qmw_kernel, quad_engine.inc): its records.
constexpr int QMW_INTS = 20;
enum {
  QM_XT = 0, QM_YT, QM_MXB, QM_MYB, QM_MVB, QM_VSO, QM_FL, QM_XSO, QM_YSO,
  QM_XS,    // LDS slot of an internal x taken from a slot (-1: x is a tip or this wave's previous step)
  QM_YS,
  QM_VOUT,  // LDS slot this step's a_v goes to (and its r comes back in), -1: its parent takes it in a register
  QM_MXG, QM_MYG, QM_MVG,
  QM_NXSO,  // the reverse: the NEXT reverse step's x / y scratch offsets (-1: a tip), so its stored
            // partials are loaded a step ahead without a scalar load (scalar loads share lgkmcnt
            // with the LDS reads a step waits on: records a step ahead measured slower)
  QM_SID,   // this step's index (its slot flags carry it: a reused slot's flag names its current value)
  QM_XID,   // internal x's step index, y's
  QM_YID,
  QM_NYSO
};
// slot flag of step id's value in pass `ph` (0 forward, 1 reverse) of block trip `trip`
PHY_HD inline int qmw_tag(int trip, int ph, int id) { return ((trip * 2 + ph) << 13) | id; }
constexpr int QMW_MAXSTEPS = 8192;
constexpr int QM_XW = 32;     // x's slot is written by another wave: wait for its flag
constexpr int QM_YW = 64;
constexpr int QM_RW = 128;    // the reverse: r_v's slot is written by another wave
constexpr int QM_XTOP = 256;  // x is this wave's previous step (register); its r leaves in a register
constexpr int QM_YTOP = 512;
constexpr int QMW_MAXW = 4;

struct QmwPlan {
  int W = 0, maxst = 0, nslot = 0;
  int nst[QMW_MAXW] = {0, 0, 0, 0};
  int root_wave = 0;
  int span = 0;           // the list schedule's length in step times (one wave: nsteps)
  std::vector<int> prog;  // [W][maxst][QMW_INTS]
};

// prog: the context's 16-int program (build_program), qp: the quad program
bool quad_mw_plan(const std::vector<int>& prog, const std::vector<int>& qp, int nsteps, int W, QmwPlan& out) {
  if (W < 2 || W > QMW_MAXW || nsteps < 2 || nsteps >= QMW_MAXSTEPS) return false;
  // step graph: children steps (an internal child's slot index is its step)
  std::vector<int> cx(nsteps, -1), cy(nsteps, -1), par(nsteps, -1);
  for (int s = 0; s < nsteps; ++s) {
    const int* p = &prog[(size_t)s * STEP_INTS];
    if (p[ST_X] < 0) cx[s] = p[ST_XSLOT];
    if (p[ST_Y] < 0) cy[s] = p[ST_YSLOT];
    for (int u : {cx[s], cy[s]})
      if (u >= 0) {
        if (u >= s) return false;
        par[u] = s;
      }
  }
  // priority: steps to the root (the farthest first)
  std::vector<int> depth(nsteps, 0);
  for (int s = nsteps - 1; s >= 0; --s) depth[s] = par[s] >= 0 ? depth[par[s]] + 1 : 0;
  std::vector<int> wave_of(nsteps, -1), tfin(nsteps, -1);
  std::vector<std::vector<int>> lists(W);
  std::vector<int> last(W, -1);  // each wave's previous step
  int done = 0;
  for (int t = 0; done < nsteps; ++t) {
    std::vector<int> ready;
    for (int s = 0; s < nsteps; ++s) {
      if (wave_of[s] >= 0) continue;
      bool ok = true;
      for (int u : {cx[s], cy[s]})
        if (u >= 0 && (wave_of[u] < 0 || tfin[u] > t)) ok = false;
      if (ok) ready.push_back(s);
    }
    std::stable_sort(ready.begin(), ready.end(), [&](int a, int b) { return depth[a] > depth[b]; });
    std::vector<char> busy(W, 0);
    for (int s : ready) {
      int w = -1;
      for (int u : {cx[s], cy[s]})  // the wave whose previous step is a child of s
        if (u >= 0 && w < 0 && !busy[wave_of[u]] && last[wave_of[u]] == u) w = wave_of[u];
      for (int k = 0; k < W && w < 0; ++k)
        if (!busy[k]) w = k;
      if (w < 0) break;
      busy[w] = 1;
      wave_of[s] = w;
      tfin[s] = t + 1;
      lists[w].push_back(s);
      last[w] = s;
      ++done;
    }
    if (t > 4 * nsteps + 8) return false;
  }
  // operand routes and slots: a value taken from a slot gets one; a slot is
  // reused only by a producer on the wave that consumed its last value, later
  // in that wave's list (program order: the reuse is safe in both passes)
  std::vector<int> pos(nsteps, 0);
  for (int w = 0; w < W; ++w)
    for (size_t i = 0; i < lists[w].size(); ++i) pos[lists[w][i]] = (int)i;
  auto prev_in_wave = [&](int s) { return pos[s] > 0 ? lists[wave_of[s]][pos[s] - 1] : -1; };
  std::vector<int> vslot(nsteps, -1);
  std::vector<std::vector<std::pair<int, int>>> freed(W);  // per wave: (slot, position after which it is free)
  int nslot = 0;
  // in global time order: every producer needing a slot takes one
  std::vector<int> order(nsteps);
  for (int s = 0; s < nsteps; ++s) order[s] = s;
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return tfin[a] < tfin[b]; });
  std::vector<int> needs(nsteps, 0);
  for (int s = 0; s < nsteps; ++s)
    if (par[s] >= 0 && prev_in_wave(par[s]) != s) needs[s] = 1;
    else if (par[s] >= 0 && wave_of[par[s]] != wave_of[s]) needs[s] = 1;
  for (int s : order) {
    if (!needs[s]) continue;
    const int w = wave_of[s];
    int got = -1;
    for (size_t k = 0; k < freed[w].size(); ++k)
      if (freed[w][k].second < pos[s]) {
        got = freed[w][k].first;
        freed[w].erase(freed[w].begin() + k);
        break;
      }
    if (got < 0) got = nslot++;
    vslot[s] = got;
    freed[wave_of[par[s]]].push_back({got, pos[par[s]]});  // free after its consumer, on the consumer's wave
  }
  out.W = W;
  out.nslot = nslot;
  out.maxst = 0;
  for (int w = 0; w < W; ++w) {
    out.nst[w] = (int)lists[w].size();
    out.maxst = std::max(out.maxst, out.nst[w]);
  }
  out.root_wave = wave_of[nsteps - 1];
  out.span = *std::max_element(tfin.begin(), tfin.end());
  out.prog.assign((size_t)W * out.maxst * QMW_INTS, 0);
  for (int w = 0; w < W; ++w)
    for (size_t i = 0; i < lists[w].size(); ++i) {
      const int s = lists[w][i];
      const int* q = &qp[(size_t)s * STEP_INTS];
      int* o = &out.prog[((size_t)w * out.maxst + i) * QMW_INTS];
      o[QM_XT] = q[QS_XT];
      o[QM_YT] = q[QS_YT];
      o[QM_MXB] = q[QS_MXB];
      o[QM_MYB] = q[QS_MYB];
      o[QM_MVB] = q[QS_MVB];
      o[QM_VSO] = q[QS_VSO];
      int fl = q[QS_FL] & F_MV;
      o[QM_XSO] = q[QS_XSO];
      o[QM_YSO] = q[QS_YSO];
      o[QM_XS] = o[QM_YS] = -1;
      const int pv = prev_in_wave(s);
      if (cx[s] >= 0) {
        if (cx[s] == pv) fl |= QM_XTOP;
        else {
          o[QM_XS] = vslot[cx[s]];
          if (wave_of[cx[s]] != w) fl |= QM_XW;
        }
      }
      if (cy[s] >= 0) {
        if (cy[s] == pv && !(fl & QM_XTOP)) fl |= QM_YTOP;
        else {
          o[QM_YS] = vslot[cy[s]];
          if (wave_of[cy[s]] != w) fl |= QM_YW;
        }
      }
      o[QM_VOUT] = vslot[s];
      if (vslot[s] >= 0 && wave_of[par[s]] != w) fl |= QM_RW;
      o[QM_FL] = fl;
      o[QM_MXG] = q[QS_MXG];
      o[QM_MYG] = q[QS_MYG];
      o[QM_MVG] = q[QS_MVG];
      o[QM_SID] = s;
      o[QM_XID] = cx[s] >= 0 ? cx[s] : 0;
      o[QM_YID] = cy[s] >= 0 ? cy[s] : 0;
      o[QM_NXSO] = o[QM_NYSO] = -1;
      if (i > 0) {  // the reverse runs the list backwards: its next step is the previous one here
        const int* pq = &qp[(size_t)lists[w][i - 1] * STEP_INTS];
        if (pq[QS_XT] < 0) o[QM_NXSO] = pq[QS_XSO];
        if (pq[QS_YT] < 0) o[QM_NYSO] = pq[QS_YSO];
      }
    }
  // consistency: a step taking both children from its previous step is impossible
  for (int s = 0; s < nsteps; ++s)
    if (cx[s] >= 0 && cy[s] >= 0 && cx[s] == prev_in_wave(s) && cy[s] == prev_in_wave(s)) return false;
  return true;
}

// The problem: sizes, the record vectors of the tip masks in the data, the unplanned program and its matrix
// numbering, host copies of the inputs (the class plan and a changed clade mode are built from them on demand).
struct Problem {
  int S = 0, P = 0, Ppad = 0, C = 0, B = 0, rooted = 0, kind = 0, max_draws = 0;
  int nsteps = 0, nslots = 0, ndeep = 0, nmat = 0;
  int R = 5;                      // 4-vectors per matrix record (4 columns + extra tip masks)
  unsigned long long extra = 0;   // the extra tip masks, 4 bits each
  std::vector<int> vec_of;        // [16] record vector of a tip mask, -1 absent
  std::vector<int> prog;          // build_program's steps, before any chunk plan
  std::vector<int> mat_branch, gpos;  // [nmat] branch of matrix m, in order of use; [B] its inverse
  std::vector<uint8_t> tips;      // [S][P] tip codes, [P] weights, [S-1][3] peel rows
  std::vector<double> w;
  std::vector<int32_t> peel;
};

// Validates the sizes and the tree (phy_create's refusals that need no
// device) and fills the problem.
int make_problem(int S, int P, int C, int rooted, int kind, const uint8_t* tipcodes, const double* weights,
                 const int32_t* peel, int max_draws, Problem& pb) {
  if (S < 3) return fail(PHY_EINVAL, "need S >= 3 taxa");
  if (P < 1) return fail(PHY_EINVAL, "need P >= 1 patterns");
  if (C < 1 || C > 16) return fail(PHY_EINVAL, "C must be in 1..16");
  if (kind < PHY_JC69 || kind > PHY_GTR) return fail(PHY_EINVAL, "unknown model");
  if (max_draws < 1) return fail(PHY_EINVAL, "max_draws must be >= 1");
  if (!tipcodes || !weights || !peel) return fail(PHY_EINVAL, "NULL input array");
  for (size_t k = 0; k < (size_t)S * P; ++k)
    if (tipcodes[k] > 15) return fail(PHY_EINVAL, "tip code > 15");
  pb = Problem();
  pb.S = S; pb.P = P; pb.C = C; pb.rooted = rooted ? 1 : 0; pb.kind = kind; pb.max_draws = max_draws;
  pb.B = rooted ? 2 * S - 2 : 2 * S - 3;
  pb.Ppad = nblk_for(P, 2) * 2 * WAVE;  // room for either column plan
  int rc = build_program(S, peel, pb.rooted, pb.prog, pb.mat_branch, pb.nslots, pb.ndeep);
  if (rc) return rc;
  pb.nsteps = S - 1; pb.nmat = (int)pb.mat_branch.size();
  if (S > 16000 || pb.ndeep > 127)  // the packed device program's field widths
    return fail(PHY_EINVAL, "tree too large for the packed program (S <= 16000, deep stack <= 127)");
  // matrix records: 4 columns + P t for every non-one-hot mask t in the data
  // (15 always: the padding patterns' mask)
  pb.vec_of.assign(16, -1);
  {
    bool present[16] = {false};
    for (size_t k = 0; k < (size_t)S * P; ++k) present[tipcodes[k]] = true;
    present[15] = true;
    for (int j = 0; j < 4; ++j) pb.vec_of[1 << j] = j;
    int R = 4;
    for (int t = 0; t < 16; ++t)
      if (present[t] && pb.vec_of[t] < 0) {
        pb.extra |= (unsigned long long)t << (4 * (R - 4));
        pb.vec_of[t] = R++;
      }
    pb.R = R;
  }
  if (((size_t)C * pb.B + 16 + 1024) * sizeof(double) > LDS_CAP)
    return fail(PHY_EINVAL, "too many branches x categories for the finalize's LDS (C * B must be <= 19,440)");
  if (lds_bytes(S, C, pb.R, 3, 1, 0) > LDS_CAP) return fail(PHY_EINVAL, "too many taxa for one block's tips in LDS");
  if (pb.nmat != pb.B) return fail(PHY_EINVAL, "internal: one matrix per branch expected");
  pb.gpos.assign(pb.B, -1);
  for (int m = 0; m < pb.nmat; ++m) pb.gpos[pb.mat_branch[m]] = m;
  for (int b = 0; b < pb.B; ++b)
    if (pb.gpos[b] < 0) return fail(PHY_EINVAL, "internal: branch " + std::to_string(b) + " not in the program");
  pb.tips.assign(tipcodes, tipcodes + (size_t)S * P);
  pb.w.assign(weights, weights + P);
  pb.peel.assign(peel, peel + 3 * (S - 1));
  return PHY_OK;
}

// Tip nibbles: record vector of the pattern's mask (R <= 16); padding = mask
// 15; pattern 2j in the low nibble of byte j, 2j+1 in the high one.  With a
// clade plan the class block follows the pattern blocks: class j's states are
// those of its first pattern.
std::vector<uint8_t> pack_tips(const Problem& pb, const CladePlan* cp = nullptr) {
  const int S = pb.S, P = pb.P, row = (pb.Ppad + (cp ? CC_COLS : 0)) / 2;
  const uint8_t pad = (uint8_t)pb.vec_of[15];
  std::vector<uint8_t> tips((size_t)S * row, (uint8_t)(pad | (pad << 4)));
  auto setnib = [&](int t, int i, int code) {
    const uint8_t v = (uint8_t)pb.vec_of[code];
    uint8_t& b = tips[(size_t)t * row + i / 2];
    b = (i & 1) ? (uint8_t)((b & 0x0F) | (v << 4)) : (uint8_t)((b & 0xF0) | v);
  };
  for (int t = 0; t < S; ++t) {
    for (int i = 0; i < P; ++i) setnib(t, i, pb.tips[(size_t)t * P + i]);
    const int ci = cp ? cp->clade_of_tip[t] : -1;
    if (ci < 0) continue;
    for (int j = 0; j < cp->ncls[ci]; ++j)
      setnib(t, pb.Ppad + j, pb.tips[(size_t)t * P + cp->rep[(size_t)ci * CC_COLS + j]]);
  }
  return tips;
}

// Every preference: the environment's at phy_create (prefs_from_env), then
// the setters of include/phylo_hip_diag.h.
struct Prefs {
  int wg_budget = 0, cols = 0, lds_budget = 0;  // phy_set_tuning's; 0: the plan's resident workgroups / automatic
  int deep = 0;           // deep stack: 0 automatic, 1 LDS, 2 global
  bool recompute = true;  // rebuild cherries in the reverse instead of storing them
  bool fin = true;        // finalize inside the sweep when one workgroup runs a draw (PHY_FIN=0: off)
  bool qfuse = true;      // Q-parameter chain rule inside the sweep / finalize (PHY_QFUSE=0: off)
  bool quad = true, qmw = true;  // the quad sweep for small calls (PHY_QUAD=0: off), its multi-wave form (PHY_QMW=0)
  int cc_mode = -1;       // clade compression: 0 off, 1 on where applicable, -1 automatic
  int engine = 0;         // 0 automatic, 1 pattern, 2 class
  bool rescale = false;   // the rescaled pattern sweep: no quad sweep, no class sweep while it is on
};

Prefs prefs_from_env() {
  auto num = [](const char* name, int dflt, int lo, int hi) {
    const char* v = getenv(name);
    return v ? std::max(lo, std::min(hi, atoi(v))) : dflt;
  };
  auto flag = [](const char* name) {
    const char* v = getenv(name);
    return v ? atoi(v) != 0 : true;
  };
  Prefs p;
  p.lds_budget = num("PHY_LDS_BUDGET", 0, 16384, INT_MAX);
  p.wg_budget = num("PHY_WG_BUDGET", 0, 1, INT_MAX);
  p.cols = num("PHY_COLS", 0, 0, 2);
  p.deep = num("PHY_DEEP", 0, 0, 2);
  p.recompute = flag("PHY_RECOMPUTE");
  p.fin = flag("PHY_FIN");
  p.qfuse = flag("PHY_QFUSE");
  p.quad = flag("PHY_QUAD");
  p.qmw = flag("PHY_QMW");
  p.cc_mode = num("PHY_CLADE_COMPRESSION", -1, -1, 1);
  p.engine = num("PHY_ENGINE", 0, 0, 3);
  return p;
}

// Workgroup slots a context starts with: an explicit budget, or up to 4
// resident per CU, and at most one workgroup per one-column block and draw.
inline long wg_cap_for(const Problem& pb, int wg_budget, int cu_count) {
  return std::min<long>((long)nblk_for(pb.P, 1) * pb.max_draws,
                        (long)std::max(wg_budget, 4 * cu_count) + pb.max_draws);
}

// The current plans of a context: the pattern sweep's LDS plan (plan_lds), and what else a launch choice
// reads -- the engine, and whether the quad sweeps' and the compressed plan's records stand.
struct SweepPlan {
  int cu_count = 256;
  int K = 1;               // columns per lane
  bool lat = false;        // K = 1 latency plan (sweep_kernel<512, 1, .>: no register spills)
  int nblk = 0;            // pattern blocks of 64 K columns
  int cap_m = 0, nchunks = 0;  // matrices per LDS chunk, chunks per pass
  int ndl = 0;             // deep entries in LDS
  bool deep_lds = false;   // the whole deep stack is in LDS
  int nrec = 0;            // cherries and chains rebuilt, not stored
  int wg_resident = 512;   // resident workgroups
  size_t lds = 0;          // LDS bytes per workgroup
  long wg_need = 0;        // workgroup regions the largest launch of this plan may use
  std::vector<int> prog, records;  // the program with this plan's chunk fields; its device form (batched / packed)
  int engine = 0;          // 0 pattern sweep (the quad sweep for small calls), 1 class sweep
  bool quad_ok = false, qmw_ok = false;  // the quad sweep's / its multi-wave form's LDS plan fits
  bool cc_ok = false;      // the compressed plan's records match this LDS plan
  int cc_nchunks = 0, cc_nrec = 0;
};

// Columns per lane, matrices per LDS chunk and the chunk boundaries over the
// program.  Occupancy is bounded by registers (two waves per SIMD for K=2,
// four for K=1) and by LDS; the automatic plan takes the most workgroups
// per CU whose LDS share still holds chunks of >= MIN_CAP matrices (or the
// whole program).  An explicit budget (lds_budget) fixes the LDS share.
// A chunk holds >= 3 matrices (one step uses up to three).
// Fills the LDS part of `plan` (the engine and the *_ok flags are others'),
// which is untouched when the plan is refused.
int plan_lds(const Problem& pb, const Prefs& prefs, int cu_count, SweepPlan& plan) {
  // automatic: two columns per lane, unless even the one-column plan's
  // largest launch has at most one wave per SIMD (a sampler's few draws):
  // then nothing shares a SIMD, and one column per lane halves each wave's
  // step body (fluA, 4 draws: 182 -> 167 us per call; 100 draws: K = 2 stays
  // ahead, 220 against 235 us)
  int K = prefs.cols;
  bool lat = false;
  if (!K) {
    K = pb.C <= 8 ? 2 : 1;
    if (K == 2 && (long)pb.max_draws * nblk_for(pb.P, 1) * pb.C <= 4L * cu_count) {
      K = 1;
      lat = true;
    }
  }
  if (K == 2 && pb.C > 8) return fail(PHY_EINVAL, "two columns per lane need C <= 8");
  if ((size_t)std::max(pb.nslots, pb.ndeep) * K * 2 * pb.C * WAVE * 16 >= (size_t)OOB)
    return fail(PHY_EINVAL, "per-workgroup scratch region too large for 32-bit buffer offsets");
  const int nb = nblk_for(pb.P, K);
  int ndl = 0;  // deep-stack entries held in LDS
  auto cap_for = [&](size_t budget) {
    int cap = pb.nmat;
    while (cap > 3 && lds_bytes(pb.S, pb.C, pb.R, cap, K, ndl) > budget) --cap;
    return cap;
  };
  auto fits = [&](int cap, size_t budget) {
    return lds_bytes(pb.S, pb.C, pb.R, cap, K, ndl) <= budget && cap >= std::min(pb.nmat, MIN_CAP);
  };
  const int by_waves = std::max(1, 4 * waves_per_simd(K, lat) / pb.C);  // workgroups per CU
  int cap = 0;
  // Deep-stack placement at a given LDS share: the whole stack in LDS if it
  // fits beside chunks of MIN_CAP matrices (mode 0/1), else (mode 0/2) its
  // outermost entries [0, ndl) in LDS and the rest in global memory, with
  // the largest ndl that still fits.
  auto place = [&](size_t budget, bool last) -> bool {
    if (prefs.deep != 2) {
      ndl = pb.ndeep;
      cap = cap_for(budget);
      if (fits(cap, budget) || (prefs.deep == 1 && last)) return true;
      if (prefs.deep == 1) return false;
    }
    for (ndl = pb.ndeep - 1; ndl >= 0; --ndl) {
      if (prefs.deep == 2) ndl = 0;
      cap = cap_for(budget);
      if (fits(cap, budget)) return true;
    }
    ndl = 0;
    cap = cap_for(budget);
    return false;
  };
  if (prefs.lds_budget > 0) {
    place(std::min<size_t>(LDS_CAP, (size_t)prefs.lds_budget), true);
  } else {
    // most workgroups per CU first
    for (int t = by_waves; t >= 1; --t)
      if (place(LDS_CAP / t, t == 1)) break;
  }
  const size_t lds = lds_bytes(pb.S, pb.C, pb.R, cap, K, ndl);
  if (lds > LDS_CAP) return fail(PHY_EINVAL, "tree too large for LDS (tips of one block)");
  std::vector<int> prog = pb.prog;
  int nch = 0, nrec = 0;
  const int rc = assign_chunks(prog, pb.nsteps, pb.nmat, cap, prefs.recompute, nch, nrec);
  if (rc) return rc;
  plan.cu_count = cu_count; plan.K = K; plan.lat = lat; plan.nblk = nb;
  plan.wg_resident = cu_count * std::min<int>(by_waves, (int)(LDS_CAP / lds));
  // workgroup regions the largest launch of this plan may use (choose_launch's
  // gx per draw): the context grows its regions to it, so no launch fails
  const long budget = prefs.wg_budget > 0 ? prefs.wg_budget : plan.wg_resident;
  plan.wg_need = std::min<long>((long)pb.max_draws * nb, budget + pb.max_draws);
  plan.records = K == 2 ? batched_records(prog, K, pb.C, pb.R) : pack_program(prog);
  plan.prog = std::move(prog);
  plan.cap_m = cap; plan.nchunks = nch; plan.nrec = nrec; plan.ndl = ndl; plan.lds = lds;
  plan.deep_lds = ndl > 0 && ndl == pb.ndeep;
  return PHY_OK;
}

// The clades a context takes for its mode (none for mode 0, for C > 8, and
// when the compressed numbering or scratch would not fit the context's).
int select_clades(const Problem& pb, int mode, CladePlan& cp) {
  cp = CladePlan();
  if (mode == 0 || pb.C > 8) return PHY_OK;
  PeelTree t;
  int rc = parse_peel(pb.S, pb.peel.data(), pb.rooted, t);
  if (rc || (rc = plan_clades(t, pb.P, pb.tips.data(), mode, cp))) return rc;
  if (cp.ncl > 0 && (cp.nmat != pb.nmat || cp.nblk * CC_COLS != pb.Ppad ||
                     (size_t)clade_nslots(cp, pb.S) * 2 * 2 * pb.C * WAVE * 16 >= (size_t)OOB))
    cp = CladePlan();
  return PHY_OK;
}

// The compressed plan's records for the current LDS plan (cap_m, recompute);
// plan.cc_ok says whether a launch may take them.
int plan_clade_records(const Problem& pb, const Prefs& prefs, const CladePlan& cp, SweepPlan& plan,
                       std::vector<int>& recs) {
  plan.cc_ok = false;
  if (cp.ncl == 0 || plan.K != 2) return PHY_OK;
  if (cp.ndeep > pb.ndeep) return PHY_OK;  // the LDS plan is sized for the whole tree's deep stack
  std::vector<int> raw;
  int rc = clade_records(cp, pb.S, pb.C, pb.R, plan.cap_m, prefs.recompute, raw, recs, plan.cc_nchunks, plan.cc_nrec);
  if (rc) return rc;
  plan.cc_ok = true;
  return PHY_OK;
}

// The quad sweeps' plans for a context: the one-wave program (every moved partial stored, no rebuilt cherries)
// when its LDS plan fits, and the multi-wave form with as many waves per category as a 1024-thread workgroup
// holds (<= 4), fewer when that schedule's hand-off slots overflow LDS (a balanced 64-taxon tree at C = 4: 3).
struct QuadPlan {
  size_t lds = 0, mw_lds = 0;  // dynamic LDS bytes (the kernels' static eigensystem copy comes on top)
  std::vector<int> prog;
  QmwPlan mw;
};

// Planned from plan.prog; says in plan.quad_ok / plan.qmw_ok which of the two stand.
QuadPlan plan_quad(const Problem& pb, SweepPlan& plan) {
  QuadPlan q;
  q.lds = quad_lds_bytes(pb.S, pb.C, pb.nmat, pb.R, pb.ndeep);
  plan.quad_ok = q.lds + EIG_LEN * sizeof(double) <= LDS_CAP;  // + qsweep_kernel's static eigensystem copy
  plan.qmw_ok = false;
  if (!plan.quad_ok) return q;
  q.prog = quad_program(plan.prog, pb.nsteps, pb.C, pb.R);
  for (int W = std::min(QMW_MAXW, 16 / pb.C); W >= 2 && !plan.qmw_ok; --W) {
    if (!quad_mw_plan(plan.prog, q.prog, pb.nsteps, W, q.mw)) continue;
    q.mw_lds = qmw_lds_bytes(pb.S, pb.C, pb.nmat, pb.R, q.mw.nslot);
    plan.qmw_ok = q.mw_lds + EIG_LEN * sizeof(double) <= LDS_CAP;
  }
  return q;
}

// The split epilogue of the quad sweeps (qfin_kernel): items of bper branches
// x C categories per workgroup, nspl workgroups per draw.
inline int qfin_bper(const Problem& pb) { return std::max(1, std::min((pb.B + 15) / 16, QFIN_ITEMS / pb.C)); }
inline int qfin_nspl(const Problem& pb) { return (pb.B + qfin_bper(pb) - 1) / qfin_bper(pb); }

enum LaunchPath {  // what one evaluation of n draws launches
  PATH_CLASS = 0,    // the class sweep (class_engine.inc)
  PATH_QUAD,         // the one-wave quad sweep
  PATH_QUAD_MW,      // the multi-wave quad sweep
  PATH_PATTERN_CC,   // the two-column pattern sweep on the compressed plan
  PATH_PATTERN,      // the pattern sweep
};
struct LaunchChoice {
  int path = PATH_PATTERN;
  int gx = 1;        // workgroups per draw of the sweep
  int g_direct = 0;  // one workgroup per draw: it writes the draw's dL/dP rows in place
  int fin = 0;       // ... and the finalize fits in its LDS: the sweep writes the whole output row
  int qf = 0;        // ... and the Q-parameter chain rule too
  int gsum_in = 0;   // the finalize sums the few per-workgroup dL/dP slots itself (else gsum_kernel first)
  int fin_qf = 0;    // the epilogue after the sweep (finalize_kernel / qfin_kernel) runs the chain rule
  bool qfin = false;        // the quad sweeps' split epilogue (qfin_kernel) applies
  bool quad_build = false;  // the quad sweep builds its matrix records (no pmat launch)
  bool quad() const { return path == PATH_QUAD || path == PATH_QUAD_MW; }
  bool cc() const { return path == PATH_PATTERN_CC; }
  // what goes with the choice (launch() sets them): the draws' eigensystems, the plan's matrix numbering
  const double* eig = nullptr;
  const int *mat_branch = nullptr, *gpos = nullptr;
};

// The single place that decides a launch.  The class sweep when it is the
// context's engine.  The quad sweep for calls of <= QUAD_MAX_DRAWS draws,
// unless a column plan is set explicitly (phy_set_tuning(cols > 0)), rescaling
// is on or PHY_QUAD=0: one workgroup of C waves per 16-column block and draw,
// as many blocks per workgroup as keep the launch within one wave per SIMD; it
// builds its own matrix records when the eigensystems are given.  Else the
// pattern sweep on persistent workgroups: the explicit budget, else exactly
// what is resident, at most one per block (every workgroup has a block to
// write its slots); on the compressed plan when that is one workgroup per draw
// of the two-column sweep, without rescaling, and clades are taken.
LaunchChoice choose_launch(const Problem& pb, const Prefs& prefs, const SweepPlan& plan, int n, bool eig_given) {
  LaunchChoice ch;
  const int C = pb.C, B = pb.B;
  if (plan.engine == 1) {
    ch.path = PATH_CLASS;
    return ch;
  }
  if (plan.quad_ok && prefs.quad && prefs.cols == 0 && n <= QUAD_MAX_DRAWS && !prefs.rescale) {
    ch.path = (plan.qmw_ok && prefs.qmw) ? PATH_QUAD_MW : PATH_QUAD;
    ch.quad_build = eig_given;
    const int nb = (pb.P + QCOLS - 1) / QCOLS;
    ch.gx = std::max(1, std::min(nb, (4 * plan.cu_count) / (C * n)));
    ch.gsum_in = ch.gx <= 16 ? 1 : 0;
    ch.fin_qf = prefs.qfuse ? 1 : 0;
    ch.qfin = ch.gx <= QFIN_SLOTS && C * qfin_bper(pb) <= QFIN_ITEMS && 8 * C <= 128 && prefs.qfuse;
  } else {
    const int budget = prefs.wg_budget > 0 ? prefs.wg_budget : plan.wg_resident;
    ch.gx = std::max(1, std::min(plan.nblk, (budget + n - 1) / n));
    ch.g_direct = ch.gx == 1 ? 1 : 0;
    const bool cc = plan.cc_ok && prefs.cc_mode != 0 && plan.K == 2 && !prefs.rescale && ch.gx == 1;
    ch.path = cc ? PATH_PATTERN_CC : PATH_PATTERN;
    // finalize inside the sweep when its LDS holds [C][B] + [C][8] doubles
    // past the tips; the chain rule too when QG_SHARED more fit
    const size_t room = plan.lds - tip_nib_bytes(pb.S, plan.K) - 16 * 4 * sizeof(double);
    ch.fin = (ch.g_direct && prefs.fin && ((size_t)C * B + 8 * C) * 8 <= room) ? 1 : 0;
    ch.qf = (ch.fin && prefs.qfuse && ((size_t)C * B + 8 * C + QG_SHARED) * 8 <= room) ? 1 : 0;
    // a draw over a few workgroups: the finalize sums their slots itself
    // (one epilogue launch: slot sums, finalize, chain rule); over many, the
    // wide gsum kernel first
    ch.gsum_in = (!ch.g_direct && ch.gx <= 16) ? 1 : 0;
    ch.fin_qf = (!ch.fin && prefs.qfuse) ? 1 : 0;
  }
  // finalize_kernel runs the chain rule too unless its LDS ([C][B] inner
  // products, Q, the reduction rows and the chain rule's QG_SHARED) would
  // pass the 160 KiB cap: then it is left to qgrad_kernel (large C*B)
  if (!ch.qfin && ((size_t)C * B + 16 + 1024 + QG_SHARED) * sizeof(double) > LDS_CAP) ch.fin_qf = 0;
  return ch;
}

// The epilogue's form of the row engines (forest_plan.h, part_plan.h;
// row_engine.inc): choose_launch's decisions for the unrescaled pattern sweep
// at one workgroup per row, taken once for the context (a budget of one
// workgroup makes gx = 1 for every n).
struct RowForm { int fin = 0, qf = 0, fin_qf = 0; };
RowForm row_epilogue_form(const Problem& pb, const Prefs& prefs, const SweepPlan& plan) {
  Prefs one = prefs;
  one.quad = false; one.cc_mode = 0; one.wg_budget = 1; one.rescale = false;
  SweepPlan q = plan;
  q.engine = 0; q.quad_ok = q.qmw_ok = q.cc_ok = false;
  const LaunchChoice ch = choose_launch(pb, one, q, 1, false);
  return RowForm{ch.fin, ch.qf, ch.fin_qf};
}

}  // namespace

#endif  // PHYLO_SWEEP_PLAN_H
