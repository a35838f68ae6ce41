// Clade compression of the batched pattern sweep (DESIGN.md 5, "Compressed
// clades"): host planning.  Included by phylo_hip.hip inside its anonymous
// namespace, after emit_steps / assign_chunks / batched_records.
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

// selection is attempted only for alignments this small (the plan is
// quadratic-ish host work and only one-workgroup-per-draw launches use it)
constexpr size_t CC_MAX_CELLS = (size_t)1 << 22;

// Cost model, in cycles of one category wave per draw (DESIGN.md 5 and 7).
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
// model says (DESIGN.md 7).  A clade is kept when its saving exceeds its
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
