// Drives the device-free class planner (phylostan_amd/csrc/class_plan.h) over
// generated trees and alignments under a host sanitizer
// (tests/test_class_plan_cpu.py builds it with -fsanitize=address,undefined),
// every knob set through ClassPrefs, and checks each plan against statements
// that do not reuse the planner's arithmetic: class counts against a naive
// count of distinct tip tuples, and every index of every table against the
// table it points into, the way the kernels and launch_class follow them.
#include <cstdio>
#include <set>

#include "class_plan.h"

static unsigned long long g_lcg = 12345;
static unsigned rnd(unsigned n) {
  g_lcg = g_lcg * 6364136223846793005ULL + 1442695040888963407ULL;
  return (unsigned)(g_lcg >> 33) % n;
}

// kind 0 caterpillar, 1 balanced, 2 random; internal nodes numbered in creation order
static std::vector<int32_t> make_peel(int S, int kind, bool rooted) {
  std::vector<int> live(S);
  for (int i = 0; i < S; ++i) live[i] = i;
  std::vector<int32_t> peel;
  for (int nxt = S; live.size() > 1; ++nxt) {
    size_t i = 0, j = 1;
    if (kind == 0 && nxt > S) i = live.size() - 1, j = 0;  // the last internal node and the next tip
    if (kind == 2) {
      i = rnd((unsigned)live.size());
      j = rnd((unsigned)live.size() - 1);
      if (j >= i) ++j;
    }
    int a = live[i], b = live[j];
    if (live.size() == 2 && !rooted && b != 2 * S - 3) std::swap(a, b);  // child 2 of the root: node 2S-3
    live.erase(live.begin() + std::max(i, j));
    live.erase(live.begin() + std::min(i, j));
    if (kind == 1) live.push_back(nxt); else live.insert(live.begin(), nxt);
    if (kind == 2) std::swap(live[0], live[rnd((unsigned)live.size())]);
    peel.insert(peel.end(), {a, b, nxt});
  }
  return peel;
}

static int g_bad = 0;
static const char* g_what = "";
#define CHECK(cond)                                                                \
  do {                                                                             \
    if (!(cond)) {                                                                 \
      if (g_bad < 40) std::fprintf(stderr, "FAIL %s: %s (line %d)\n", g_what, #cond, __LINE__); \
      ++g_bad;                                                                     \
      return;                                                                      \
    }                                                                              \
  } while (0)

struct Shape {
  const char* name;
  int S, P, rooted;
  std::vector<int32_t> peel;
  std::vector<uint8_t> tips;  // [S][P]
  std::vector<double> w;
};

// distinct tip-code tuples below every internal node, counted with a set
static std::vector<int> naive_classes(const Shape& sh, const std::vector<int>& vec_of) {
  const int S = sh.S, P = sh.P, N = 2 * S - 1;
  std::vector<std::vector<int>> below(N);
  for (int t = 0; t < S; ++t) below[t] = {t};
  std::vector<int> n(N, 0);
  for (int r = 0; r < S - 1; ++r) {
    const int x = sh.peel[3 * r], y = sh.peel[3 * r + 1], v = sh.peel[3 * r + 2];
    below[v] = below[x];
    below[v].insert(below[v].end(), below[y].begin(), below[y].end());
    std::set<std::vector<int>> seen;
    std::vector<int> tup(below[v].size());
    for (int i = 0; i < P; ++i) {
      for (size_t k = 0; k < tup.size(); ++k) tup[k] = vec_of[sh.tips[(size_t)below[v][k] * P + i]];
      seen.insert(tup);
    }
    n[v] = (int)seen.size();
  }
  return n;
}

static bool in(long long v, long long lo, long long hi) { return v >= lo && v < hi; }  // [lo, hi)

static void check_plan(const Shape& sh, const Problem& pb, const ClassPrefs& prefs, const ClassPlan& p,
                       const std::vector<int>& naive, long long& long_seen) {
  const int S = sh.S, P = sh.P, N = 2 * S - 1, root = sh.peel[3 * (S - 2) + 2];
  std::vector<int> par(N, -1), level(N, 0), ch1(N, -1), ch2(N, -1);
  for (int r = 0; r < S - 1; ++r) {
    const int x = sh.peel[3 * r], y = sh.peel[3 * r + 1], v = sh.peel[3 * r + 2];
    par[x] = par[y] = v;
    ch1[v] = x;
    ch2[v] = y;
    level[v] = 1 + std::max(level[x], level[y]);
  }
  const int L = level[root];
  CHECK(p.levels == L && p.root == root && (int)p.nodes.size() == N && (int)p.lv.size() == L + 1);
  auto ncls = [&](int v) { return v < S ? pb.R : p.nodes[v].n; };
  // class counts: the naive count; sizes
  long long classes = 0;
  for (int v = S; v < N; ++v) {
    CHECK(p.nodes[v].n == naive[v]);
    if (v != root) classes += naive[v];
  }
  CHECK(p.classes == classes && p.nroot == naive[root]);
  const long long slots = (long long)p.cls.size() / 2, ntl = (long long)p.tiles.size(), nsp = (long long)p.spans.size();
  CHECK(slots == p.nslots + p.nroot && p.rootoff == p.nslots && p.nslots % WAVE == 0);
  CHECK((long long)p.secpos.size() == slots && (long long)p.sspan.size() == slots);
  CHECK(p.ntiles == std::max<long long>(ntl, 1) && p.nspans == nsp && p.nstage >= 8 && p.nstage % 8 == 0);
  CHECK((long long)p.stperm.size() == p.nstage);
  // root weights and pattern map
  double ws = 0, wr = 0;
  for (double x : sh.w) ws += x;
  for (double x : p.wroot) wr += x;
  CHECK((int)p.wroot.size() == p.nroot && (int)p.pat_root.size() == P && ws == wr);  // integer weights: exact
  for (int i = 0; i < P; ++i) CHECK(in(p.pat_root[i], 0, p.nroot));
  // stperm is a permutation
  {
    std::vector<char> hit(p.nstage, 0);
    for (int q : p.stperm) {
      CHECK(in(q, 0, p.nstage) && !hit[q]);
      hit[q] = 1;
    }
  }
  // the dL/dP rows of the branches tile [0, ngs)
  {
    std::vector<char> hit(std::max(p.ngs, 1), 0);
    CHECK((int)p.gbase.size() == p.B && (int)p.gcount.size() == p.B && (int)p.pbase.size() == p.B);
    int mg = 0;
    for (int b = 0; b < p.B; ++b) {
      CHECK(p.gcount[b] >= 1 && p.gbase[b] >= 0 && p.gbase[b] + p.gcount[b] <= p.ngs);
      for (int g = p.gbase[b]; g < p.gbase[b] + p.gcount[b]; ++g) {
        CHECK(!hit[g]);
        hit[g] = 1;
      }
      mg = std::max(mg, p.gcount[b]);
      CHECK(in(p.pbase[b], -1, p.nsub) && (p.pbase[b] >= 0) == (p.gcount[b] > GSUB_MIN));
    }
    for (int g = 0; g < p.ngs; ++g) CHECK(hit[g]);
    CHECK(mg == p.max_gcount && (int)p.gsub.size() == p.nsub);
    for (const CPair& g : p.gsub) CHECK(g.x >= 0 && g.y >= 1 && g.y <= GSUB_ROWS && g.x + g.y <= p.ngs);
  }
  // nodes: every offset inside its table
  for (int v = S; v < N; ++v) {
    const CNode& nd = p.nodes[v];
    const int x = ch1[v], y = ch2[v];
    CHECK(nd.off >= 0 && nd.off + nd.n <= (v == root ? slots : (long long)p.nslots));
    CHECK(x < S ? nd.offx == -1 && in(nd.mx, 0, p.nmat) && in(nd.gx, 0, p.ngs) : nd.offx == p.nodes[x].off && nd.mx == -1 && nd.gx == -1);
    CHECK(y < S ? nd.offy == -1 && in(nd.my, 0, p.nmat) && in(nd.gy, 0, p.ngs) : nd.offy == p.nodes[y].off && nd.my == -1 && nd.gy == -1);
    CHECK(in(nd.mv, -1, p.nmat) && in(nd.gv, -1, p.ngs) && (nd.mv >= 0) == (nd.gv >= 0) && (v != root || nd.mv == -1));
    CHECK(in(nd.stx, -1, p.nstage) && in(nd.sty, -1, p.nstage) && in(nd.sin, -1, p.nstage) && in(nd.ptile, -1, ntl));
    CHECK(nd.stx == (x >= S ? p.nodes[x].sin : -1) && nd.sty == (y >= S ? p.nodes[y].sin : -1));
    CHECK((nd.secy == 0 || nd.secy == 1) && (nd.sord == 0 || nd.sord == 1));
    for (int q = 0; q < nd.n; ++q) {
      CHECK(in(p.cls[2 * ((size_t)nd.off + q)], 0, ncls(x)) && in(p.cls[2 * ((size_t)nd.off + q) + 1], 0, ncls(y)));
      CHECK(in(p.secpos[(size_t)nd.off + q], 0, nd.n));
    }
  }
  CHECK(p.root_tips == ((ch1[root] < S || ch2[root] < S) ? 1 : 0));
  CHECK(p.rootr >= 1 && p.nrootch >= 1 && (long long)p.nrootch * p.rootr * ROOT_CHUNK >= p.nroot);
  // tiles and spans
  for (const CTile& t : p.tiles) {
    CHECK(in(t.node, S, N) && t.node != root && t.t >= 0 && (long long)t.t * WAVE < t.m && in(t.kfirst, 0, ncls(t.node)));
    CHECK(t.sb == -1 || (t.sb >= 0 && t.sb % WAVE == 0 && t.sb + WAVE <= p.nstage));
    CHECK((t.lo | t.hi) != 0 || (t.flags & 1));
  }
  for (const CSpan& s : p.spans)
    CHECK(in(s.node, S, N) && s.node != root && in(s.k, 0, ncls(s.node)) && s.t0 >= 0 && s.t0 < s.t1 && s.t1 < ntl &&
          p.tiles[s.t0].node == s.node && p.tiles[s.t1].node == s.node);
  // chunks: every class of every non-root internal node in exactly one
  {
    std::vector<char> hit(std::max(p.nslots, 1), 0);
    for (size_t i = 0; i < p.chunks.size(); ++i) {
      const CChunkN& c = p.chunks[i];
      CHECK(in(c.node, S, N) && c.node != root && c.j0 >= 0 && c.jn >= 1 && c.jn <= WAVE && c.j0 + c.jn <= ncls(c.node));
      CHECK(c.ci == c.j0 / WAVE && std::memcmp(&c.nd, &p.nodes[c.node], sizeof(CNode)) == 0);
      for (int j = 0; j < c.jn; ++j) {
        const long long s = (long long)c.nd.off + c.j0 + j;
        CHECK(in(s, 0, p.nslots) && !hit[s]);
        hit[s] = 1;
      }
    }
    for (int v = S; v < N; ++v)
      if (v != root)
        for (int q = 0; q < p.nodes[v].n; ++q) CHECK(hit[p.nodes[v].off + q]);
  }
  // levels and the clade table: ranges inside their tables
  CHECK(in(p.Lc, 0, std::max(L - 1, 1)) && (int)p.clade.size() == std::max(p.nclade, 1) * std::max(p.Lc, 1));
  for (int l = 1; l < L; ++l) {
    const ClassLevel& v = p.lv[l];
    CHECK(v.chunk0 >= 0 && v.nchunk >= 0 && v.chunk0 + v.nchunk <= (long long)p.chunks.size());
    CHECK(v.tile0 >= 0 && v.ntile >= 0 && v.tile0 + v.ntile <= ntl && v.span0 >= 0 && v.nspan >= 0 && v.span0 + v.nspan <= nsp);
    CHECK(v.lfix0 >= 0 && v.nlfix >= 0 && v.lfix0 + v.nlfix <= (long long)p.lfix.size());
    CHECK(v.sec0 >= 0 && ((long long)v.sec0 + v.ntile) * WAVE <= p.nstage);
    for (int i = v.chunk0; i < v.chunk0 + v.nchunk; ++i) CHECK(level[p.chunks[i].node] == l);
    for (int i = v.tile0; i < v.tile0 + v.ntile; ++i) CHECK(level[p.tiles[i].node] == l && p.tiles[i].sb >= 0);
    for (int i = v.span0; i < v.span0 + v.nspan; ++i) CHECK(level[p.spans[i].node] == l);
  }
  std::vector<int> handlers(nsp, 0);  // who sums each tile-crossing segment
  for (const CladeLevel& c : p.clade) {
    CHECK(c.chunk0 >= 0 && c.nchunk >= 0 && c.chunk0 + c.nchunk <= (long long)p.chunks.size());
    CHECK(c.tile0 >= 0 && c.ntile >= 0 && c.tile0 + c.ntile <= ntl && c.span0 >= 0 && c.nspan >= 0 && c.span0 + c.nspan <= nsp);
    for (int i = c.span0; i < c.span0 + c.nspan; ++i) ++handlers[i];
  }
  CHECK((int)p.rtile.size() == p.nrtile && (int)p.rspan.size() == p.nrspan);
  for (int i : p.rtile) CHECK(in(i, 0, ntl));
  for (int i : p.rspan) {
    CHECK(in(i, 0, nsp));
    ++handlers[i];
  }
  for (int i : p.lfix) CHECK(in(i, 0, nsp));
  for (int l = 1; l < L; ++l)
    if (!p.lv[l].revfix)
      for (int i = p.lv[l].lfix0; i < p.lv[l].lfix0 + p.lv[l].nlfix; ++i) ++handlers[p.lfix[i]];
  CHECK((int)p.clong.size() == p.nclong && (p.clf.empty() || p.clf.size() == p.chunks.size()));
  for (size_t ci = 0; ci < p.clf.size(); ++ci) {
    CHECK(p.clf[ci].x >= 0 && p.clf[ci].y >= 0 && p.clf[ci].x + p.clf[ci].y <= p.nclong);
    for (int i = p.clf[ci].x; i < p.clf[ci].x + p.clf[ci].y; ++i) {
      CHECK(in(p.clong[i], 0, nsp));
      const CSpan& s = p.spans[p.clong[i]];
      CHECK(p.lv[level[s.node]].revfix && (size_t)(p.nodes[s.node].off + s.k) / WAVE == ci);
      ++handlers[p.clong[i]];
    }
  }
  for (long long i = 0; i < nsp; ++i) {
    const CSpan& s = p.spans[i];
    const CPair ss = p.sspan[(size_t)p.nodes[s.node].off + s.k];
    const bool is_short = s.t1 - s.t0 <= SPAN_LANE_MAX;
    if (ss.y) {
      CHECK(is_short && ss.x == s.t0 && ss.y == s.t1 - s.t0);
      ++handlers[i];
    }
    CHECK(handlers[i] == 1);
    if (!is_short) ++long_seen;
  }
  for (const CPair& ss : p.sspan) CHECK(ss.y == 0 || (ss.x >= 0 && ss.y >= 1 && (long long)ss.x + ss.y < ntl));
  // level pairs
  CHECK(p.pair.empty() == (p.npairs == 0) && (p.pair.empty() || p.pair.size() == p.chunks.size()) &&
        p.gc.size() == p.pair.size() * WAVE);
  for (size_t ci = 0; ci < p.pair.size(); ++ci) {
    const int v = p.chunks[ci].node;
    for (int c = 0; c < 2; ++c) {
      const int r = c ? p.pair[ci].y : p.pair[ci].x;
      CHECK(r == -1 || (r == (c ? ch2[v] : ch1[v]) && r >= S && p.lv[level[v]].pair == 2 && level[r] == level[v] - 1));
      if (r < 0) continue;
      for (int j = 0; j < p.chunks[ci].jn; ++j) {
        const CQuad& g = p.gc[ci * WAVE + j];
        CHECK(in(c ? g.z : g.x, 0, ncls(ch1[r])) && in(c ? g.w : g.y, 0, ncls(ch2[r])));
      }
    }
  }
  // the top chain
  CHECK(in(p.chain_m, 0, CHAIN_MAX + 1) && p.chain_m != 1 && (int)p.links.size() == p.chain_m);
  if (p.chain_m) {
    CHECK(p.chain_hi == L - 1 && p.chain_lo == L - p.chain_m && p.chain_lo > p.Lc && p.chain_ntp % WAVE == 0 &&
          p.chain_ntp >= p.chain_ntop && p.chain_ntop >= 1);
    CHECK(p.ctab.size() == (size_t)5 * p.chain_m * p.chain_ntp && (int)p.crep.size() == p.chain_ntp);
    for (int i = 0; i < p.chain_m; ++i) {
      const CLink& k = p.links[i];
      CHECK(k.off >= 0 && k.off < p.nslots && in(k.mv, -1, p.nmat) && in(k.spine, i ? 0 : -1, i ? 2 : 0));
      CHECK(in(k.stx, -1, p.nstage) && in(k.sty, -1, p.nstage) && in(k.gv, -1, p.ngs) && in(k.gx, -1, p.ngs) && in(k.gy, -1, p.ngs));
      for (int kt = 0; kt < p.chain_ntop; ++kt)
        for (int c = 3; c < 5; ++c) CHECK(in(p.ctab[((size_t)c * p.chain_m + i) * p.chain_ntp + kt], 0, p.chain_ntop));
    }
    CHECK(p.chain_toff == p.links[p.chain_m - 1].off);
  }
  // what each knob asks for
  if (prefs.clade >= 0) CHECK(p.Lc == std::max(0, std::min(prefs.clade, L - 2)));
  if (!prefs.chain) CHECK(p.chain_m == 0);
  if (!prefs.pair) CHECK(p.npairs == 0);
  if (!prefs.revfix) CHECK(p.nclong == 0);
  if (prefs.stage_order > (1ll << 39)) CHECK(p.nsord == 0);
  if (prefs.root_wgs == 1) CHECK(p.nrootch == 1 && p.rootr == (p.nroot + ROOT_CHUNK - 1) / ROOT_CHUNK);
  CHECK(p.root_chain_pref == (prefs.root_chain ? 1 : 0));
  int npair = 0, nsord = 0;
  for (int l = 1; l < L; ++l) {
    npair += p.lv[l].pair == 1;
    nsord += p.lv[l].sord;
    if (p.lv[l].pair == 1) CHECK(l + 1 < L && p.lv[l + 1].pair == 2 && p.lv[l + 1].chunk0 == p.lv[l].chunk0 + p.lv[l].nchunk);
  }
  CHECK(npair == p.npairs && nsord == p.nsord);
}

static Shape shape(const char* name, int S, int P, int kind, int rooted) {
  Shape sh{name, S, P, rooted, make_peel(S, kind, rooted != 0), std::vector<uint8_t>((size_t)S * P), std::vector<double>(P)};
  for (auto& t : sh.tips) t = rnd(16) == 0 ? 15 : (uint8_t)(1 << rnd(4));
  for (auto& x : sh.w) x = 1 + rnd(5);
  return sh;
}

int main() {
  std::vector<Shape> shapes;
  for (int S : {3, 4})  // no clade level, no chain
    for (int kind = 0; kind < 2; ++kind)
      for (int rooted = 0; rooted < 2; ++rooted)
        for (int P : {1, 7, 70}) shapes.push_back(shape("tiny", S, P, kind, rooted));
  shapes.push_back(shape("caterpillar12", 12, 150, 0, 1));  // a chain hitting CHAIN_MAX
  shapes.push_back(shape("caterpillar12u", 12, 150, 0, 0));
  shapes.push_back(shape("balanced40", 40, 200, 1, 1));  // clades
  shapes.push_back(shape("balanced40u", 40, 257, 1, 0));
  shapes.push_back(shape("random17", 17, 130, 2, 1));
  for (int n : {63, 64, 65}) {  // a cherry, its parent and the root of exactly n classes: chunk and tile edges
    Shape sh = shape("edge", 5, n + 3, 1, 1);
    const int a = sh.peel[0], b = sh.peel[1];  // the first cherry's tips
    for (int i = 0; i < sh.P; ++i)
      for (int t = 0; t < sh.S; ++t)
        sh.tips[(size_t)t * sh.P + i] = t == a ? (uint8_t)(1 + (i % n) % 9) : t == b ? (uint8_t)(1 + (i % n) / 9) : 1;
    shapes.push_back(sh);
  }
  {  // 48 x 5,000, 90 % one state: segments crossing more than SPAN_LANE_MAX tiles
    Shape sh = shape("repetitive", 48, 5000, 2, 1);
    const uint8_t other[5] = {1, 2, 4, 8, 15};
    for (auto& t : sh.tips) t = rnd(10) < 9 ? 1 : other[rnd(5)];
    shapes.push_back(sh);
  }
  {  // duplicate columns share a root class
    Shape sh = shape("duplicates", 10, 100, 2, 1);
    for (int i = 80; i < 100; ++i)
      for (int t = 0; t < 10; ++t) sh.tips[(size_t)t * 100 + i] = sh.tips[(size_t)t * 100 + i - 80];
    shapes.push_back(sh);
  }
  std::vector<ClassPrefs> knobs(11);
  knobs[1].clade = 0;
  knobs[2].clade = 3;
  knobs[3].chain = false;
  knobs[4].pair = false;
  knobs[5].pair_max = 100;
  knobs[6].revfix = false;
  knobs[7].stage_order = 0;
  knobs[8].stage_order = 1ll << 40;
  knobs[9].root_wgs = 1;
  knobs[10].clade = 0;  // every level launched on its own, no chain: the long spans reach lfix / clong
  knobs[10].chain = false;
  knobs[10].root_chain = false;
  long plans = 0;
  long long long_rep = 0, clong_rep = 0, lfix_rep = 0;
  for (const Shape& sh : shapes) {
    g_what = sh.name;
    Problem pb;
    if (make_problem(sh.S, sh.P, 4, sh.rooted, PHY_GTR, sh.tips.data(), sh.w.data(), sh.peel.data(), 1, pb) != PHY_OK) {
      std::fprintf(stderr, "FAIL %s: make_problem: %s\n", sh.name, g_err.c_str());
      ++g_bad;
      continue;
    }
    const std::vector<int> naive = naive_classes(sh, pb.vec_of);
    const bool rep = std::string(sh.name) == "repetitive";
    for (const ClassPrefs& prefs : knobs) {
      ClassPlan p;
      const int rc = class_plan(sh.S, sh.P, 4, sh.rooted, sh.tips.data(), sh.w.data(), sh.peel.data(), pb.vec_of, pb.R,
                                pb.nmat, pb.gpos, prefs, p);
      if (rc != PHY_OK) {
        std::fprintf(stderr, "FAIL %s: class_plan: %s\n", sh.name, g_err.c_str());
        ++g_bad;
        continue;
      }
      long long longs = 0;
      check_plan(sh, pb, prefs, p, naive, longs);
      (void)class_plan_tables(p);
      if (rep) long_rep += longs, clong_rep += p.nclong, lfix_rep += (long long)p.lfix.size();
      if (std::string(sh.name) == "caterpillar12" && prefs.clade == 0 && prefs.chain && p.chain_m != CHAIN_MAX) {
        std::fprintf(stderr, "FAIL caterpillar12: chain of %d levels, not CHAIN_MAX\n", p.chain_m);
        ++g_bad;
      }
      if (std::string(sh.name) == "duplicates" && p.nroot > 80) {
        std::fprintf(stderr, "FAIL duplicates: %d root classes of 80 distinct columns\n", p.nroot);
        ++g_bad;
      }
      ++plans;
    }
  }
  if (!long_rep || !clong_rep || !lfix_rep) {  // the repetitive shape must reach the long-span tables
    std::fprintf(stderr, "FAIL repetitive: long spans %lld, lfix %lld, clong %lld\n", long_rep, lfix_rep, clong_rep);
    ++g_bad;
  }
  std::printf("class_plan_check: %ld plans, %d failures\n", plans, g_bad);
  return g_bad ? 1 : 0;
}
