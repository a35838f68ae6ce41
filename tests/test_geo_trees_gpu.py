"""GPU: the tree-sample (mixture) phylogeography engine, ``phy_geo_trees_*``,
through ``geo.GeoTreesLikelihood`` (ctypes on the C-ABI), against the truth of
tests/geo_trees_truth.py: per tree the complex log L_t from expm(Q t), combined
by a complex log-sum-exp with log w_t, every derivative Im f(theta + 1e-30 i) /
1e-30; summaries: the p_t-weighted Minin-Suchard counts and root marginals.

Bars (the project's): log L_mix and each finite ``tree_ll`` entry at relative
1e-10; each gradient array, ``jumps`` and ``root`` within 1e-9 of the array's
largest entry; at K = 2 the rate gradient is exactly zero and is compared
absolutely, <= 1e-12.  Where an array is long a seeded subset of its entries is
compared with the truth and the whole array with the host restatement
(``geo.geo_trees_host`` / ``geo_trees_summaries_host``, which
tests/test_geo_trees_cpu.py pins to the truth) at the same bar.

Samples larger than a handful of trees cycle through a pool of distinct trees
with distinct weights: the mixture equals the pool's with each tree's weights
summed, so the truth costs the pool and the device still runs every tree.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from phylostan_amd import _lib, data as dataio, geo
from tests import cases
from tests import geo_oracle as go
from tests import geo_summary_truth as gst
from tests import geo_trees_truth as gt

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_BAR, GRAD_BAR, K2_RATE_BAR = 1e-10, 1e-9, 1e-12


def logsumexp(x):
    x = np.asarray(x, float)
    m = x.max()
    return m + np.log(np.exp(x - m).sum())


def pooled(peels, blens, logw, T):
    """A T-tree sample cycling through the pool: (peels, blens, logw [T], cls
    [T], pool weights): tree t is pool tree t % n with its own weight."""
    n = len(peels)
    cls = np.arange(T) % n
    pw = np.asarray([logsumexp(logw[cls == d]) if np.any(cls == d) else -np.inf for d in range(n)])
    return peels[cls], blens[cls], cls, pw


def check_rows(rows_tll, tips, peels, blens, params, logw, entries, extended=False, cls=None, seed=0):
    """One draw's (row, tree_ll) against the truth and the host restatement on
    the sample ``peels / blens / logw`` (the pool, when ``cls`` maps the device's
    trees to it)."""
    row, tll = rows_tll
    K = tips.shape[1]
    R = geo.rate_count(K)
    rates, freqs = params[:R], params[R:]
    ll, gr, gf = row[0], row[1:1 + R], row[1 + R:]
    tl, tlls, tg = gt.mix_truth_gradients(tips, peels, blens, rates, freqs, logw, extended=extended,
                                          max_entries=entries, seed=seed)
    _, hr, hf, _ = geo.geo_trees_host(tips, peels, blens, rates, freqs, logw)
    print("S %d K %d T %d: log L_mix %.12g truth %.12g rel %.2e" % (tips.shape[0], K, len(tll), ll, tl, abs(ll - tl) / abs(tl)))
    assert abs(ll - tl) <= LL_BAR * abs(tl)
    want_tll = tlls if cls is None else tlls[cls]
    assert np.all(np.abs(tll - want_tll) <= LL_BAR * np.abs(want_tll))
    for name, got, host in (("rates", gr, hr), ("freqs", gf, hf)):
        idx, want = tg[name]
        scale = np.abs(host).max()
        e_truth, e_host = np.abs(got[idx] - want).max(), np.abs(got - host).max()
        print("  d/d%s: |max| %.3e, vs truth %.2e, vs host %.2e" % (name, scale, e_truth, e_host))
        if name == "rates" and K == 2:
            assert e_truth <= K2_RATE_BAR and np.abs(got).max() <= K2_RATE_BAR
            continue
        assert e_truth <= GRAD_BAR * scale, name
        assert e_host <= GRAD_BAR * scale, name
    return tlls


def check_summaries(jumps, root, tips, peels, blens, params, logw, tlls, entries, seed=0):
    """jumps and root against the truth (every entry for ``entries`` None, else
    that many seeded entries of jumps) and the host restatement."""
    K = tips.shape[1]
    R = geo.rate_count(K)
    rates, freqs = params[:R], params[R:]
    p = gt.tree_weights(tlls, logw)
    hj, hr = geo.geo_trees_summaries_host(tips, peels, blens, rates, freqs, logw)
    pairs = [(i, j) for i in range(K) for j in range(K)]
    if entries is not None and len(pairs) > entries:
        rng = np.random.default_rng(seed)
        pairs = [pairs[k] for k in np.sort(rng.choice(len(pairs), entries, replace=False))]
    want = {pq: 0.0 for pq in pairs}
    troot = np.zeros(K)
    for t in range(len(peels)):
        if p[t] == 0.0:
            continue
        for pq, v in gst.jump_truth(tips, peels[t], blens[t], rates, freqs, entries=pairs).items():
            want[pq] += p[t] * v
        troot += p[t] * gt.root_truth(tips, peels[t], blens[t], rates, freqs)
    scale = np.abs(hj).max()
    e_truth = max(abs(jumps[pq] - v) for pq, v in want.items())
    print("  jumps: |max| %.3e, vs truth %.2e, vs host %.2e; root vs truth %.2e"
          % (scale, e_truth, np.abs(jumps - hj).max(), np.abs(root - troot).max()))
    assert e_truth <= GRAD_BAR * scale
    assert np.abs(jumps - hj).max() <= GRAD_BAR * scale
    assert np.abs(root - troot).max() <= GRAD_BAR * troot.max()
    assert np.abs(root - hr).max() <= GRAD_BAR * troot.max()


@functools.lru_cache(maxsize=None)
def flu_peel():
    tree = dataio.read_tree(os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.tree"))
    tree.resolve_polytomies(update_bipartitions=True)
    dataio.setup_indexes(tree)
    peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
    return peel0, geo.tree_branch_lengths(tree, peel0)


@functools.lru_cache(maxsize=None)
def resident_workgroups(K=5):
    """The tree phase's grid cap on this device at S = 7 (the workspace budget
    does not bind) and K states (the LDS plan admits two workgroups per CU up
    to K = 45 or so, one at K = 64): G = min(T, this)."""
    tips, peels, blens, _ = gt.make_sample(7, K, 1, 1)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=1)
    try:
        info = eng.info()
    finally:
        eng.close()
    assert info["groups"] == 1 and info["workgroups"] >= 1
    return info["workgroups"]


# ---------------------------------------------------------------- 1. one tree is the single-tree engine
@pytest.mark.parametrize("S,K", [(3, 3), (7, 5), (69, 33)])
def test_one_tree_is_phy_geo_eval(S, K):
    rng = np.random.default_rng(10 * S + K)
    if S == 69:
        peel, tree_blens = flu_peel()
        blens = tree_blens * (0.3 / tree_blens.mean())
    else:
        peel = go.random_peel(S, rng)
        blens = rng.exponential(0.3, 2 * S - 3)
    blens[1] = 0.0
    tips = go.random_tips(S, K, rng, missing=(0,))
    _, params = go.random_draws(3, 2 * S - 3, K, rng)
    B, R = 2 * S - 3, geo.rate_count(K)
    one = geo.GeoLikelihood(tips, peel, max_draws=3)
    eng = geo.GeoTreesLikelihood(tips, peel[None], blens[None], max_draws=3)
    try:
        old, marg, ojumps, _ = one.evaluate_summaries(np.tile(blens, (3, 1)), params)
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik
        assert eng.info()["groups"] == 1 and eng.T == 1 and eng.outlen == 1 + R + K
    finally:
        one.close()
        eng.close()
    for n in range(3):
        assert abs(rows[n, 0] - old[n, 0]) <= LL_BAR * abs(old[n, 0])
        assert abs(tll[n, 0] - old[n, 0]) <= LL_BAR * abs(old[n, 0])  # w = 1: the mixture is the tree
        for got, want in ((rows[n, 1:1 + R], old[n, 1 + B:1 + B + R]), (rows[n, 1 + R:], old[n, 1 + B + R:]),
                          (jumps[n], ojumps[n]), (root[n], marg[n, 2 * S - 2])):
            assert np.abs(got - want).max() <= GRAD_BAR * np.abs(want).max()
            # both engines run the phases of geo_phases.inc and the tree's weight is 1: the same bits
            # (profiles/geo_shared_phases_ab.json, one_tree_equals_single_tree_engine)
            assert np.array_equal(got, want)
        assert rows[n, 0] == old[n, 0] and tll[n, 0] == old[n, 0]


# ---------------------------------------------------------------- 2. mixed topologies
@pytest.mark.parametrize("S,K,T,missing,entries", [
    (4, 2, 3, (0,), None), (4, 2, 3, (), None), (4, 3, 3, (0,), None), (4, 3, 3, (), None),
    (7, 5, 7, (0, 3), None), (7, 5, 7, (), None), (7, 17, 7, (0,), 3), (7, 17, 7, (), 3),
    (69, 64, 5, (0, 11), 1)])
def test_mixed_topologies(S, K, T, missing, entries):
    peels = None
    if S == 69:  # fluA's tree and four random topologies on its tips
        rng = np.random.default_rng(69)
        peels = np.stack([flu_peel()[0]] + [go.random_peel(S, rng) for _ in range(T - 1)])
    tips, peels, blens, params = gt.make_sample(S, K, T, 2000 + 10 * S + K + len(missing), missing=missing, peels=peels)
    logw = np.log(np.random.default_rng(T + K).dirichlet(np.ones(T) * 2.0))
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=2)
    try:
        assert eng.info()["groups"] == min(T, resident_workgroups(K))
        if S == 7:
            assert eng.info()["max_levels"] == S - 1 and eng.info()["widest_level"] >= 3  # caterpillar and balanced
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    tlls = check_rows((rows[0], tll[0]), tips, peels, blens, params, logw, entries)
    check_summaries(jumps[0], root[0], tips, peels, blens, params, logw, tlls, None if K <= 5 else 2 if K < 64 else 1)


# ---------------------------------------------------------------- 3. more trees than groups
@functools.lru_cache(maxsize=None)
def pool_case(K):
    S, n = 7, 7
    tips, peels, blens, params = gt.make_sample(S, K, n, 3000 + K)
    return tips, peels, blens, params


@pytest.mark.parametrize("K", [5, 64])
@pytest.mark.parametrize("which", ["G-1", "G", "G+1", "2G+1", "300"])
def test_more_trees_than_groups(K, which):
    W = resident_workgroups(K)
    T = {"G-1": max(W - 1, 1), "G": W, "G+1": W + 1, "2G+1": 2 * W + 1, "300": 300}[which]
    tips, ppeels, pblens, params = pool_case(K)
    logw = np.random.default_rng(T).normal(0.0, 3.0, T) - np.log(T)
    peels, blens, cls, pw = pooled(ppeels, pblens, logw, T)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=2)
    try:
        info = eng.info()
        assert info["groups"] == min(T, W) and info["workgroups"] == W
        rows, jumps, root = eng.evaluate_summaries(np.stack([params, params]))
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    assert rows[0].tobytes() == rows[1].tobytes() and tll[0].tobytes() == tll[1].tobytes()
    live = np.isfinite(pw)  # on a device of fewer than 8 workgroups G - 1 trees do not reach every pool tree
    for d in range(len(ppeels)):  # the copies of a pool tree, in whatever group they fall, are the same bits
        assert len(set(tll[0][cls == d].tolist())) <= 1
    tlls = check_rows((rows[0], tll[0]), tips, ppeels[live], pblens[live], params, pw[live], 2 if K > 5 else None,
                      cls=np.cumsum(live)[cls] - 1, seed=T)
    check_summaries(jumps[0], root[0], tips, ppeels[live], pblens[live], params, pw[live], tlls, None if K <= 5 else 2)


# ---------------------------------------------------------------- 4. extreme weights
def test_a_term_that_underflows_is_exactly_zero():
    S, K, T = 7, 3, 4
    tips, peels, blens, params = gt.make_sample(S, K, T, 41)
    logw = np.log([0.3, 0.3, 0.4, 1.0])
    logw[1] = -800.0
    keep = [0, 2, 3]
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    sub = geo.GeoTreesLikelihood(tips, peels[keep], blens[keep], log_weights=logw[keep], max_draws=1)
    try:
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
        rows3, jumps3, root3 = sub.evaluate_summaries(params)
    finally:
        eng.close()
        sub.close()
    assert np.all(np.isfinite(tll))  # the tree has a likelihood, its weighted term has not
    assert eng.tree_posterior(rows)[0, 1] == 0.0
    assert rows.tobytes() == rows3.tobytes() and jumps.tobytes() == jumps3.tobytes() and root.tobytes() == root3.tobytes()
    tlls = check_rows((rows[0], tll[0]), tips, peels, blens, params, logw, None)
    check_summaries(jumps[0], root[0], tips, peels, blens, params, logw, tlls, None)


@pytest.mark.parametrize("gap", [30.0, 700.0, 760.0])
def test_the_dominant_tree_is_last_in_its_group(gap):
    """2G + 1 trees, so every group walks two or three; the last tree of every
    group outweighs those before it by e^gap: the running maximum rises at the
    end of each walk and the sums so far are rescaled (at 760 to exactly 0)."""
    S, K = 7, 3
    W = resident_workgroups(K)
    T = 2 * W + 1
    tips, ppeels, pblens, params = gt.make_sample(S, K, 7, 42)
    G = min(T, W)
    start = [(g * T) // G for g in range(G + 1)]  # phylo_hip_diag.h: group g walks trees start[g] .. start[g + 1] - 1
    logw = np.full(T, -gap - np.log(T))
    logw[np.asarray(start[1:]) - 1] = -np.log(T)
    logw += np.random.default_rng(int(gap)).normal(0.0, 0.5, T)
    peels, blens, cls, pw = pooled(ppeels, pblens, logw, T)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        assert eng.info()["groups"] == G
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    tlls = check_rows((rows[0], tll[0]), tips, ppeels, pblens, params, pw, None, cls=cls)
    check_summaries(jumps[0], root[0], tips, ppeels, pblens, params, pw, tlls, None)


def test_weights_far_below_the_fp64_range():
    S, K, T = 7, 3, 4
    tips, peels, blens, params = gt.make_sample(S, K, T, 43)
    logw = np.full(T, -1500.0) + np.log([0.1, 0.2, 0.3, 0.4])
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    assert np.isfinite(rows).all() and rows[0, 0] < -1500.0 and np.exp(rows[0, 0]) == 0.0
    tlls = check_rows((rows[0], tll[0]), tips, peels, blens, params, logw, None, extended=True)
    check_summaries(jumps[0], root[0], tips, peels, blens, params, logw, tlls, None)


def test_two_600_tip_trees_past_the_fp64_range():
    S, K, T = 600, 8, 2
    rng = np.random.default_rng(600)
    peels = np.stack([go.random_peel(S, rng), go.random_peel(S, rng)])
    tips = go.random_tips(S, K, rng)
    blens = rng.exponential(0.3, (T, 2 * S - 3))
    _, params = go.random_draws(1, 2 * S - 3, K, rng)
    params = params[0]
    R = geo.rate_count(K)
    with np.errstate(divide="ignore"):
        plain = go.truth(tips, peels[0], blens[0], params[:R], params[R:]).real
    assert plain == -np.inf, "the plain truth must underflow on this input: enlarge S"
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=1)
    try:
        rows = eng.evaluate_rows(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    assert np.isfinite(rows).all() and rows[0, 0] < np.log(np.finfo(np.float64).tiny)
    check_rows((rows[0], tll[0]), tips, peels, blens, params, gt.uniform_logw(T), 4, extended=True)


# ---------------------------------------------------------------- 5. ties and near ties
@pytest.mark.parametrize("arm", ["tie", "near"])
def test_repeated_eigenvalues(arm):
    """Equal rates and frequencies: a (K-1)-fold eigenvalue (Phi's tie arm); one rate moved by 1e-11: its near arm."""
    S, K, T = 9, 5, 3
    tips, peels, blens, _ = gt.make_sample(S, K, T, 900 + K)
    rates = np.ones(geo.rate_count(K))
    if arm == "near":
        rates[1] += 1e-11
    params = np.concatenate([rates, np.full(K, 1.0 / K)])
    logw = np.log([0.5, 0.2, 0.3])
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    tlls = check_rows((rows[0], tll[0]), tips, peels, blens, params, logw, 5)
    check_summaries(jumps[0], root[0], tips, peels, blens, params, logw, tlls, None)


# ---------------------------------------------------------------- 6. bitwise
def test_rows_do_not_depend_on_the_batch():
    S, K, T, n = 7, 5, 7, 300
    tips, peels, blens, _ = gt.make_sample(S, K, T, 61)
    _, params = go.random_draws(n, 2 * S - 3, K, np.random.default_rng(62))
    big = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=n)
    four = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=4)
    one = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=1)
    try:
        assert n * big.info()["groups"] > big.info()["workgroups"]  # the 300-draw call loops
        rows, jumps, root = big.evaluate_summaries(params)
        tll = big.tree_loglik.copy()
        plain = big.evaluate_rows(params)
        assert plain.tobytes() == rows.tobytes() and big.tree_loglik.tobytes() == tll.tobytes()
        again = big.evaluate_summaries(params)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(again, (rows, jumps, root)))
        for k in (0, 150, 299):
            r1, j1, o1 = one.evaluate_summaries(params[k])
            assert r1[0].tobytes() == rows[k].tobytes() and one.tree_loglik[0].tobytes() == tll[k].tobytes(), k
            assert j1[0].tobytes() == jumps[k].tobytes() and o1[0].tobytes() == root[k].tobytes(), k
            batch = np.stack([params[5], params[9], params[k], params[7]])  # as draw 3 of 4
            r4, j4, o4 = four.evaluate_summaries(batch)
            assert r4[2].tobytes() == rows[k].tobytes() and four.tree_loglik[2].tobytes() == tll[k].tobytes(), k
            assert j4[2].tobytes() == jumps[k].tobytes() and o4[2].tobytes() == root[k].tobytes(), k
    finally:
        big.close()
        four.close()
        one.close()
    assert np.isfinite(rows).all()


def test_rows_do_not_depend_on_the_chunk_of_draws():
    """K = 64 and more trees than groups: a call's (draw, group) slots pass their
    budget, so the draws run in chunks; a draw of a later chunk is bitwise the
    draw alone."""
    S, K, n = 7, 64, 40
    W = resident_workgroups(K)
    T = W + 44
    tips, ppeels, pblens, _ = pool_case(K)
    logw = np.random.default_rng(7).normal(0.0, 1.0, T) - np.log(T)
    peels, blens, _, _ = pooled(ppeels, pblens, logw, T)
    _, params = go.random_draws(n, 2 * S - 3, K, np.random.default_rng(64))
    big = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=n)
    one = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        rows = big.evaluate_rows(params)
        tll = big.tree_loglik.copy()
        for k in (0, n - 1):
            alone = one.evaluate_rows(params[k])
            assert alone[0].tobytes() == rows[k].tobytes() and one.tree_loglik[0].tobytes() == tll[k].tobytes(), k
    finally:
        big.close()
        one.close()
    assert np.isfinite(rows).all()


# ---------------------------------------------------------------- 7. failure rows and refusals
def test_a_bad_draw_does_not_touch_its_neighbours():
    S, K, T = 7, 4, 5
    tips, peels, blens, params = gt.make_sample(S, K, T, 71)
    R = geo.rate_count(K)
    batch = np.tile(params, (4, 1))
    batch[1, 2] = np.nan        # a NaN rate
    batch[2, R + 1] = 0.0       # a zero frequency
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=4)
    try:
        alone = eng.evaluate_summaries(params)
        tll1 = eng.tree_loglik.copy()
        rows, jumps, root = eng.evaluate_summaries(batch)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    for k in (1, 2):
        assert rows[k, 0] == -np.inf and np.all(rows[k, 1:] == 0.0) and np.all(tll[k] == -np.inf)
        assert not jumps[k].any() and not root[k].any()
    for k in (0, 3):
        assert rows[k].tobytes() == alone[0][0].tobytes() and tll[k].tobytes() == tll1[0].tobytes()
        assert jumps[k].tobytes() == alone[1][0].tobytes() and root[k].tobytes() == alone[2][0].tobytes()
    assert np.isfinite(rows[0]).all()


def test_a_tree_without_likelihood_has_no_weight():
    """A branch of -1e6 (finite, so the context takes it) on tree 0: e^{lam t}
    overflows and that tree's likelihood is not finite, for that tree alone.
    A tip whose partial is all zeros: L = 0 on every tree."""
    S, K = 4, 3
    tips = np.eye(K)[[0, 1, 2, 0]]
    rng = np.random.default_rng(3)
    blens = rng.exponential(0.3, (3, 5))
    blens[0, 2] = -1e6
    _, params = go.random_draws(1, 5, K, rng)
    logw = gt.uniform_logw(3)
    dead = tips.copy()
    dead[3] = 0.0
    eng = geo.GeoTreesLikelihood(tips, gt.S4_PEELS, blens, max_draws=1)
    none = geo.GeoTreesLikelihood(dead, gt.S4_PEELS[1:], blens[1:], max_draws=1)
    try:
        rows, jumps, root = eng.evaluate_summaries(params[0])
        tll = eng.tree_loglik.copy()
        r0, j0, o0 = none.evaluate_summaries(params[0])
        t0 = none.tree_loglik.copy()
    finally:
        eng.close()
        none.close()
    assert tll[0, 0] == -np.inf and np.all(np.isfinite(tll[0, 1:]))
    tlls = check_rows((rows[0], tll[0, 1:]), tips, gt.S4_PEELS[1:], blens[1:], params[0], logw[1:], None)
    check_summaries(jumps[0], root[0], tips, gt.S4_PEELS[1:], blens[1:], params[0], logw[1:], tlls, None)
    # every tree without a likelihood: the draw's failure row
    assert r0[0, 0] == -np.inf and not r0[0, 1:].any() and np.all(t0 == -np.inf) and not j0.any() and not o0.any()


def test_refusals():
    S, K, T = 7, 4, 3
    tips, peels, blens, params = gt.make_sample(S, K, T, 72)
    lib = _lib.load()
    PHY_EINVAL, PHY_ERANGE = 1, 4
    ctx = ctypes.c_void_p()
    i32 = np.ascontiguousarray(peels, np.int32)

    def create(tips_p=tips.ctypes.data, t=T, k=K, peels_p=None, blens_p=blens.ctypes.data, lw=None, out=ctypes.byref(ctx)):
        return lib.phy_geo_trees_create(S, k, tips_p, t, i32.ctypes.data if peels_p is None else peels_p, blens_p, lw, 2,
                                        0, out)

    assert create(tips_p=None) == PHY_EINVAL and create(blens_p=None) == PHY_EINVAL and create(out=None) == PHY_EINVAL
    assert lib.phy_geo_trees_create(S, K, tips.ctypes.data, T, None, blens.ctypes.data, None, 2, 0,
                                    ctypes.byref(ctx)) == PHY_EINVAL
    assert create(t=0) == PHY_EINVAL and b"T = 0" in lib.phy_last_error()
    with pytest.raises(_lib.PhyloHipError, match=r"tree 0: .*supported 2..64"):
        geo.GeoTreesLikelihood(np.ones((S, 65)), peels, blens)
    bad = peels.copy()
    bad[2, 1, 0] = bad[2, 0, 0]
    with pytest.raises(_lib.PhyloHipError, match=r"tree 2: .*(already has a parent|before it is computed)"):
        geo.GeoTreesLikelihood(tips, bad, blens)
    for w in (np.nan, np.inf, -np.inf):
        with pytest.raises(_lib.PhyloHipError, match=r"tree 1: log weight"):
            geo.GeoTreesLikelihood(tips, peels, blens, log_weights=[0.0, w, 0.0])
    for v in (np.nan, np.inf):
        b2 = blens.copy()
        b2[1, 4] = v
        with pytest.raises(_lib.PhyloHipError, match=r"tree 1: branch length 4"):
            geo.GeoTreesLikelihood(tips, peels, b2)
    with pytest.raises(_lib.PhyloHipError, match=r"\[0, 1\]"):
        geo.GeoTreesLikelihood(tips * 2.0, peels, blens)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=2)
    try:
        with pytest.raises(_lib.PhyloHipError, match="n_draws out of range"):
            eng.evaluate_rows(np.tile(params, (3, 1)))
        out = np.empty((1, eng.outlen))
        assert lib.phy_geo_trees_eval(eng.ctx, 0, params.ctypes.data, out.ctypes.data, None) == PHY_ERANGE
        assert lib.phy_geo_trees_eval(eng.ctx, 1, None, out.ctypes.data, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval(eng.ctx, 1, params.ctypes.data, None, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval_summaries(eng.ctx, 1, params.ctypes.data, None, None, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval(None, 1, params.ctypes.data, out.ctypes.data, None) == PHY_EINVAL
        # tree_ll and out are optional where the header says so
        assert lib.phy_geo_trees_eval(eng.ctx, 1, params.ctypes.data, out.ctypes.data, None) == 0
        flat = np.empty((1, K * K + K))
        assert lib.phy_geo_trees_eval_summaries(eng.ctx, 1, params.ctypes.data, None, None, flat.ctypes.data) == 0
        assert out[0].tobytes() == eng.evaluate_rows(params)[0].tobytes()
        assert lib.phy_geo_trees_num_trees(eng.ctx) == T and lib.phy_geo_trees_summary_len(eng.ctx) == K * K + K
    finally:
        eng.close()
    assert lib.phy_geo_trees_output_len(None) == -1 and lib.phy_geo_trees_num_trees(None) == -1
    assert lib.phy_geo_trees_summary_len(None) == -1


# ---------------------------------------------------------------- 8. identities
@pytest.mark.parametrize("S,K,T", [(7, 5, 7), (69, 20, 9)])
def test_identities(S, K, T):
    rng = np.random.default_rng(80 + S)
    peels = np.stack([go.random_peel(S, rng) for _ in range(T)])
    tips, peels, blens, _ = gt.make_sample(S, K, T, 81 + S, peels=peels)
    _, params = go.random_draws(3, 2 * S - 3, K, rng)
    logw = np.log(rng.dirichlet(np.ones(T)))
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=3)
    try:
        rows, jumps, root = eng.evaluate_summaries(params)
        p = eng.tree_posterior(rows)
    finally:
        eng.close()
    assert np.all(np.abs(p.sum(1) - 1.0) <= 1e-10)
    assert np.all(np.abs(root.sum(1) - 1.0) <= 1e-12)
    times = np.trace(jumps, axis1=1, axis2=2)
    assert np.all(np.abs(times - p @ blens.sum(1)) <= 1e-9 * blens.sum(1).max())


# ---------------------------------------------------------------- the DS1 topologies
def test_all_42_ds1_topologies():
    """tests/golden/DS1_topologies.npz: the reference's 42 DS1 trees, each in
    its own tip order.  ``data.unrooted_peel`` brings every peel into the geo
    convention; tip ids go through ``perm`` to one numbering.  Seeded branch
    lengths and locations, K = 5."""
    D = np.load(os.path.join(cases.GOLDEN, "DS1_topologies.npz"), allow_pickle=False)
    T, S, K = D["peel"].shape[0], 27, 5
    peels = np.zeros((T, S - 1, 3), np.int32)
    for k in range(T):
        p = np.asarray(dataio.unrooted_peel(D["peel"][k].tolist()), np.int32) - 1
        tip = p < S
        p[tip] = D["perm"][k][p[tip]]
        peels[k] = p
    assert len({peels[k].tobytes() for k in range(T)}) == T
    tips, peels, blens, params = gt.make_sample(S, K, T, 42, peels=peels, mean_blen=0.1)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=1)
    try:
        assert eng.info()["groups"] == min(T, resident_workgroups(K))
        rows, jumps, root = eng.evaluate_summaries(params)
        tll = eng.tree_loglik.copy()
    finally:
        eng.close()
    logw = gt.uniform_logw(T)
    tlls = check_rows((rows[0], tll[0]), tips, peels, blens, params, logw, 2)
    check_summaries(jumps[0], root[0], tips, peels, blens, params, logw, tlls, 3)


# ---------------------------------------------------------------- 9. the CLI on the device
def test_cli_run_geo_trees_on_the_engine(tmp_path):
    """run --geo --trees -a vb --ancestral, S = 30, K = 3, T = 8, on the device engine."""
    from tests.test_geo_trees_cpu import write_dataset
    tree, meta, sample = write_dataset(tmp_path, 30, 3, 8, 30)
    out = str(tmp_path / "geo")
    post, lines = go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree, "--trees",
                              sample, "-o", out, "-S", "11", "--eta", "0.1", "--iter", "100", "--elbo_samples", "10",
                              "--samples", "20", "--tol_rel_obj", "0.01"], host=False)
    assert isinstance(post.trees, geo.GeoTreesLikelihood) and post.trees.T == 8
    for ext in ("", ".diag", ".jumps.tsv", ".root.tsv", ".treeprob.tsv"):
        assert os.path.exists(out + ext), ext
    assert not os.path.exists(out + ".trees")
    rows = [ln.rstrip("\n").split("\t") for ln in open(out + ".treeprob.tsv")][1:]
    assert [r[0] for r in rows] == [str(t) for t in range(8)]
    assert abs(sum(float(r[1]) for r in rows) - 1.0) <= 1e-12
    rows = [ln.rstrip("\n").split("\t") for ln in open(out + ".root.tsv")][1:]
    assert abs(sum(float(r[1]) for r in rows) - 1.0) <= 1e-12
    assert len([s for s in lines if s.startswith("Expected migrations")]) == 1
