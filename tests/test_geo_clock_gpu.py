"""GPU: the trait clock rate on the tree-sample engine,
``phy_geo_trees_eval_clock`` / ``phy_geo_trees_eval_clock_summaries`` through
``geo.GeoTreesLikelihood``, and ``GeoLikelihood.evaluate_rows_clock`` on the
single-tree engine.

Truth and bars: tests/geo_clock_truth.py (the expm truths at ``mu * blens``,
d/dmu by the complex step on mu; log L at relative 1e-10, each gradient array
at 1e-9 of its largest entry, d/dmu at 1e-9 of max(|truth|, the size of the
terms that cancel in it)).  The bitwise tests pin the rule that the effective
length ``mu * t`` is one fp64 product formed before anything else uses it: a
context on ``blens`` at mu gives the bits of a context on the numpy product.
"""
import ctypes
import functools
import os

import numpy as np
import pytest

from phylostan_amd import _lib, geo, stan_io
from tests import geo_clock_truth as gc
from tests import geo_oracle as go
from tests import geo_trees_truth as gt
from tests.test_geo_trees_gpu import flu_peel, pooled

pytestmark = pytest.mark.gpu

MUS = (2.0 ** -5, 0.03, 1.7, 40.0)


@functools.lru_cache(maxsize=None)
def groups_cap(S, K):
    """G of a context with more trees than the tree phase has workgroups."""
    tips, peels, blens, _ = gt.make_sample(S, K, 1, 1)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=1)
    try:
        return eng.info()["workgroups"]
    finally:
        eng.close()


@functools.lru_cache(maxsize=None)
def sample(S, K, which):
    """(tips, peels, blens, logw, params [9, R + K]) of T trees, T a number or
    'G+1' / '2G+1'; past seven trees the sample cycles through a pool of seven
    with distinct weights."""
    T = which if isinstance(which, int) else {"G+1": 1, "2G+1": 2}[which] * groups_cap(S, K) + 1
    n = min(T, 7)
    tips, ppeels, pblens, _ = gt.make_sample(S, K, n, 7000 + 10 * S + K)
    rng = np.random.default_rng(T + K)
    logw = rng.normal(0.0, 1.0, T) - np.log(T)
    peels, blens, _, _ = pooled(ppeels, pblens, logw, T)
    _, params = go.random_draws(9, 2 * S - 3, K, rng)
    return tips, np.ascontiguousarray(peels), np.ascontiguousarray(blens), logw, params


def off_diagonal(K):
    return ~np.eye(K, dtype=bool)


def both_calls(eng, params, mu):
    """The clock rows of evaluate_rows_clock and evaluate_summaries_clock, which must be the same bits."""
    rows = eng.evaluate_rows_clock(params, mu)
    tll = eng.tree_loglik.copy()
    rows2, jumps, root = eng.evaluate_summaries_clock(params, mu)
    assert rows.tobytes() == rows2.tobytes() and tll.tobytes() == eng.tree_loglik.tobytes()
    return rows, tll, jumps, root


# ---------------------------------------------------------------- 1. mu = 1 is the plain call
@pytest.mark.parametrize("S,K,which", [(3, 2, 1), (7, 5, 7), (9, 64, "2G+1")])
def test_unit_rate_is_the_plain_call(S, K, which):
    tips, peels, blens, logw, params = sample(S, K, which)
    R = geo.rate_count(K)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=2)
    try:
        assert eng.lib.phy_geo_trees_clock_output_len(eng.ctx) == 2 + R + K == eng.outlen + 1
        plain, pj, pr = eng.evaluate_summaries(params[:2])
        ptll = eng.tree_loglik.copy()
        rows, tll, jumps, root = both_calls(eng, params[:2], np.ones(2))
        again = eng.evaluate_rows(params[:2])  # the plain call after the clock calls: the bits it had
    finally:
        eng.close()
    assert rows.shape == (2, 2 + R + K) and np.isfinite(rows).all()
    assert rows[:, :1 + R + K].tobytes() == plain.tobytes() and tll.tobytes() == ptll.tobytes()
    assert again.tobytes() == plain.tobytes()
    off = off_diagonal(K)
    assert jumps[:, off].tobytes() == pj[:, off].tobytes() and root.tobytes() == pr.tobytes()
    d, pd = np.diagonal(jumps, axis1=1, axis2=2), np.diagonal(pj, axis1=1, axis2=2)
    assert np.all(np.abs(d - pd) <= 1e-15 * np.abs(pd))


# ---------------------------------------------------------------- 2. a clock is a rescaled tree
@pytest.mark.parametrize("mu", MUS)
@pytest.mark.parametrize("S,K,which", [(7, 5, 7), (9, 64, "G+1")])
def test_a_clock_is_a_rescaled_tree(S, K, which, mu):
    tips, peels, blens, logw, params = sample(S, K, which)
    R = geo.rate_count(K)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=2)
    scaled = geo.GeoTreesLikelihood(tips, peels, mu * blens, log_weights=logw, max_draws=2)
    try:
        rows, tll, jumps, root = both_calls(eng, params[:2], np.full(2, mu))
        plain, pj, pr = scaled.evaluate_summaries(params[:2])
        ptll = scaled.tree_loglik.copy()
    finally:
        eng.close()
        scaled.close()
    assert np.isfinite(rows).all()
    assert rows[:, :1 + R + K].tobytes() == plain.tobytes() and tll.tobytes() == ptll.tobytes()
    off = off_diagonal(K)
    assert jumps[:, off].tobytes() == pj[:, off].tobytes() and root.tobytes() == pr.tobytes()
    d, pd = np.diagonal(jumps, axis1=1, axis2=2), np.diagonal(pj, axis1=1, axis2=2) / mu
    assert np.all(np.abs(d - pd) <= 1e-14 * np.abs(pd))


# ---------------------------------------------------------------- 3. against the truth
CASES = gc.truth_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_against_the_truth(name):
    tips, peels, blens, params, logw, mus, extended, entries = CASES[name]
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=len(mus))
    try:
        rows, tll, jumps, root = both_calls(eng, np.tile(params, (len(mus), 1)), np.asarray(mus))
    finally:
        eng.close()
    for n, mu in enumerate(mus):
        gc.check_clock_row(rows[n], tll[n], tips, peels, blens, params, logw, mu, entries=entries, extended=extended)


# ---------------------------------------------------------------- 4. the two routes to d/dmu
@pytest.mark.parametrize("S,K,T", [(7, 5, 7), (69, 20, 9)])
def test_the_two_routes_to_the_rate_gradient_agree(S, K, T):
    rng = np.random.default_rng(40 + S)
    peels = np.stack([go.random_peel(S, rng) for _ in range(T)])
    tips, peels, blens, _ = gt.make_sample(S, K, T, 41 + S, peels=peels)
    _, params = go.random_draws(3, 2 * S - 3, K, rng)
    logw = np.log(rng.dirichlet(np.ones(T)))
    mus = np.array([0.3, 1.0, 6.0])
    R = geo.rate_count(K)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=3)
    try:
        rows, tll, jumps, root = both_calls(eng, params, mus)
        p = eng.tree_posterior(rows)
    finally:
        eng.close()
    lengths = blens.sum(1)
    for n, mu in enumerate(mus):
        want, wtll = gc.host_clock_row(tips, peels, blens, params[n], logw, mu)
        size = gc.cancelling_size(tips, peels, blens, params[n, :R], params[n, R:], logw, mu, wtll, host=True)
        bar = gc.dmu_bar(want[-1], size)
        print("S %d K %d mu %g: d/dmu %.12g, host %.12g, err %.2e, bar %.2e"
              % (S, K, mu, rows[n, -1], want[-1], abs(rows[n, -1] - want[-1]), bar))
        assert abs(rows[n, -1] - want[-1]) <= bar
        # mu d/dmu = sum_{i != j} jumps_ij + mu sum_i Q_ii dwell_i: every move counted, less what was expected
        Q = geo.rate_matrix(params[n, R:], params[n, :R])[0]
        dwell = np.diag(jumps[n])
        lhs = mu * rows[n, -1]
        moves, expected = jumps[n][off_diagonal(K)].sum(), mu * np.dot(np.diag(Q), dwell)
        print("  mu d/dmu %.12g, moves %.12g + mu sum Q_ii dwell_i %.12g" % (lhs, moves, expected))
        assert abs(lhs - (moves + expected)) <= 1e-9 * max(abs(lhs), abs(moves + expected))
        assert abs(dwell.sum() - p[n] @ lengths) <= 1e-9 * lengths.max()


# ---------------------------------------------------------------- 5. one tree is the single-tree path
@pytest.mark.parametrize("S,K", [(7, 5), (69, 33)])
def test_one_tree_is_the_single_tree_path(S, K):
    rng = np.random.default_rng(50 * S + K)
    if S == 69:
        peel, tree_blens = flu_peel()
        blens = tree_blens * (0.3 / tree_blens.mean())
    else:
        peel = go.random_peel(S, rng)
        blens = rng.exponential(0.3, 2 * S - 3)
    blens[1] = 0.0
    tips = go.random_tips(S, K, rng, missing=(0,))
    _, params = go.random_draws(3, 2 * S - 3, K, rng)
    mus = np.array([0.05, 1.0, 7.5])
    B, R = 2 * S - 3, geo.rate_count(K)
    one = geo.GeoLikelihood(tips, peel, max_draws=3)
    eng = geo.GeoTreesLikelihood(tips, peel[None], blens[None], max_draws=3)
    try:
        old = one.evaluate_rows_clock(np.tile(blens, (3, 1)), params, mus)
        srows, marg, ojumps, _ = one.evaluate_summaries_clock(np.tile(blens, (3, 1)), params, mus)
        rows, tll, jumps, root = both_calls(eng, params, mus)
    finally:
        one.close()
        eng.close()
    assert old.shape == (3, 2 + B + R + K) and old.tobytes() == srows.tobytes()
    for n in range(3):
        print("S %d K %d mu %g: log L %r single-tree %r; d/dmu %.12g single-tree %.12g"
              % (S, K, mus[n], rows[n, 0], old[n, 0], rows[n, -1], old[n, -1]))
        assert rows[n, 0] == old[n, 0] and tll[n, 0] == old[n, 0]
        for got, want in ((rows[n, 1:1 + R], old[n, 1 + B:1 + B + R]), (rows[n, 1 + R:1 + R + K], old[n, 1 + B + R:-1]),
                          (jumps[n], ojumps[n]), (root[n], marg[n, 2 * S - 2])):
            assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        scale = max(abs(old[n, -1]), np.abs(blens * old[n, 1:1 + B] / mus[n]).sum())
        assert abs(rows[n, -1] - old[n, -1]) <= 1e-12 * scale


# ---------------------------------------------------------------- 6. rows do not depend on the batch
NINE = np.array([0.011, 0.07, 0.25, 0.6, 1.0, 1.9, 4.4, 13.0, 55.0])


def test_rows_do_not_depend_on_the_batch():
    S, K = 7, 5
    tips, peels, blens, logw, params = sample(S, K, "2G+1")
    big = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=9)
    one = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        assert big.info()["groups"] == groups_cap(S, K) and big.T == 2 * big.info()["groups"] + 1
        rows, tll, jumps, root = both_calls(big, params, NINE)
        back = both_calls(big, params[::-1], NINE[::-1])
        for a, b in zip(back, (rows, tll, jumps, root)):
            assert a[::-1].tobytes() == b.tobytes()
        for k in range(9):
            r1, t1, j1, o1 = both_calls(one, params[k], NINE[k:k + 1])
            assert r1[0].tobytes() == rows[k].tobytes() and t1[0].tobytes() == tll[k].tobytes(), k
            assert j1[0].tobytes() == jumps[k].tobytes() and o1[0].tobytes() == root[k].tobytes(), k
    finally:
        big.close()
        one.close()
    assert np.isfinite(rows).all() and len({r.tobytes() for r in rows}) == 9


def test_rows_do_not_depend_on_the_chunk_of_draws():
    """K = 64 and more trees than groups (the shape of the plain engine's test of
    the same name): the call's slots pass their budget and the draws run in
    chunks.  Forty draws, the nine rates in turn."""
    S, K, n = 7, 64, 40
    W = groups_cap(S, K)
    T = W + 44
    tips, ppeels, pblens, _ = gt.make_sample(S, K, 7, 3000 + K)
    logw = np.random.default_rng(7).normal(0.0, 1.0, T) - np.log(T)
    peels, blens, _, _ = pooled(ppeels, pblens, logw, T)
    _, params = go.random_draws(n, 2 * S - 3, K, np.random.default_rng(64))
    mus = NINE[np.arange(n) % 9]
    big = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=n)
    one = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=1)
    try:
        rows, tll, jumps, root = both_calls(big, params, mus)
        back = both_calls(big, params[::-1], mus[::-1])
        for a, b in zip(back, (rows, tll, jumps, root)):
            assert a[::-1].tobytes() == b.tobytes()
        for k in (0, 1, 2, 3, n - 5, n - 4, n - 3, n - 2, n - 1):  # nine draws, the nine rates, both ends of the call
            r1, t1, j1, o1 = both_calls(one, params[k], mus[k:k + 1])
            assert r1[0].tobytes() == rows[k].tobytes() and t1[0].tobytes() == tll[k].tobytes(), k
            assert j1[0].tobytes() == jumps[k].tobytes() and o1[0].tobytes() == root[k].tobytes(), k
    finally:
        big.close()
        one.close()
    assert np.isfinite(rows).all()


# ---------------------------------------------------------------- 7. a bad rate
@pytest.mark.parametrize("bad", [0.0, -1.0, np.nan, np.inf])
def test_a_bad_rate_does_not_touch_its_neighbours(bad):
    tips, peels, blens, logw, params = sample(7, 5, 7)
    mus = np.array([0.4, 2.0, bad, 0.9, 11.0])
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=5)
    try:
        rows, tll, jumps, root = both_calls(eng, params[:5], mus)  # status 0: no exception
        for k in (0, 1, 3, 4):
            r1, t1, j1, o1 = both_calls(eng, params[k], mus[k:k + 1])
            assert r1[0].tobytes() == rows[k].tobytes() and t1[0].tobytes() == tll[k].tobytes(), k
            assert j1[0].tobytes() == jumps[k].tobytes() and o1[0].tobytes() == root[k].tobytes(), k
            assert np.isfinite(rows[k]).all()
    finally:
        eng.close()
    assert rows[2, 0] == -np.inf and np.all(rows[2, 1:] == 0.0) and np.all(tll[2] == -np.inf)
    assert not jumps[2].any() and not root[2].any()


# ---------------------------------------------------------------- 8. refusals
def test_refusals():
    tips, peels, blens, logw, params = sample(7, 5, 7)
    lib = _lib.load()
    PHY_EINVAL, PHY_ERANGE = 1, 4
    K = 5
    eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=2)
    try:
        p = np.ascontiguousarray(params[:3])
        mu = np.ones(3)
        out = np.empty((3, 2 + geo.rate_count(K) + K))
        flat = np.empty((3, K * K + K))
        assert lib.phy_geo_trees_eval_clock(eng.ctx, 1, p.ctypes.data, None, out.ctypes.data, None) == PHY_EINVAL
        assert b"clock" in lib.phy_last_error()
        assert lib.phy_geo_trees_eval_clock_summaries(eng.ctx, 1, p.ctypes.data, None, out.ctypes.data, None,
                                                      flat.ctypes.data) == PHY_EINVAL
        assert b"clock" in lib.phy_last_error()
        assert lib.phy_geo_trees_eval_clock(None, 1, p.ctypes.data, mu.ctypes.data, out.ctypes.data, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval_clock(eng.ctx, 1, None, mu.ctypes.data, out.ctypes.data, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval_clock(eng.ctx, 1, p.ctypes.data, mu.ctypes.data, None, None) == PHY_EINVAL
        assert lib.phy_geo_trees_eval_clock_summaries(eng.ctx, 1, p.ctypes.data, mu.ctypes.data, None, None,
                                                      None) == PHY_EINVAL
        for n in (0, 3):  # max_draws + 1
            assert lib.phy_geo_trees_eval_clock(eng.ctx, n, p.ctypes.data, mu.ctypes.data, out.ctypes.data,
                                                None) == PHY_ERANGE
            assert b"n_draws out of range" in lib.phy_last_error()
            assert lib.phy_geo_trees_eval_clock_summaries(eng.ctx, n, p.ctypes.data, mu.ctypes.data, out.ctypes.data,
                                                          None, flat.ctypes.data) == PHY_ERANGE
        with pytest.raises(_lib.PhyloHipError, match="n_draws out of range"):
            eng.evaluate_rows_clock(p, mu)
        # out and tree_ll are optional in the summaries form, as in the plain one
        assert lib.phy_geo_trees_eval_clock_summaries(eng.ctx, 1, p.ctypes.data, mu.ctypes.data, None, None,
                                                      flat.ctypes.data) == 0
        assert lib.phy_geo_trees_eval_clock(eng.ctx, 1, p.ctypes.data, mu.ctypes.data, out.ctypes.data, None) == 0
        assert out[0].tobytes() == eng.evaluate_rows_clock(p[0], 1.0)[0].tobytes()
    finally:
        eng.close()
    assert lib.phy_geo_trees_clock_output_len(None) == -1


# ---------------------------------------------------------------- 9. the command line on the engine
def test_cli_run_geo_trees_clock_on_the_engine(tmp_path):
    """run --geo --trees --geo_clock --ancestral -a vb: 12 tips, K = 3, five trees, on the device engine."""
    from tests.test_geo_trees_cpu import write_dataset
    tree, meta, trees = write_dataset(tmp_path, 12, 3, 5, 90)
    base = ["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree, "--trees", trees, "-S", "11",
            "--eta", "0.1", "--iter", "60", "--elbo_samples", "8", "--samples", "16", "--tol_rel_obj", "0.01"]
    out = str(tmp_path / "est")
    post, lines = go.run_geo(base + ["-o", out, "--geo_clock"], host=False)
    assert isinstance(post.trees, geo.GeoTreesLikelihood) and post.trees.T == 5 and post.clock_estimated
    header, data = stan_io.read_samples(out)
    assert header[-2:] == ["freqs_geo.3", "rate_geo"]
    assert np.all(np.isfinite(data[:, -1])) and np.all(data[:, -1] > 0.0)
    assert os.path.exists(out + ".rates.tsv") and os.path.exists(out + ".jumps.tsv")
    from phylostan_amd import treeio
    taxa = [t.label for t in treeio.read_tree(tree).taxon_namespace]
    _, tblens = geo.tree_sample(treeio.read_trees(trees), taxa)
    probs = np.array([float(ln.split("\t")[1]) for ln in open(out + ".treeprob.tsv").read().splitlines()[1:]])
    times = sum(float(ln.split("\t")[-1]) for ln in open(out + ".jumps.tsv").read().splitlines()[1:])
    want = probs @ tblens.sum(1)
    print("dwell times sum %.12g, posterior-weighted tree length %.12g" % (times, want))
    assert abs(times - want) <= 1e-8 * want
    assert len([s for s in lines if s.startswith("rate_geo: posterior mean")]) == 1
    out = str(tmp_path / "fix")  # another model: another description
    post, lines = go.run_geo(["-s", str(tmp_path / "f.stan")] + base[2:] + ["-o", out, "--geo_rate", "0.5"], host=False)
    assert post.clock_fixed == 0.5 and os.path.exists(out + ".rates.tsv")
    header, _ = stan_io.read_samples(out)
    assert "rate_geo" not in header and header[-1] == "freqs_geo.3"
