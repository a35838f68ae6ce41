"""GPU: the discrete-trait (phylogeography) engine, ``phy_geo_*``, against the
complex-step truth of tests/geo_oracle.py.

Bars (the project's): log L at relative 1e-10, each gradient array within 1e-9
of its largest entry.  The truth costs one complex evaluation per entry, so
where an array is long a seeded subset of its entries is compared with the
truth and the whole array with ``geo_gradients_host`` -- which the CPU suite
(tests/test_geo_cpu.py) pins to the truth entry by entry -- at the same bar.
At K = 2 the normalisation cancels the single rate: its gradient is exactly
zero and is compared absolutely, <= 1e-12.
"""
import functools
import os

import numpy as np
import pytest

from phylostan_amd import _lib, geo
from tests import geo_oracle as go

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_BAR, GRAD_BAR, K2_RATE_BAR = 1e-10, 1e-9, 1e-12


def split(row, B, K):
    R = geo.rate_count(K)
    return row[0], row[1:1 + B], row[1 + B:1 + B + R], row[1 + B + R:]


def check_row(row, tips, peel, blens, params, entries, extended=False, seed=0):
    """One output row against the truth (a seeded subset of each gradient
    array) and the host restatement (every entry)."""
    S, K = tips.shape
    B, R = 2 * S - 3, geo.rate_count(K)
    rates, freqs = params[:R], params[R:]
    ll, gb, gr, gf = split(row, B, K)
    tl, tg = go.truth_gradients(tips, peel, blens, rates, freqs, extended=extended, max_entries=entries, seed=seed)
    _, hb, hr, hf = geo.geo_gradients_host(tips, peel, blens, rates, freqs)
    print("S %d K %d: log L %.12g truth %.12g rel %.2e" % (S, K, ll, tl, abs(ll - tl) / abs(tl)))
    assert abs(ll - tl) <= LL_BAR * abs(tl)
    for name, got, host in (("blens", gb, hb), ("rates", gr, hr), ("freqs", gf, hf)):
        idx, want = tg[name]
        scale = np.abs(host).max()
        e_truth, e_host = np.abs(got[idx] - want).max(), np.abs(got - host).max()
        print("  d/d%s: |max| %.3e, vs truth %.2e, vs host %.2e" % (name, scale, e_truth, e_host))
        if name == "rates" and K == 2:
            assert e_truth <= K2_RATE_BAR and np.abs(got).max() <= K2_RATE_BAR
            continue
        assert e_truth <= GRAD_BAR * scale, name
        assert e_host <= GRAD_BAR * scale, name


def make_case(S, K, seed, peel=None):
    """One all-ones tip (0) and one zero-length branch (1) in every case."""
    rng = np.random.default_rng(seed)
    peel = go.random_peel(S, rng) if peel is None else peel
    tips = go.random_tips(S, K, rng, missing=(0,))
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens[0, 1] = 0.0
    return tips, peel, blens[0], params[0]


@functools.lru_cache(maxsize=None)
def flu_peel():
    from phylostan_amd import data as dataio
    tree = dataio.read_tree(os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.tree"))
    tree.resolve_polytomies(update_bipartitions=True)
    dataio.setup_indexes(tree)
    peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
    return peel0, geo.tree_branch_lengths(tree, peel0)


@pytest.mark.parametrize("K", [2, 3, 4, 5, 17, 33, 64])
@pytest.mark.parametrize("S", [3, 7])
def test_small_trees_every_k(S, K):
    tips, peel, blens, params = make_case(S, K, 100 * S + K)
    eng = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        row = eng.evaluate_rows(blens, params)[0]
        assert eng.sweeps(1)[0] >= 1
    finally:
        eng.close()
    check_row(row, tips, peel, blens, params, entries=4)


@pytest.mark.parametrize("K,entries", [(5, 6), (33, 3), (64, 1)])
def test_fluA_tree_synthetic_locations(K, entries):
    peel, tree_blens = flu_peel()
    S = peel.shape[0] + 1
    assert S == 69
    tips, _, _, params = make_case(S, K, 69000 + K, peel=peel)
    blens = tree_blens * (0.3 / tree_blens.mean())  # the tree's shape at the locations' time scale
    blens[1] = 0.0
    eng = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        row = eng.evaluate_rows(blens, params)[0]
    finally:
        eng.close()
    check_row(row, tips, peel, blens, params, entries=entries)


def test_caterpillar_200_tips():
    S, K = 200, 4
    peel = go.caterpillar_peel(S)
    tips, _, blens, params = make_case(S, K, 200, peel=peel)
    blens *= 0.2
    eng = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        assert eng.info()["levels"] == S - 1 and eng.info()["widest_level"] == 1
        row = eng.evaluate_rows(blens, params)[0]
    finally:
        eng.close()
    check_row(row, tips, peel, blens, params, entries=4)


@pytest.mark.parametrize("K", [4, 17])
@pytest.mark.parametrize("arm", ["tie", "near"])
def test_repeated_eigenvalues(K, arm):
    """Equal rates and frequencies: a (K-1)-fold eigenvalue (Phi's tie arm);
    one rate moved by 1e-11: its near arm."""
    tips, peel, blens, _ = make_case(9, K, 900 + K)
    rates = np.ones(geo.rate_count(K))
    if arm == "near":
        rates[1] += 1e-11
    params = np.concatenate([rates, np.full(K, 1.0 / K)])
    eng = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        row = eng.evaluate_rows(blens, params)[0]
    finally:
        eng.close()
    check_row(row, tips, peel, blens, params, entries=5)


BATCH_S, BATCH_K, BATCH_N = 7, 5, 300


@functools.lru_cache(maxsize=None)
def batch_case():
    tips, peel, _, _ = make_case(BATCH_S, BATCH_K, 77)
    blens, params = go.random_draws(BATCH_N, 2 * BATCH_S - 3, BATCH_K, np.random.default_rng(78))
    R = geo.rate_count(BATCH_K)
    truth = [go.truth_gradients(tips, peel, blens[n], params[n, :R], params[n, R:], max_entries=2, seed=n)
             for n in range(BATCH_N)]
    host = [geo.geo_gradients_host(tips, peel, blens[n], params[n, :R], params[n, R:]) for n in range(BATCH_N)]
    return tips, peel, blens, params, truth, host


@pytest.mark.parametrize("n", [1, 4, 33, 300])
def test_batches(n):
    """Every row of a batch against the oracle; draw k of a batch bitwise the
    draw alone; a repeated call bitwise the first.  The context holds fewer
    workgroups' worth of draws than the largest batch only if the device has
    fewer than 150 CUs; the loop over draws is the same code either way."""
    tips, peel, blens, params, truth, host = batch_case()
    B, K = 2 * BATCH_S - 3, BATCH_K
    eng = geo.GeoLikelihood(tips, peel, max_draws=n)
    one = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        rows = eng.evaluate_rows(blens[:n], params[:n])
        again = eng.evaluate_rows(blens[:n], params[:n])
        assert rows.tobytes() == again.tobytes()
        for k in sorted({0, n // 2, n - 1}):
            alone = one.evaluate_rows(blens[k], params[k])[0]
            assert alone.tobytes() == rows[k].tobytes(), k
    finally:
        eng.close()
        one.close()
    worst = 0.0
    for k in range(n):
        ll, gb, gr, gf = split(rows[k], B, K)
        tl, tg = truth[k]
        assert abs(ll - tl) <= LL_BAR * abs(tl), k
        for name, got, hst in (("blens", gb, host[k][1]), ("rates", gr, host[k][2]), ("freqs", gf, host[k][3])):
            idx, want = tg[name]
            scale = np.abs(hst).max()
            err = max(np.abs(got[idx] - want).max(), np.abs(got - hst).max()) / scale
            worst = max(worst, err)
            assert err <= GRAD_BAR, (k, name)
    print("batch %d: worst gradient error %.2e of the array's largest entry" % (n, worst))


def test_more_draws_than_workgroups():
    """The workspace budget (512 MiB) caps the grid: at 700 tips and K = 64 it
    leaves about 100 workgroups, so a 150-draw call loops; each row is bitwise
    the draw alone."""
    S, K, n = 700, 64, 150
    rng = np.random.default_rng(5)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng)
    blens, params = go.random_draws(n, 2 * S - 3, K, rng, mean_blen=0.05)
    eng = geo.GeoLikelihood(tips, peel, max_draws=n)
    one = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        assert eng.info()["workgroups"] < n
        rows = eng.evaluate_rows(blens, params)
        assert np.all(np.isfinite(rows))
        for k in (0, n - 1):
            assert one.evaluate_rows(blens[k], params[k])[0].tobytes() == rows[k].tobytes()
    finally:
        eng.close()
        one.close()


def test_rescaling_past_the_fp64_range():
    S, K = 600, 8
    rng = np.random.default_rng(600)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng)
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens, params = blens[0], params[0]
    R = geo.rate_count(K)
    with np.errstate(divide="ignore"):
        plain = go.truth(tips, peel, blens, params[:R], params[R:]).real
    assert plain == -np.inf, "the plain truth must underflow on this input: enlarge S"
    eng = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        row = eng.evaluate_rows(blens, params)[0]
    finally:
        eng.close()
    assert np.isfinite(row[0]) and row[0] < np.log(np.finfo(np.float64).tiny)
    check_row(row, tips, peel, blens, params, entries=4, extended=True)


def test_refusals():
    tips, peel, blens, params = make_case(7, 4, 1)
    lib = _lib.load()
    with pytest.raises(_lib.PhyloHipError, match="supported 2..64"):
        geo.GeoLikelihood(np.ones((7, 65)), peel)
    with pytest.raises(_lib.PhyloHipError, match="supported 2..64"):
        geo.GeoLikelihood(np.ones((7, 1)), peel)
    bad = peel.copy()
    bad[-1, 1], bad[-1, 0] = bad[-1, 0], bad[-1, 1]
    with pytest.raises(_lib.PhyloHipError, match="last peel row"):
        geo.GeoLikelihood(tips, bad)
    bad = peel.copy()
    bad[1, 0] = bad[0, 0]
    with pytest.raises(_lib.PhyloHipError, match="already has a parent|before it is computed"):
        geo.GeoLikelihood(tips, bad)
    with pytest.raises(_lib.PhyloHipError, match=r"\[0, 1\]"):
        geo.GeoLikelihood(tips * 2.0, peel)
    eng = geo.GeoLikelihood(tips, peel, max_draws=2)
    try:
        with pytest.raises(_lib.PhyloHipError, match="n_draws out of range"):
            eng.evaluate_rows(np.tile(blens, (3, 1)), np.tile(params, (3, 1)))
        p2 = np.tile(params, (2, 1))
        p2[1, geo.rate_count(4) + 2] = 0.0  # a non-positive frequency: -inf, status 0, the other draw untouched
        rows = eng.evaluate_rows(np.tile(blens, (2, 1)), p2)
        assert rows[1, 0] == -np.inf and np.all(rows[1, 1:] == 0.0)
        assert np.isfinite(rows[0]).all()
        assert rows[0].tobytes() == eng.evaluate_rows(blens, params)[0].tobytes()
    finally:
        eng.close()
    assert lib.phy_geo_output_len(None) == -1


def test_cli_run_geo_nuts_on_the_engine(tmp_path):
    """run --geo -a nuts, 2 chains x (100 + 100), S = 30, K = 3, on the device
    engine: finite lp__, simplex rows, rates >= 0.1.  No posterior statistic.

    About 20 s on an MI355X, of which the engine's calls are 0.16 ms each: the
    emitted model puts no prior on rates_geo and its normalised Q hides their
    common scale, so the posterior is improper along it and NUTS builds its
    deepest trees (some 130,000 gradient rounds for these 400 iterations)."""
    from phylostan_amd import cli, stan_io
    tree, meta = go.write_geo_dataset(str(tmp_path), S=30, K=3, seed=30)
    out = str(tmp_path / "geo")
    go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "-t", tree, "-o", out, "-a", "nuts", "--chains", "2",
             "--iter", "200", "-S", "11"], host=False)
    for c in range(2):
        header, data = stan_io.read_samples(out + "_%d.csv" % c)
        assert header[0] == "lp__" and header[7:10] == ["rates_geo.1", "rates_geo.2", "rates_geo.3"]
        assert header[10:] == ["freqs_geo.1", "freqs_geo.2", "freqs_geo.3"]
        assert data.shape == (100, 13) and np.all(np.isfinite(data[:, 0]))
        assert np.all(data[:, 7:10] >= 0.1)
        assert np.all(data[:, 10:] > 0.0) and np.allclose(data[:, 10:].sum(1), 1.0, atol=1e-5)
        assert not os.path.exists(out + "_%d.trees" % c)
    assert cli.load_artifact(str(tmp_path / "m.stan"))["options"]["geo"] is True
