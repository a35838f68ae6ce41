"""GPU: the phylogeography engines (``phy_geo_*``, ``phy_geo_trees_*``) on short
and zero-length branches: the cases of tests/geo_short_cases.py through
``GeoLikelihood.evaluate_rows``, ``evaluate_summaries``, ``evaluate_rows_clock``,
``evaluate_summaries_clock`` and ``GeoTreesLikelihood.evaluate_rows``,
``evaluate_summaries`` and ``evaluate_rows_clock``.  The host restatements on
the same cases: tests/test_geo_short_cpu.py, whose cached truths these tests
share.

Rows are checked as ``test_geo_gpu.check_row`` and ``test_geo_trees_gpu.check_rows``
check them: a seeded subset of each gradient array against the truth, every
entry against the host restatement, at the project's bars (log L relative
1e-10, each gradient array within 1e-9 of its largest entry, marginals absolute
1e-10, count arrays within 1e-9 of their largest entry, d/dmu at
``geo_clock_truth.dmu_bar``).

``test_dwell_times`` and the dwell-sum identity of ``check_invariants`` (in
``test_summaries_against_the_truths``): taken from the diagonal of ``G = V W
V^T`` the device's dwell times missed at mean length 1e-8 even with the expm1
forms, by 2.2e-8 (S = 4, K = 3) and 5.8e-8 (S = 7, K = 5) of the largest, and
their sum by 2.1e-8 and 7.0e-8 of the tree's length: G's off-diagonal entries
are of order 1 there while its diagonal is of order t, and the product keeps
1e-16 of the former.  Both device engines now form them from their two orders
in t, as the host does (``geo.psi_rule``; DESIGN.md, "Short branches of the geo
engines").
"""
import numpy as np
import pytest

from phylostan_amd import geo
from tests import geo_clock_truth as gc
from tests import geo_oracle as go
from tests import geo_short_cases as sc
from tests.test_geo_gpu import GRAD_BAR, K2_RATE_BAR, LL_BAR, split
from tests.test_geo_short_cpu import (CLOCK, SINGLE, SUMMARY, TREES, check_dwell, check_single, check_summaries,
                                      single_truth)
from tests.test_geo_summaries_cpu import JUMP_BAR, MARG_BAR
from tests.test_geo_trees_gpu import check_rows
from tests.test_geo_trees_gpu import check_summaries as check_trees_summaries

pytestmark = pytest.mark.gpu


def device_row(c, summaries=False):
    eng = geo.GeoLikelihood(c.tips, c.peel, max_draws=1)
    try:
        if summaries:
            return tuple(x[0] for x in eng.evaluate_summaries(c.blens, c.params))
        return eng.evaluate_rows(c.blens, c.params)[0]
    finally:
        eng.close()


def check_against_host(row, c):
    """Every entry of a single-tree row against the host restatement."""
    S, K = c.tips.shape
    rates, freqs = sc.split_params(c.params, K)
    ll, gb, gr, gf = split(row, 2 * S - 3, K)
    hl, hb, hr, hf = geo.geo_gradients_host(c.tips, c.peel, c.blens, rates, freqs)
    assert abs(ll - hl) <= LL_BAR * abs(hl)
    for name, got, host in (("blens", gb, hb), ("rates", gr, hr), ("freqs", gf, hf)):
        err, scale = np.abs(got - host).max(), np.abs(host).max()
        print("  d/d%s vs host %.2e of %.3e" % (name, err, scale))
        assert err <= GRAD_BAR * scale, name


@pytest.mark.parametrize("name", list(SINGLE))
def test_rows_against_the_truth(name):
    c = SINGLE[name]
    S, K = c.tips.shape
    row = device_row(c)
    check_single(name, *split(row, 2 * S - 3, K))
    check_against_host(row, c)


def test_a_zero_length_branch_passes_its_tip_through():
    """At length 0 the discordant tip's parent cannot be in another state: the
    device's log L is the truth's, 11 to 13 below that at length 1e-12."""
    for K in sc.DISCORDANT_KS:
        rows = [device_row(SINGLE["discordant-K%d-m1e-08-%s" % (K, z)]) for z in ("z0", "z12")]
        assert np.isfinite(rows[0][0]) and rows[1][0] - rows[0][0] > 5.0


@pytest.mark.parametrize("name", list(SUMMARY))
def test_summaries_against_the_truths(name):
    c = SUMMARY[name]
    S, K = c.tips.shape
    rates, freqs = sc.split_params(c.params, K)
    row, marg, jumps, bjumps = device_row(c, summaries=True)
    assert row.tobytes() == device_row(c).tobytes()
    hm, hj, hb = geo.geo_summaries_host(c.tips, c.peel, c.blens, rates, freqs)
    assert np.abs(marg - hm).max() <= MARG_BAR
    assert np.abs(jumps - hj).max() <= JUMP_BAR * np.abs(hj).max()
    assert np.abs(bjumps - hb).max() <= JUMP_BAR * np.abs(hb).max()
    check_summaries(name, marg, jumps, bjumps, grad_blens=row[1:1 + 2 * S - 3])


@pytest.mark.parametrize("name", list(SUMMARY))
def test_dwell_times(name):
    check_dwell(name, device_row(SUMMARY[name], summaries=True)[2])


@pytest.mark.parametrize("name", [n for n in CLOCK if n != "trees"])
def test_single_tree_with_a_small_clock_rate(name):
    c = CLOCK[name]
    S, K = c.tips.shape
    B, R = 2 * S - 3, geo.rate_count(K)
    rates, freqs = sc.split_params(c.params, K)
    eng = geo.GeoLikelihood(c.tips, c.peel, max_draws=1)
    try:
        row = eng.evaluate_rows_clock(c.blens, c.params, c.mu)[0]
        srow, marg, jumps, bjumps = (x[0] for x in eng.evaluate_summaries_clock(c.blens, c.params, c.mu))
    finally:
        eng.close()
    assert srow.tobytes() == row.tobytes()
    ll, gb, gr, gf, gm = row[0], row[1:1 + B], row[1 + B:1 + B + R], row[1 + B + R:-1], row[-1]
    tl, tg = go.truth_gradients(c.tips, c.peel, c.mu * c.blens, rates, freqs)
    assert abs(ll - tl) <= gc.LL_BAR * abs(tl)
    want_gb = c.mu * tg["blens"][1]
    assert np.abs(gb - want_gb).max() <= gc.GRAD_BAR * np.abs(want_gb).max()
    assert np.abs(gr - tg["rates"][1]).max() <= gc.GRAD_BAR * np.abs(gr).max()
    assert np.abs(gf - tg["freqs"][1]).max() <= gc.GRAD_BAR * np.abs(gf).max()
    want = go.truth(c.tips, c.peel, c.blens * complex(c.mu, gc.STEP), rates, freqs).imag / gc.STEP
    bar = gc.dmu_bar(want, min(1.0, c.mu) * np.abs(c.blens * tg["blens"][1]).sum())
    print("%s: d/dmu %.12g truth %.12g err %.2e bar %.2e" % (name, gm, want, abs(gm - want), bar))
    assert abs(gm - want) <= bar
    # the summaries: those of the host at mu * blens, the dwell times back in the tree's unit
    hm, hj, hb = geo.geo_summaries_host(c.tips, c.peel, c.blens, rates, freqs, clock=c.mu)
    off = ~np.eye(K, dtype=bool)
    assert np.abs(marg - hm).max() <= MARG_BAR
    assert np.abs(jumps[off] - hj[off]).max() <= JUMP_BAR * np.abs(hj[off]).max()
    assert np.abs(bjumps - hb).max() <= JUMP_BAR * np.abs(hb).max()


def test_tree_sample_with_a_small_clock_rate():
    c, mu = CLOCK["trees"]
    eng = geo.GeoTreesLikelihood(c.tips, c.peels, c.blens, c.logw, max_draws=1)
    try:
        row = eng.evaluate_rows_clock(c.params, mu)[0]
        tll = eng.tree_loglik[0]
    finally:
        eng.close()
    gc.check_clock_row(row, tll, c.tips, c.peels, c.blens, c.params, c.logw, mu, entries=c.entries)
    host, htll = gc.host_clock_row(c.tips, c.peels, c.blens, c.params, c.logw, mu)
    R, K = geo.rate_count(c.tips.shape[1]), c.tips.shape[1]
    for got, want in ((row[1:1 + R], host[1:1 + R]), (row[1 + R:1 + R + K], host[1 + R:1 + R + K])):
        assert np.abs(got - want).max() <= GRAD_BAR * np.abs(want).max()


@pytest.mark.parametrize("name", list(TREES))
def test_tree_samples_against_the_truth(name):
    c = TREES[name]
    eng = geo.GeoTreesLikelihood(c.tips, c.peels, c.blens, c.logw, max_draws=1)
    try:
        rows = eng.evaluate_rows(c.params)
        tll = eng.tree_loglik[0].copy()
        srows, jumps, root = eng.evaluate_summaries(c.params)
    finally:
        eng.close()
    assert srows.tobytes() == rows.tobytes()
    tlls = check_rows((rows[0], tll), c.tips, c.peels, c.blens, c.params, c.logw, c.entries)
    check_trees_summaries(jumps[0], root[0], c.tips, c.peels, c.blens, c.params, c.logw, tlls, None)


def test_short_draws_in_a_batch_are_the_draws_alone():
    """The five tiny cases' branch lengths and the K = 5 tiny case's parameters
    (each draw its own), mixed with ordinary draws in one call: every row is
    bitwise the draw evaluated alone, and the short rows meet the truth."""
    base = SINGLE["tiny-K5"]
    S, K = base.tips.shape
    B, R = 2 * S - 3, geo.rate_count(K)
    rng = np.random.default_rng(55)
    short_blens = np.stack([SINGLE["tiny-K%d" % k].blens for k in sc.TINY_KS])  # every tiny case has S = 7
    _, short_params = go.random_draws(len(sc.TINY_KS), B, K, rng)
    short_params[0] = base.params
    ord_blens, ord_params = go.random_draws(6, B, K, rng)
    order = rng.permutation(11)
    blens = np.concatenate([short_blens, ord_blens])[order]
    params = np.concatenate([short_params, ord_params])[order]
    eng = geo.GeoLikelihood(base.tips, base.peel, max_draws=11)
    one = geo.GeoLikelihood(base.tips, base.peel, max_draws=1)
    try:
        rows = eng.evaluate_rows(blens, params)
        for n in range(11):
            assert one.evaluate_rows(blens[n], params[n])[0].tobytes() == rows[n].tobytes(), n
    finally:
        eng.close()
        one.close()
    for n in range(11):
        tl, tg = go.truth_gradients(base.tips, base.peel, blens[n], params[n, :R], params[n, R:], max_entries=2, seed=n)
        ll, gb, gr, gf = split(rows[n], B, K)
        assert abs(ll - tl) <= LL_BAR * abs(tl), n
        for name, got in (("blens", gb), ("rates", gr), ("freqs", gf)):
            idx, want = tg[name]
            assert np.abs(got[idx] - want).max() <= GRAD_BAR * np.abs(got).max(), (n, name)


def test_one_short_tree_is_phy_geo_eval():
    """``phy_geo_trees_eval`` at T = 1 returns ``phy_geo_eval``'s bits
    (``test_geo_trees_gpu.test_one_tree_is_phy_geo_eval``) on a short tree."""
    c = SINGLE["discordant-K5-m1e-08-z0"]
    S, K = c.tips.shape
    B, R = 2 * S - 3, geo.rate_count(K)
    one = geo.GeoLikelihood(c.tips, c.peel, max_draws=1)
    eng = geo.GeoTreesLikelihood(c.tips, c.peel[None], c.blens[None], max_draws=1)
    try:
        old, marg, ojumps, _ = one.evaluate_summaries(c.blens, c.params)
        rows, jumps, root = eng.evaluate_summaries(c.params)
        tll = eng.tree_loglik
    finally:
        one.close()
        eng.close()
    assert np.isfinite(old[0, 0]) and rows[0, 0] == old[0, 0] and tll[0, 0] == old[0, 0]
    assert np.array_equal(rows[0, 1:1 + R], old[0, 1 + B:1 + B + R])
    assert np.array_equal(rows[0, 1 + R:], old[0, 1 + B + R:])
    assert np.array_equal(jumps[0], ojumps[0]) and np.array_equal(root[0], marg[0, 2 * S - 2])
    assert abs(old[0, 0] - single_truth("discordant-K5-m1e-08-z0")[0]) <= LL_BAR * abs(old[0, 0])
    assert K2_RATE_BAR < np.abs(old[0, 1 + B:1 + B + R]).max()  # a gradient, not the zero row of a refusal
