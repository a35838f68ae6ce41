"""CPU: the phylogeography host restatements on short and zero-length branches
(tests/geo_short_cases.py): ``geo.geo_gradients_host`` with and without a
clock, ``geo_summaries_host``, ``geo_trees_host`` and
``geo_trees_summaries_host`` against the truths that share no algebra with them
(expm(Q t) by a Taylor series, complex-step derivatives, enumeration).  The
device on the same cases: tests/test_geo_short_gpu.py.

Bars: the project's, as the files that own them state them -- log L at relative
1e-10, each gradient array within 1e-9 of its largest entry, marginals absolute
1e-10, each count array within 1e-9 of its largest entry, d/dmu at
``geo_clock_truth.dmu_bar``.  The dwell times (the diagonal of ``jumps``) are of
the order of the tree's length and would go unchecked beside off-diagonal counts
of order 1, so they are compared as an array of their own, within 1e-9 of the
largest dwell time.

Before the expm1 forms of ``geo._geo_passes`` the host missed these bars by up
to nine orders ("Short branches" of the geo engines, has the table):
log L 3e-9 to 6e-8 on the tiny cases, off by 16 to 19 percent or not finite on
the discordant ones at mean length 1e-8.

``test_dwell_times``: taken from the diagonal of ``G = V W V^T`` the dwell times
missed at mean length 1e-8 even with the expm1 forms, by 9.7e-8 (S = 4, K = 3)
and 8.0e-8 (S = 7, K = 5) of the largest: G's off-diagonal entries are of order
1 there while its diagonal is of order t, and the product rounds at 1e-16 of the
former.  ``geo_summaries_host`` forms them from their two orders in t
(``geo.psi_rule``) and is at 8e-16 and 4e-16.
"""
import functools

import numpy as np
import pytest

from phylostan_amd import geo
from tests import geo_clock_truth as gc
from tests import geo_oracle as go
from tests import geo_short_cases as sc
from tests import geo_summary_truth as gst
from tests import geo_trees_truth as gt
from tests.test_geo_summaries_cpu import JUMP_BAR, MARG_BAR, check_invariants
from tests.test_geo_trees_cpu import GRAD_BAR, LL_BAR, check_host

SINGLE = sc.single_cases()
SUMMARY = sc.summary_cases()
TREES = sc.tree_cases()
CLOCK = sc.clock_cases()


@functools.lru_cache(maxsize=None)
def single_truth(name):
    """(log L, {array: (indices, derivatives)}) of a single-tree case: computed once, never changed."""
    c = SINGLE[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    tl, tg = go.truth_gradients(c.tips, c.peel, c.blens, rates, freqs, max_entries=c.entries)
    assert np.isfinite(tl) and all(np.all(np.isfinite(g)) for _, g in tg.values())
    return tl, tg


@functools.lru_cache(maxsize=None)
def summary_truth(name):
    """(jumps [K, K], bjumps [B], marginals by enumeration or None)."""
    c = SUMMARY[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    tj = gst.jump_matrix(c.tips, c.peel, c.blens, rates, freqs)
    tb = gst.branch_jump_truth(c.tips, c.peel, c.blens, rates, freqs)
    tm = gst.brute_marginals(c.tips, c.peel, c.blens, rates, freqs) if c.enumerate else None
    assert np.all(np.isfinite(tj)) and np.all(np.isfinite(tb))
    return tj, tb, tm


def check_single(name, ll, gb, gr, gf):
    """A single-tree row against the truth, at the bars of test_geo_cpu.py."""
    tl, tg = single_truth(name)
    print("%s: log L %.12g truth %.12g rel %.2e" % (name, ll, tl, abs(ll - tl) / abs(tl)))
    assert abs(ll - tl) <= LL_BAR * abs(tl)
    for arr, got in (("blens", gb), ("rates", gr), ("freqs", gf)):
        idx, want = tg[arr]
        err, scale = np.abs(got[idx] - want).max(), np.abs(got).max()
        print("  d/d%s: |max| %.3e, vs truth %.2e" % (arr, scale, err))
        assert err <= GRAD_BAR * scale, arr


@pytest.mark.parametrize("name", list(SINGLE))
def test_host_gradients_against_the_truth(name):
    c = SINGLE[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    check_single(name, *geo.geo_gradients_host(c.tips, c.peel, c.blens, rates, freqs))


def test_a_zero_length_branch_passes_its_tip_through():
    """Length 0 is the identity, not V V^T: moving the discordant tip's branch
    from 0 to 1e-12 raises the likelihood by the change it now admits there,
    and the host follows the truth on both sides."""
    for K in sc.DISCORDANT_KS:
        z0, z12 = (single_truth("discordant-K%d-m1e-08-%s" % (K, z))[0] for z in ("z0", "z12"))
        assert z12 - z0 > 5.0  # q 1e-12 against (q 1e-8)^2


@pytest.mark.parametrize("name", [n for n in CLOCK if n != "trees"])
def test_host_single_tree_with_a_small_clock_rate(name):
    c = CLOCK[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    ll, gb, gr, gf, gm = geo.geo_gradients_host(c.tips, c.peel, c.blens, rates, freqs, clock=c.mu)
    tl, tg = go.truth_gradients(c.tips, c.peel, c.mu * c.blens, rates, freqs)
    assert abs(ll - tl) <= gc.LL_BAR * abs(tl)
    want_gb = c.mu * tg["blens"][1]  # with respect to the tree's own lengths
    assert np.abs(gb - want_gb).max() <= gc.GRAD_BAR * np.abs(want_gb).max()
    assert np.abs(gr - tg["rates"][1]).max() <= gc.GRAD_BAR * np.abs(gr).max()
    assert np.abs(gf - tg["freqs"][1]).max() <= gc.GRAD_BAR * np.abs(gf).max()
    want = go.truth(c.tips, c.peel, c.blens * complex(c.mu, gc.STEP), rates, freqs).imag / gc.STEP
    bar = gc.dmu_bar(want, min(1.0, c.mu) * np.abs(c.blens * tg["blens"][1]).sum())
    print("%s: d/dmu %.12g truth %.12g err %.2e bar %.2e" % (name, gm, want, abs(gm - want), bar))
    assert abs(gm - want) <= bar


def test_host_tree_sample_with_a_small_clock_rate():
    c, mu = CLOCK["trees"]
    row, tll = gc.host_clock_row(c.tips, c.peels, c.blens, c.params, c.logw, mu)
    gc.check_clock_row(row, tll, c.tips, c.peels, c.blens, c.params, c.logw, mu, entries=c.entries)


@pytest.mark.parametrize("name", list(TREES))
def test_host_mixture_against_the_truth(name):
    c = TREES[name]
    K = c.tips.shape[1]
    rates, freqs = sc.split_params(c.params, K)
    _, _, _, tll = check_host(c.tips, c.peels, c.blens, c.params, c.logw, entries=c.entries)
    assert gt.tree_weights(tll, c.logw).max() < 0.9  # more than one tree carries weight
    jumps, root = geo.geo_trees_summaries_host(c.tips, c.peels, c.blens, rates, freqs, c.logw)
    tj, tr, p = gt.summaries_truth(c.tips, c.peels, c.blens, rates, freqs, c.logw)
    assert np.abs(jumps - tj).max() <= GRAD_BAR * np.abs(tj).max()
    assert np.abs(root - tr).max() <= GRAD_BAR * tr.max()
    assert abs(root.sum() - 1.0) <= 1e-12


def check_summaries(name, marg, jumps, bjumps, grad_blens=None):
    """Marginals, jumps and bjumps of a summary case against the truths, and the invariants."""
    c = SUMMARY[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    tj, tb, tm = summary_truth(name)
    ej, eb = np.abs(jumps - tj).max() / np.abs(tj).max(), np.abs(bjumps - tb).max() / np.abs(tb).max()
    print("%s: jumps %.2e, bjumps %.2e of the largest entry" % (name, ej, eb))
    assert ej <= JUMP_BAR and eb <= JUMP_BAR
    if tm is not None:
        print("  marginals vs enumeration %.2e" % np.abs(marg - tm).max())
        assert np.abs(marg - tm).max() <= MARG_BAR
    check_invariants(c.tips, c.peel, c.blens, rates, freqs, marg, jumps, bjumps, grad_blens=grad_blens)


def check_dwell(name, jumps):
    tj = summary_truth(name)[0]
    err = np.abs(np.diag(jumps) - np.diag(tj)).max() / np.diag(tj).max()
    print("%s: dwell times %.2e of the largest, %.3e" % (name, err, np.diag(tj).max()))
    assert err <= JUMP_BAR


@pytest.mark.parametrize("name", list(SUMMARY))
def test_host_summaries_against_the_truths(name):
    c = SUMMARY[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    check_summaries(name, *geo.geo_summaries_host(c.tips, c.peel, c.blens, rates, freqs))


@pytest.mark.parametrize("name", list(SUMMARY))
def test_dwell_times(name):
    c = SUMMARY[name]
    rates, freqs = sc.split_params(c.params, c.tips.shape[1])
    check_dwell(name, geo.geo_summaries_host(c.tips, c.peel, c.blens, rates, freqs)[1])
