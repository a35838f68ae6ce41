"""The short-branch cases of the phylogeography engines, shared by
tests/test_geo_short_cpu.py (the host restatements) and
tests/test_geo_short_gpu.py (the device).  numpy only; built from the
generators of tests/geo_oracle.py and tests/geo_trees_truth.py.

A trait tree's branches are the time tree's: samples of one outbreak sit on
branches of 1e-8 and of exactly 0 beside ordinary ones.  There ``V (e^{lam t} o
V^T x)`` equals ``P(t) x`` to 1e-16 absolutely, which is 1e-16 / (q t) of a
transition probability q t ("Short branches" of the geo engines).
Every case has dense positive rates (``random_draws``: >= 0.1), so every entry
of P is of order q t and the truth is finite without ``extended=True``.

* ``single_cases()``   one tree, one draw: name -> ``Case`` (tips, peel, blens,
  params, entries); ``entries`` truth entries per gradient array.
  - tiny:        S = 7, mean length 1e-8, tip 0 all ones, ``blens[1] = 0``;
  - discordant:  every tip in state a but tip 1, in state a + 1 on branch 1 of
                 length 0 (``z0``) or 1e-12 (``z12``): the likelihood is that of
                 one change on a tree of total length ~ B m, and at length 0
                 the change cannot be on branch 1;
  - mixed:       S = 9, lengths cycling through 1e-8, 0.3, 1e-4, 5.0, one 0:
                 the expm1 and exp regimes and Phi's arms in one row;
  - tie / near:  a (K-1)-fold eigenvalue and one split by 1e-11, mean 1e-8;
  - ladder:      a 40-tip caterpillar, mean 1e-8: 39 levels of accumulation.
* ``clock_cases()``    ordinary trees at mu = 1e-8 and 1e-4: the same effective
  lengths by the other route.
* ``tree_cases()``     tree samples: all short, and one short among ordinary.
* ``summary_cases()``  S = 4, K = 3 (marginals by enumeration) and S = 7, K = 5.
"""
import collections
import functools

import numpy as np

from phylostan_amd import geo
from tests import geo_clock_truth as gc
from tests import geo_oracle as go
from tests import geo_trees_truth as gt

Case = collections.namedtuple("Case", "tips peel blens params entries")
TreesCase = collections.namedtuple("TreesCase", "tips peels blens params logw entries")
ClockCase = collections.namedtuple("ClockCase", "tips peel blens params mu")
SummaryCase = collections.namedtuple("SummaryCase", "tips peel blens params enumerate")

TINY_KS = (3, 5, 17, 33, 64)
DISCORDANT_KS = (3, 5, 17, 33)
SHORT = 1e-8


def _entries(K):
    """Truth entries per gradient array: one complex evaluation each."""
    return 2 if K >= 64 else 3 if K >= 17 else 4


def tiny(K, S=7, mean=SHORT):
    rng = np.random.default_rng(100 + K)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=(0,))
    blens, params = go.random_draws(1, 2 * S - 3, K, rng, mean_blen=mean)
    blens[0, 1] = 0.0
    return Case(tips, peel, blens[0], params[0], _entries(K))


def discordant(K, mean, zero=0.0, S=7):
    base = tiny(K, S, mean)
    a = int(np.random.default_rng(100 + K).integers(0, K))
    tips = np.zeros((S, K))
    tips[:, a] = 1.0
    tips[1] = 0.0
    tips[1, (a + 1) % K] = 1.0
    blens = base.blens.copy()
    blens[1] = zero
    return Case(tips, base.peel, blens, base.params, base.entries)


def mixed_scales(K, S=9):
    rng = np.random.default_rng(900 + K)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=(0,))
    _, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens = np.asarray([(1e-8, 0.3, 1e-4, 5.0)[b % 4] for b in range(2 * S - 3)])
    blens[5] = 0.0
    return Case(tips, peel, blens, params[0], _entries(K))


def repeated(K, arm, S=9):
    """``test_repeated_eigenvalues``' constructions on a short tree."""
    rng = np.random.default_rng(900 + K)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=(0,))
    blens, _ = go.random_draws(1, 2 * S - 3, K, rng, mean_blen=SHORT)
    blens[0, 1] = 0.0
    rates = np.ones(geo.rate_count(K))
    if arm == "near":
        rates[1] += 1e-11
    return Case(tips, peel, blens[0], np.concatenate([rates, np.full(K, 1.0 / K)]), _entries(K))


def ladder(S=40, K=5):
    rng = np.random.default_rng(4000 + K)
    peel = go.caterpillar_peel(S)
    tips = go.random_tips(S, K, rng, missing=(0,))
    blens, params = go.random_draws(1, 2 * S - 3, K, rng, mean_blen=SHORT)
    blens[0, 1] = 0.0
    return Case(tips, peel, blens[0], params[0], 4)


@functools.lru_cache(maxsize=None)
def single_cases():
    out = collections.OrderedDict()
    for K in TINY_KS:
        out["tiny-K%d" % K] = tiny(K)
    for K in DISCORDANT_KS:
        for mean in (1e-4, 1e-8):
            out["discordant-K%d-m%g-z0" % (K, mean)] = discordant(K, mean)
            out["discordant-K%d-m%g-z12" % (K, mean)] = discordant(K, mean, zero=1e-12)
    for K in (5, 33):
        out["mixed-K%d" % K] = mixed_scales(K)
    for K in (4, 17):
        for arm in ("tie", "near"):
            out["%s-K%d" % (arm, K)] = repeated(K, arm)
    out["ladder-S40-K5"] = ladder()
    return out


@functools.lru_cache(maxsize=None)
def clock_cases():
    """Single trees with a trait clock: name -> ``ClockCase``; and the tree
    sample ``"mixed"`` of ``geo_clock_truth.truth_cases()`` at mu = 1e-7:
    ``(TreesCase, mu)`` under ``"trees"``."""
    out = collections.OrderedDict()
    base = tiny(5, mean=0.3)
    for mu in (1e-8, 1e-4):
        out["clock-mu%g" % mu] = ClockCase(base.tips, base.peel, base.blens, base.params, mu)
    tips, peels, blens, params, logw, _, _, entries = gc.truth_cases()["mixed"]
    out["trees"] = (TreesCase(tips, peels, blens, params, logw, entries), 1e-7)
    return out


@functools.lru_cache(maxsize=None)
def tree_cases():
    out = collections.OrderedDict()
    tips, peels, blens, params = gt.make_sample(7, 5, 7, 7100, mean_blen=SHORT)
    logw = np.log(np.random.default_rng(71).dirichlet(np.ones(7) * 2.0))
    out["all-short"] = TreesCase(tips, peels, blens, params, logw, None)
    tips, peels, blens, params = gt.make_sample(7, 5, 3, 7200)
    blens = blens.copy()
    blens[1] *= SHORT / 0.3  # the caterpillar and the random tree ordinary, the balanced tree short
    # a short tree's likelihood is (q t)^changes: weights that leave it a posterior share of 0.2 beside 0.3 and 0.5
    rates, freqs = split_params(params, 5)
    lls = np.asarray([go.truth(tips, peels[t], blens[t], rates, freqs).real for t in range(3)])
    logw = np.log([0.3, 0.2, 0.5]) - (lls - lls.max())
    out["one-short"] = TreesCase(tips, peels, blens, params, logw, None)
    return out


@functools.lru_cache(maxsize=None)
def summary_cases():
    out = collections.OrderedDict()
    for mean in (1e-4, 1e-8):
        c = tiny(3, S=4, mean=mean)
        out["S4-K3-m%g" % mean] = SummaryCase(c.tips, c.peel, c.blens, c.params, True)
    for mean in (1e-4, 1e-8):
        c = tiny(5, mean=mean)
        out["S7-K5-m%g" % mean] = SummaryCase(c.tips, c.peel, c.blens, c.params, False)
    c = discordant(3, 1e-4, S=4)
    out["S4-K3-discordant"] = SummaryCase(c.tips, c.peel, c.blens, c.params, True)
    return out


def split_params(params, K):
    R = geo.rate_count(K)
    return params[:R], params[R:]
