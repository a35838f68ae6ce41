"""Truths of the tree-sample (mixture) phylogeography engine
(``phy_geo_trees_*``, ``geo.geo_trees_host``) that share no algebra with the
kernel, and the samples the CPU and GPU suites share.  numpy only.

* ``mix_truth``: per tree the complex log L_t of ``geo_oracle.truth`` (P =
  expm(Q t), no eigensystem), combined by a complex log-sum-exp with log w_t.
* ``mix_truth_gradients``: each derivative as Im f(theta + 1e-30 i) / 1e-30.
* ``summaries_truth``: the p_t-weighted means of ``geo_summary_truth``'s
  Minin-Suchard counts and of the root's marginal.  The root marginal of one
  tree is its normalised root partial, pruned with expm(Q t) (``root_truth``);
  tests/test_geo_trees_cpu.py pins that to ``brute_marginals`` at S = 4.
"""
import math

import numpy as np

from phylostan_amd.geo import rate_count
from tests import geo_oracle as go
from tests import geo_summary_truth as gst

STEP = go.STEP

# the three unrooted topologies of four tips: 01|23, 02|13, 03|12
S4_PEELS = np.asarray([[(0, 1, 4), (2, 3, 5), (4, 5, 6)],
                       [(0, 2, 4), (1, 3, 5), (4, 5, 6)],
                       [(0, 3, 4), (1, 2, 5), (4, 5, 6)]], np.int32)


def balanced_peel(S):
    """Tips paired level by level (ceil(log2 S) levels); the last row is (x, 2S-3, 2S-2)."""
    live = list(range(S))
    peel = []
    nxt = S
    while len(live) > 1:
        a, b = live.pop(0), live.pop(0)
        peel.append((a, b, nxt))
        live.append(nxt)
        nxt += 1
    a, b, p = peel[-1]
    peel[-1] = (min(a, b), max(a, b), p)
    return np.asarray(peel, np.int32)


def mixed_peels(S, T, rng):
    """T peels of S tips: at S = 4 the three topologies in turn; otherwise a
    caterpillar, a balanced tree (their level counts differ), then random
    trees."""
    if S == 4:
        return np.stack([S4_PEELS[t % 3] for t in range(T)])
    out = []
    for t in range(T):
        out.append(go.caterpillar_peel(S) if t == 0 else balanced_peel(S) if t == 1 else go.random_peel(S, rng))
    return np.stack(out)


def make_sample(S, K, T, seed, missing=(0,), mean_blen=0.3, peels=None):
    """(tips, peels [T, S-1, 3], blens [T, B], params [R + K]); tip 0 all ones
    unless ``missing`` says otherwise, one zero-length branch in tree 0."""
    rng = np.random.default_rng(seed)
    peels = mixed_peels(S, T, rng) if peels is None else np.asarray(peels, np.int32)
    tips = go.random_tips(S, K, rng, missing=missing)
    blens = rng.exponential(mean_blen, (T, 2 * S - 3))
    blens[0, 1] = 0.0
    _, params = go.random_draws(1, 2 * S - 3, K, rng)
    return tips, peels, blens, params[0]


def uniform_logw(T):
    return np.full(T, -math.log(T))


def mix_truth(tips, peels, blens, rates, freqs, logw, extended=False):
    """(complex log L_mix, complex log L_t [T])."""
    lls = np.asarray([go.truth(tips, peels[t], blens[t], rates, freqs, extended=extended)
                      for t in range(len(peels))], complex)
    x = lls + np.asarray(logw, float)
    m = x[np.argmax(x.real)]
    return m + np.log(np.exp(x - m).sum()), lls


def mix_truth_gradients(tips, peels, blens, rates, freqs, logw, extended=False, max_entries=None, seed=0):
    """(log L_mix, log L_t [T], {name: (indices, derivatives)}) for rates and freqs."""
    args = {"rates": np.asarray(rates, float), "freqs": np.asarray(freqs, float)}
    lmix, lls = mix_truth(tips, peels, blens, logw=logw, extended=extended, **args)
    rng = np.random.default_rng(seed)
    out = {}
    for name, x in args.items():
        idx = np.arange(x.size)
        if max_entries is not None and x.size > max_entries:
            idx = np.sort(rng.choice(x.size, max_entries, replace=False))
        g = np.empty(idx.size)
        for n, k in enumerate(idx):
            z = {m: v.astype(complex) for m, v in args.items()}
            z[name][k] += 1j * STEP
            g[n] = mix_truth(tips, peels, blens, logw=logw, extended=extended, **z)[0].imag / STEP
        out[name] = (idx, g)
    return float(lmix.real), lls.real.copy(), out


def root_truth(tips, peel, blens, rates, freqs):
    """The root's posterior state distribution: the normalised root partial, pruned with P = expm(Q t)."""
    S, K = tips.shape
    pm = go.expm(go.build_q(freqs, rates)[None] * np.asarray(blens, complex)[:, None, None]).real
    part = {n: np.asarray(tips[n], float) for n in range(S)}
    last = len(peel) - 1
    for r, (a, b, p) in enumerate(peel):
        part[p] = (pm[a] @ part[a]) * (part[b] if r == last else pm[b] @ part[b])
    v = part[peel[-1][2]]
    return v / v.sum()


def tree_weights(lls, logw):
    """p_t from real log L_t and log w_t."""
    x = np.asarray(lls, float) + np.asarray(logw, float)
    w = np.exp(x - x.max())
    return w / w.sum()


def summaries_truth(tips, peels, blens, rates, freqs, logw):
    """(jumps [K, K], root [K], p [T])."""
    K = tips.shape[1]
    _, lls = mix_truth(tips, peels, blens, rates, freqs, logw)
    p = tree_weights(lls.real, logw)
    jumps = np.zeros((K, K))
    root = np.zeros(K)
    for t in range(len(peels)):
        jumps += p[t] * gst.jump_matrix(tips, peels[t], blens[t], rates, freqs)
        root += p[t] * root_truth(tips, peels[t], blens[t], rates, freqs)
    return jumps, root, p


def split_params(params, K):
    R = rate_count(K)
    return params[:R], params[R:]


class HostGeoTreesLikelihood:
    """``evaluate_rows`` / ``evaluate_summaries`` on the host restatements:
    what the CPU suite gives ``cli.run --geo --trees`` in place of the device
    engine."""

    def __init__(self, tips, peels, blens, log_weights=None, max_draws=128, device=0):
        from phylostan_amd import geo
        self.geo = geo
        self.tips = np.asarray(tips, float)
        self.peels = np.asarray(peels)
        self.blens = np.asarray(blens, float)
        self.S, self.K = self.tips.shape
        self.T = self.peels.shape[0]
        self.R = rate_count(self.K)
        self.log_weights = uniform_logw(self.T) if log_weights is None else np.asarray(log_weights, float)
        self.tree_loglik = None

    def evaluate_rows(self, params):
        params = np.atleast_2d(params)
        rows = np.empty((params.shape[0], 1 + self.R + self.K))
        self.tree_loglik = np.empty((params.shape[0], self.T))
        for n in range(params.shape[0]):
            ll, gr, gf, tll = self.geo.geo_trees_host(self.tips, self.peels, self.blens, params[n, :self.R],
                                                      params[n, self.R:], self.log_weights)
            rows[n] = np.concatenate([[ll], gr, gf])
            self.tree_loglik[n] = tll
        return rows

    def evaluate_summaries(self, params):
        params = np.atleast_2d(params)
        rows = self.evaluate_rows(params)
        jumps = np.empty((params.shape[0], self.K, self.K))
        root = np.empty((params.shape[0], self.K))
        for n in range(params.shape[0]):
            jumps[n], root[n] = self.geo.geo_trees_summaries_host(self.tips, self.peels, self.blens,
                                                                  params[n, :self.R], params[n, self.R:],
                                                                  self.log_weights)
        return rows, jumps, root

    def tree_posterior(self, rows):
        return self.geo.tree_posterior(self.tree_loglik, self.log_weights, np.asarray(rows)[:, 0])

    def close(self):
        pass
