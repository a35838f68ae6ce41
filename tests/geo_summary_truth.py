"""Truths of the phylogeography summaries (``phy_geo_eval_summaries``,
``geo.geo_summaries_host``) that share no algebra with the kernel.  numpy only.

* ``brute_marginals``: the posterior state distribution of every node by
  enumeration of all joint assignments of the 2S-2 nodes below the root (the
  merged root child 2S-3 *is* the root of the unrooted tree: the two share one
  state), each weighted by its tip partials and the entries of P_b = expm(Q t_b).
* ``jump_truth``: Minin and Suchard's expectations as derivatives of log L with
  respect to the entries of Q itself, ``E[N_ij] = Q_ij dlogL/dQ_ij`` and
  ``E[T_i] = dlogL/dQ_ii``, each read as ``Im log L(Q + i 1e-30 E_ij) / 1e-30``.
  Q is perturbed directly: not renormalised, its diagonal not adjusted.
* ``branch_jump_truth``: the same with Q perturbed on one branch only, along
  ``Q_off`` (Q with a zero diagonal): ``sum_{i != j} Q_ij dlogL/dQ^(b)_ij`` is
  that directional derivative, one complex evaluation per branch.

P = expm(Q t) is ``geo_oracle.expm`` (scaling and squaring of a Taylor series).
"""
import itertools

import numpy as np

from tests.geo_oracle import STEP, build_q, expm


def loglik_q(tips, peel, blens, Qs):
    """Complex log L with branch b's generator ``Qs[b]`` (``Qs [B, K, K]``)."""
    S, K = tips.shape
    t = np.asarray(blens, complex)
    pm = expm(np.asarray(Qs, complex) * t[:, None, None])
    part = {n: np.asarray(tips[n], complex) for n in range(S)}
    last = len(peel) - 1
    for r, (a, b, p) in enumerate(peel):
        v = (pm[a] @ part[a]) * (part[b] if r == last else pm[b] @ part[b])
        part[p] = v
    return np.log(part[peel[-1][2]].sum())


def jump_truth(tips, peel, blens, rates, freqs, entries=None):
    """``{(i, j): value}``: E[N_ij] for i != j, E[T_i] for i == j, at ``entries``
    (a list of pairs; None: all K^2)."""
    K = tips.shape[1]
    B = len(blens)
    Q = build_q(freqs, rates)
    if entries is None:
        entries = [(i, j) for i in range(K) for j in range(K)]
    out = {}
    for i, j in entries:
        Qp = Q.copy()
        Qp[i, j] += 1j * STEP
        d = loglik_q(tips, peel, blens, np.broadcast_to(Qp, (B, K, K))).imag / STEP
        out[(i, j)] = d if i == j else Q[i, j].real * d
    return out


def jump_matrix(tips, peel, blens, rates, freqs):
    K = tips.shape[1]
    out = np.zeros((K, K))
    for (i, j), v in jump_truth(tips, peel, blens, rates, freqs).items():
        out[i, j] = v
    return out


def branch_jump_truth(tips, peel, blens, rates, freqs, branches=None):
    """E[transitions on branch b] for each b of ``branches`` (None: all)."""
    K = tips.shape[1]
    B = len(blens)
    Q = build_q(freqs, rates)
    Qoff = Q.copy()
    Qoff[np.arange(K), np.arange(K)] = 0.0
    branches = range(B) if branches is None else branches
    out = []
    for b in branches:
        Qs = np.broadcast_to(Q, (B, K, K)).copy()
        Qs[b] = Q + 1j * STEP * Qoff
        out.append(loglik_q(tips, peel, blens, Qs).imag / STEP)
    return np.asarray(out)


def brute_marginals(tips, peel, blens, rates, freqs):
    """marg [2S-1, K] by enumeration; K^(2S-2) joint states, so S <= 5 or so."""
    tips = np.asarray(tips, float)
    S, K = tips.shape
    N = 2 * S - 1
    root, merged = N - 1, N - 2
    P = expm(build_q(freqs, rates)[None] * np.asarray(blens, complex)[:, None, None]).real
    parent = {}
    for a, b, p in peel:
        parent[int(a)] = int(p)
        parent[int(b)] = int(p)
    marg = np.zeros((N, K))
    for x in itertools.product(range(K), repeat=N - 1):
        state = list(x) + [x[merged]]  # the root shares the merged child's state
        w = 1.0
        for n in range(N - 1):
            if n < S:
                w *= tips[n, state[n]]
            if n != merged:
                w *= P[n, state[parent[n]], state[n]]
            if w == 0.0:
                break
        if w == 0.0:
            continue
        for n in range(N):
            marg[n, state[n]] += w
    return marg / marg[root].sum()
