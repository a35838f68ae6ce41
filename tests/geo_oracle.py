"""References of the discrete-trait (phylogeography) engine.  numpy only.

(a) ``stan_loglik``: a loop-for-loop restatement of the Stan the reference
    emits -- ``calculate_p_matrices`` (generate_script.py:895-950) with
    ``numpy.linalg.eigh`` for ``eigenvalues_sym`` / ``eigenvectors_sym``, and
    the pruning loop with ``target += log(sum(root))`` (:1085-1096).

(b) ``truth`` / ``truth_gradients``: shares no algebra with the kernel.  Q is
    built directly, P = expm(Q t) by scaling and squaring of a Taylor series
    (the scheme of ``oracle/complex_step.py`` for any K), everything on complex
    arrays, each partial derivative read as Im f(theta + i 1e-30) / 1e-30.
    ``extended=True`` normalises every internal partial by its largest real
    part and accumulates the logs, for trees whose likelihood leaves the fp64
    range.

Also the small generators the tests share (peels, tip partials, draws) and the
oracle-backed likelihood the CPU suite hands to ``cli.run``.
"""
import argparse
import os

import numpy as np

from phylostan_amd.geo import geo_gradients_host, rate_count, rate_pairs

STEP = 1e-30
_TAYLOR_TERMS = 20  # |X| <= 1/2: the first dropped term is 2^-21 / 21! ~ 1e-26


# ------------------------------------------------------------------ (a)
def stan_p_matrices(states, freqs, rates, blens):
    bcount = len(blens)
    pmats = [None] * bcount
    s = 0.0
    P2 = np.diag(np.sqrt(freqs))
    P2inv = np.diag(1.0 / np.sqrt(freqs))
    R = np.zeros((states, states))
    index = 1
    for col in range(1, states):
        for row in range(col + 1, states + 1):
            R[row - 1, col - 1] = rates[index - 1]
            R[col - 1, row - 1] = R[row - 1, col - 1]
            index = index + 1
    Q = R @ np.diag(freqs)
    for i in range(states):
        Q[i, i] = 0.0
        Q[i, i] = -np.sum(Q[i, :])
        s -= Q[i, i] * freqs[i]
    Q = Q / s
    A = P2 @ Q @ P2inv
    eigenvalues, eigenvectors = np.linalg.eigh(0.5 * (A + A.T))  # eigen*_sym read one triangle
    m1 = P2inv @ eigenvectors
    m2 = eigenvectors.T @ P2
    for b in range(bcount):
        if blens[b] != 0.0:
            pmats[b] = m1 @ np.diag(np.exp(eigenvalues * blens[b])) @ m2
        else:
            pmats[b] = np.diag(np.ones(states))
    return pmats


def stan_loglik(tips, peel, blens, rates, freqs):
    """peel 0-based; returns target (a float; -inf when the root sum is 0)."""
    S, K = tips.shape
    pm = stan_p_matrices(K, np.asarray(freqs, float), np.asarray(rates, float), np.asarray(blens, float))
    partials = [None] * (2 * S - 1)
    for n in range(S):
        partials[n] = np.asarray(tips[n], float)
    for n in range(S - 2):
        a, b, p = peel[n]
        partials[p] = (pm[a] @ partials[a]) * (pm[b] @ partials[b])
    a, b, p = peel[S - 2]
    partials[p] = (pm[a] @ partials[a]) * partials[b]
    with np.errstate(divide="ignore"):
        return float(np.log(np.sum(partials[p])))


# ------------------------------------------------------------------ (b)
def expm(A):
    """exp of complex matrices A[..., K, K]: each scaled by its own power of
    two to a row-sum norm <= 1/2, a Taylor series, squared back."""
    A = np.asarray(A, complex)
    K = A.shape[-1]
    nrm = np.abs(A).sum(-1).max(-1)
    s = np.where(nrm > 0, np.ceil(np.log2(np.maximum(nrm, 1e-300))) + 1, 0.0)
    s = np.maximum(s, 0.0).astype(np.int64)
    X = A / np.exp2(s)[..., None, None]
    T = np.broadcast_to(np.eye(K, dtype=complex), A.shape).copy()
    term = T.copy()
    for k in range(1, _TAYLOR_TERMS + 1):
        term = term @ X / k
        T = T + term
    for j in range(int(s.max()) if s.size else 0):
        T = np.where((s > j)[..., None, None], T @ T, T)
    return T


def build_q(freqs, rates):
    f = np.asarray(freqs, complex)
    r = np.asarray(rates, complex)
    K = f.size
    R = np.zeros((K, K), complex)
    for k, (row, col) in enumerate(rate_pairs(K)):
        R[row, col] = R[col, row] = r[k]
    Q = R * f[None, :]
    idx = np.arange(K)
    Q[idx, idx] = 0.0
    Q[idx, idx] = -Q.sum(1)
    return Q / (-np.dot(np.diag(Q), f))


def truth(tips, peel, blens, rates, freqs, extended=False):
    """Complex log L at (possibly complex) parameters."""
    S, K = tips.shape
    t = np.asarray(blens, complex)
    pm = expm(build_q(freqs, rates)[None] * t[:, None, None])
    part = {n: np.asarray(tips[n], complex) for n in range(S)}
    logs = 0.0 + 0.0j
    last = len(peel) - 1
    for r, (a, b, p) in enumerate(peel):
        v = (pm[a] @ part[a]) * (part[b] if r == last else pm[b] @ part[b])
        if extended:
            m = v[np.argmax(v.real)]
            v = v / m
            logs = logs + np.log(m)
        part[p] = v
    return np.log(part[peel[-1][2]].sum()) + logs


def truth_gradients(tips, peel, blens, rates, freqs, extended=False, max_entries=None, seed=0):
    """(log L, {name: (indices, complex-step derivatives)}) for blens, rates
    and freqs.  ``max_entries`` checks that many seeded entries of each array
    (one complex evaluation each); None: all."""
    args = {"blens": np.asarray(blens, float), "rates": np.asarray(rates, float), "freqs": np.asarray(freqs, float)}
    ll = truth(tips, peel, extended=extended, **args).real
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
            g[n] = truth(tips, peel, extended=extended, **z).imag / STEP
        out[name] = (idx, g)
    return float(ll), out


# ------------------------------------------------------------------ generators
def random_peel(S, rng):
    """A random tree's peel, 0-based, internal nodes S.. in creation order, the
    last row (child1, 2S-3, 2S-2)."""
    nodes = list(range(S))
    peel = []
    nxt = S
    while len(nodes) > 1:
        i, j = rng.choice(len(nodes), 2, replace=False)
        a, b = nodes[i], nodes[j]
        nodes = [n for k, n in enumerate(nodes) if k not in (i, j)] + [nxt]
        peel.append((int(a), int(b), nxt))
        nxt += 1
    a, b, p = peel[-1]  # node 2S-3 was made when three nodes were left, so it is a root child
    peel[-1] = (min(a, b), max(a, b), p)
    return np.asarray(peel, np.int32)


def caterpillar_peel(S):
    """One internal node per level: ((0,1),2),3)... ; the last row joins tip
    S-1 to the ladder, which is node 2S-3."""
    peel = [(0, 1, S)]
    for k in range(2, S - 1):
        peel.append((S + k - 2, k, S + k - 1))
    peel.append((S - 1, 2 * S - 3, 2 * S - 2))
    return np.asarray(peel, np.int32)


def random_tips(S, K, rng, missing=(0,)):
    tips = np.zeros((S, K))
    tips[np.arange(S), rng.integers(0, K, S)] = 1.0
    for m in missing:
        tips[m] = 1.0
    return tips


def random_draws(n, B, K, rng, mean_blen=0.3):
    """(blens [n, B], params [n, R + K]) with distinct parameters."""
    blens = rng.exponential(mean_blen, (n, B))
    rates = 0.1 + rng.exponential(1.0, (n, rate_count(K)))
    freqs = rng.dirichlet(np.ones(K) * 3.0, n)
    return blens, np.concatenate([rates, freqs], axis=1)


class HostGeoLikelihood:
    """``evaluate_rows`` on ``geo_gradients_host``: what the CPU suite gives
    ``cli.run`` in place of the device engine."""

    def __init__(self, tips, peel0, max_draws=128, device=0):
        self.tips = np.asarray(tips, float)
        self.peel = np.asarray(peel0)
        self.S, self.K = self.tips.shape
        self.R = rate_count(self.K)
        self.B = 2 * self.S - 3
        self.calls = 0

    def evaluate_rows(self, blens, params):
        blens, params = np.atleast_2d(blens), np.atleast_2d(params)
        self.calls += 1
        rows = np.empty((blens.shape[0], 1 + self.B + self.R + self.K))
        for n in range(blens.shape[0]):
            ll, gb, gr, gf = geo_gradients_host(self.tips, self.peel, blens[n], params[n, :self.R],
                                                params[n, self.R:])
            rows[n] = np.concatenate([[ll], gb, gr, gf])
        return rows

    def close(self):
        pass


# ------------------------------------------------------------------ the CLI
def write_geo_dataset(dirname, S, K, seed, negative=False):
    """A random tree (newick) and a metadata table with K locations."""
    rng = np.random.default_rng(seed)
    peel = random_peel(S, rng)
    text = {n: "t%d" % (n + 1) for n in range(S)}
    for a, b, p in peel:
        la, lb = rng.exponential(0.3, 2)
        if negative and p == S:
            la = -0.01
        text[p] = "(%s:%.6f,%s:%.6f)" % (text[a], la, text[b], lb)
    tree = os.path.join(dirname, "geo.tree")
    with open(tree, "w") as fp:
        fp.write(text[2 * S - 2] + ";\n")
    places = ["P%d" % k for k in range(K)]
    where = [places[k] for k in range(K)] + [places[int(k)] for k in rng.integers(0, K, S - K)]
    meta = os.path.join(dirname, "meta.tsv")
    with open(meta, "w") as fp:
        fp.write("strain\tCountry\tRegion\n")
        for n in rng.permutation(S):
            fp.write("t%d\t%s\tR%d\n" % (n + 1, where[n], n % 2))
    return tree, meta


def run_geo(argv, factory=None, host=True, **kw):
    from phylostan_amd import cli
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    arg = parser.parse_args(["run"] + argv)
    lines = []
    if factory is None and host:
        factory = HostGeoLikelihood
    post = cli.run(arg, likelihood_factory=factory, log=lines.append, **kw)
    return post, lines
