"""Shared by the forest tests: forests of peels on one alignment, per-row
parameter points and the per-row truth (``oracle.cpu.evaluate`` on the row's
own peel)."""
import functools
import os

import numpy as np

from phylostan_amd import models
from tests import cases


def caterpillar_peel(S):
    return cases.random_peel(S, None, caterpillar=True)


def balanced_peel(S):
    """Neighbours joined level by level, internal nodes numbered in creation order."""
    nodes, nxt, peel = list(range(S)), S, []
    while len(nodes) > 1:
        a, b = nodes.pop(0), nodes.pop(0)
        peel.append([a, b, nxt])
        nodes.append(nxt)
        nxt += 1
    return np.array(peel, dtype=np.int32)


def forest_peels(S, rooted, seeds, shapes=True):
    """[caterpillar, balanced,] then one random peel per seed; unrooted peels
    follow the (child1, 2S-3) last-row rule."""
    peels = [caterpillar_peel(S), balanced_peel(S)] if shapes else []
    peels += [cases.random_peel(S, np.random.default_rng(s)) for s in seeds]
    if not rooted:
        peels = [cases.make_unrooted(p) for p in peels]
    return np.array(peels, dtype=np.int32)


class Forest:
    """An alignment, T peels and n parameter rows (each with its tree)."""

    def __init__(self, tipcodes, weights, peels, rooted, model, C, tree_of_row, blens, model_vecs):
        self.tipcodes, self.weights, self.peels = tipcodes, weights, np.asarray(peels, dtype=np.int32)
        self.rooted, self.model, self.C = rooted, model, C
        self.tree_of_row = np.asarray(tree_of_row, dtype=np.int32)
        self.blens, self.model_vecs = np.asarray(blens), np.asarray(model_vecs)
        self.S, self.P = tipcodes.shape
        self.B = blens.shape[1]
        self.outlen = 1 + self.B + 2 * C + 14
        self._truth = None

    def truth(self):
        """(rows [n, outlen], site_ll [n, P]) from the oracle, computed once."""
        if self._truth is None:
            from oracle import cpu
            rows, sites = [], []
            for t, bl, mv in zip(self.tree_of_row, self.blens, self.model_vecs):
                out, sl = cpu.evaluate(self.tipcodes, self.weights, self.peels[t], self.rooted,
                                       models.MODEL_IDS[self.model], mv, bl, self.C, site_ll=True)
                rows.append(out[:self.outlen])
                sites.append(sl)
            self._truth = (np.array(rows), np.array(sites))
        return self._truth

    def engine(self, max_rows, peels=None):
        from phylostan_amd.forest import ForestLikelihood
        return ForestLikelihood(self.tipcodes, self.weights, self.peels if peels is None else peels, self.rooted,
                                self.model, self.C, max_rows=max_rows)


def random_rows(rng, n, B, C, model):
    """n parameter points: branch lengths and model vectors, all different."""
    blens = rng.uniform(0.01, 0.3, (n, B))
    mvs = []
    for _ in range(n):
        freqs, rates = np.full(4, 0.25), np.ones(6)
        if model != "JC69":
            freqs = rng.dirichlet(np.full(4, 5.0))
            rates = rng.uniform(0.5, 3.0, 6) if model == "GTR" else models.hky_exchangeabilities(rng.uniform(1.0, 8.0))
        rs, ps = models.weibull_site_rates(rng.uniform(0.3, 2.0), C)
        mvs.append(models.model_vector(freqs, rates, rs, ps))
    return blens, np.array(mvs)


@functools.lru_cache(maxsize=None)
def random_forest(seed, S, P, C, model, rooted, tree_of_row=(3, 0, 0, 2, 1, 3, 1, 2, 0), seeds=(1, 2)):
    base = cases.random_case(seed, S=S, P=P, C=C, model=model, rooted=True)  # the data and weights only
    peels = forest_peels(S, rooted, [seed * 100 + s for s in seeds])
    B = 2 * S - 2 if rooted else 2 * S - 3
    blens, mvs = random_rows(np.random.default_rng(seed + 7), len(tree_of_row), B, C, model)
    return Forest(base.tipcodes, base.weights, peels, rooted, model, C, tree_of_row, blens, mvs)


@functools.lru_cache(maxsize=None)
def ds1_forest():
    """The 42 DS1 topologies in topology 0's tip order: tip j of topology k is
    row perm[k][j] of tipbits0, so its peel's tip ids and its tip branch
    lengths move through perm[k].  Returns (tipbits0, weights, peels [42],
    blens [42] at the fixture's points, the reference site_ll and loglik)."""
    d = np.load(os.path.join(cases.GOLDEN, "DS1_topologies.npz"), allow_pickle=False)
    tip0, perm = d["tipbits0"], d["perm"]
    S = tip0.shape[0]
    peels, blens, site, ll = [], [], [], []
    for k in range(perm.shape[0]):
        j = int(np.nonzero(d["ll_topologies"] == k)[0][0])
        peel = d["peel"][k].astype(np.int64) - 1
        tipmask = peel < S
        peel[tipmask] = perm[k][peel[tipmask]]
        bl = np.array(d["blens"][j], dtype=np.float64)
        out = bl.copy()
        out[perm[k]] = bl[:S]
        peels.append(peel)
        blens.append(out)
        site.append(d["site_ll"][j])
        ll.append(float(d["loglik"][j]))
    return tip0, d["weights"], np.array(peels, dtype=np.int32), np.array(blens), np.array(site), np.array(ll)
