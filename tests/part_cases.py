"""Shared cases of the partitioned engine's tests: ``cases.random_case`` data
cut into partitions of given widths on one peel, per-partition parameter
points for every draw, the C oracle's rows at the scaled lengths and the
complex-step truth of d/dmu."""
import functools

import numpy as np

from phylostan_amd import models, partition as pt
from tests import cases

RTOL_LL, RTOL_G, RTOL_Q = 1e-10, 1e-9, 1e-8  # the project's bars (tests/test_gpu_parity.py, __graft_entry__.smoke)
AMBIGUITY = (15, 3, 5, 10, 6)

# (widths, S, C, model, rooted): the block-range walk at one and two columns per lane (a partition inside one
# block, ending on a block boundary, one column past it, of one column), the union of masks, the fold over K = 2..4
SHAPES = [
    ((1, 1), 7, 1, "JC69", False),
    ((63, 65), 8, 2, "HKY", True),
    ((64, 128, 129), 9, 4, "GTR", False),
    ((127, 1, 200), 10, 2, "GTR", True),
    ((130, 3, 64, 257), 12, 1, "HKY", False),
    ((63, 65), 11, 4, "JC69", True),
]
SHAPE_IDS = ["%s-S%d-C%d-%s-%s" % ("+".join(map(str, s[0])), s[1], s[2], s[3], "rooted" if s[4] else "unrooted")
             for s in SHAPES]


class PartCase:
    def __init__(self, widths, S, C, model, rooted, n, seed=3, ambiguous=0.1, clean=()):
        base = cases.random_case(seed, S=S, P=int(sum(widths)), C=C, model=model, rooted=rooted, ambiguous=ambiguous)
        self.widths, self.S, self.C, self.model, self.rooted, self.n = tuple(widths), S, C, model, rooted, n
        self.K = len(widths)
        self.peel0 = base.peel0
        self.B = base.blens.size
        self.kind = models.MODEL_IDS[model]
        rng = np.random.default_rng(seed + 77)
        off = np.concatenate([[0], np.cumsum(widths)])
        self.off = off
        self.parts = []
        for k in range(self.K):
            tip = base.tipcodes[:, off[k]:off[k + 1]].copy()
            if k in clean:  # no ambiguity codes at all
                tip = rng.choice([1, 2, 4, 8], size=tip.shape).astype(np.uint8)
            self.parts.append((tip, base.weights[off[k]:off[k + 1]].copy()))
        self.rowlen = 1 + self.B + 2 * C + 14
        self.outlen = 1 + self.B + self.K * (1 + 2 * C + 14)
        self.blens = rng.uniform(0.01, 0.3, (n, self.B))
        self.mu = rng.uniform(0.3, 2.5, (n, self.K))
        self.points = [[self._point(rng) for _ in range(self.K)] for _ in range(n)]
        self.model_vecs = np.array([[models.model_vector(*p) for p in row] for row in self.points])

    def _point(self, rng):
        freqs = rng.dirichlet(np.full(4, 5.0))
        rates = rng.uniform(0.5, 3.0, 6)
        if self.model == "HKY":
            rates = models.hky_exchangeabilities(rng.uniform(1.0, 8.0))
        if self.model == "JC69":
            freqs, rates = np.full(4, 0.25), np.ones(6)
        rs, ps = models.weibull_site_rates(rng.uniform(0.3, 2.0), self.C)
        return freqs, rates, rs, ps

    def case(self, d, k, blens=None):
        """Partition k of draw d as a single-alignment case at the scaled lengths (the rounded product)."""
        freqs, rates, rs, ps = self.points[d][k]
        bl = self.mu[d, k] * self.blens[d] if blens is None else blens
        return cases.Case("part%d_%d" % (d, k), self.parts[k][0], self.parts[k][1], self.peel0, self.rooted,
                          self.model, self.C, bl, freqs, rates, rs, ps)

    def evaluators(self):
        from oracle import cpu

        def make(k):
            tip, w = self.parts[k]
            return lambda bl, mv, site_ll: cpu.evaluate(tip, w, self.peel0, self.rooted, self.kind, mv, bl, self.C,
                                                        site_ll=site_ll)
        return [make(k) for k in range(self.K)]

    def host(self):
        return pt.partition_host(self.evaluators(), self.B, self.C, self.widths)

    @functools.lru_cache(maxsize=None)
    def truth(self):
        """(rows [n, K, rowlen], site [n, sum P_k]) of the C oracle, partition by partition."""
        evs = self.evaluators()
        rows = np.empty((self.n, self.K, self.rowlen))
        site = np.empty((self.n, int(self.off[-1])))
        for d in range(self.n):
            for k in range(self.K):
                row, s = evs[k](self.mu[d, k] * self.blens[d], self.model_vecs[d, k], True)
                rows[d, k] = row[:self.rowlen]
                site[d, self.off[k]:self.off[k + 1]] = s
        rows.setflags(write=False)
        site.setflags(write=False)
        return rows, site

    @functools.lru_cache(maxsize=None)
    def dmu_truth(self, draws=(0,)):
        """{(d, k): Im log L_k((mu_k + i h) t) / h}, h = 1e-30 (oracle/complex_step.py)."""
        from oracle import complex_step as cs
        out = {}
        for d in draws:
            for k in range(self.K):
                freqs, rates, rs, ps = self.points[d][k]
                bl = (self.mu[d, k] + 1j * cs.STEP) * self.blens[d].astype(complex)
                out[(d, k)] = cs.loglik(self.case(d, k), bl, freqs, rates, rs, ps)[0].imag / cs.STEP
        return out

    def engine(self, max_draws, device=0):
        return pt.PartitionedLikelihood(self.parts, self.peel0, self.rooted, self.model, self.C, max_draws=max_draws,
                                        device=device)

    def plan(self, max_draws, cu_count=0):
        return pt.plan_partitions([p[0] for p in self.parts], self.peel0, self.rooted, self.C, max_draws,
                                  model=self.model, cu_count=cu_count)


@functools.lru_cache(maxsize=None)
def shape_case(i, n=9):
    return PartCase(*SHAPES[i], n=n, seed=3 + i)


@functools.lru_cache(maxsize=None)
def ambiguity_case(n=3):
    """Partition 0 free of ambiguity codes, partition 1 carrying all of 15, 3, 5, 10, 6."""
    c = PartCase((70, 90), 8, 2, "GTR", True, n=n, seed=21, ambiguous=0.3, clean=(0,))
    present = set(np.unique(c.parts[1][0]).tolist())
    assert set(AMBIGUITY) <= present and not (set(AMBIGUITY) & set(np.unique(c.parts[0][0]).tolist()))
    return c


def _close(a, b, rtol, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    scale = max(np.max(np.abs(b)), 1e-300)
    err = np.max(np.abs(a - b)) / scale
    assert err <= rtol, "%s: max rel err %.3e > %.1e" % (what, err, rtol)


def check_truth(c, out, rows, site, draws=None, dmu_draws=(0,)):
    """Contract 1 on the first len(out) draws of ``c`` (or ``draws``)."""
    trows, tsite = c.truth()
    draws = list(range(len(out))) if draws is None else list(draws)
    B, C = c.B, c.C
    tail = 2 * C + 14
    for i, d in enumerate(draws):
        for k in range(c.K):
            r, ref = rows[i, k], trows[d, k]
            what = "draw %d partition %d" % (d, k)
            assert abs(r[0] - ref[0]) <= RTOL_LL * abs(ref[0]), "%s: log L %r vs %r" % (what, r[0], ref[0])
            sl = slice(c.off[k], c.off[k + 1])
            np.testing.assert_allclose(site[i, sl], tsite[d, sl], rtol=RTOL_LL, atol=1e-12, err_msg=what)
            o = 1 + B
            _close(r[1:o], ref[1:o], RTOL_G, what + " d/dblens")
            _close(r[o:o + C], ref[o:o + C], RTOL_G, what + " drs")
            _close(r[o + C:o + 2 * C], ref[o + C:o + 2 * C], RTOL_G, what + " dps")
            _close(r[o + 2 * C:o + 2 * C + 4], ref[o + 2 * C:o + 2 * C + 4], RTOL_G, what + " dfreqs (root)")
            if c.model != "JC69":  # the device's chain rule against the host's on the oracle's dL/dP
                _close(r[o + 2 * C + 4:o + 2 * C + 10], ref[o + 2 * C + 4:o + 2 * C + 10], RTOL_Q, what + " drates")
                _close(r[o + 2 * C + 10:], ref[o + 2 * C + 10:], RTOL_Q, what + " dfreqs")
            # the partition's block of the draw's row carries the same tail
            blk = out[i, 1 + B + k * (1 + tail):1 + B + (k + 1) * (1 + tail)]
            np.testing.assert_array_equal(blk[1:], r[1 + B:])
        ll = sum(trows[d, k, 0] for k in range(c.K))
        assert abs(out[i, 0] - ll) <= RTOL_LL * abs(ll), "draw %d: log L %r vs %r" % (d, out[i, 0], ll)
        dt = sum(c.mu[d, k] * trows[d, k, 1:1 + B] for k in range(c.K))
        _close(out[i, 1:1 + B], dt, RTOL_G, "draw %d d/dt" % d)
    truth = c.dmu_truth(tuple(d for d in dmu_draws if d in draws))
    for (d, k), ref in truth.items():
        i = draws.index(d)
        got = out[i, 1 + B + k * (1 + tail)]
        scale = float(np.sum(np.abs(c.blens[d] * trows[d, k, 1:1 + B])))
        print("d/dmu draw %d partition %d: %.17g vs complex step %.17g (err / scale %.2e)"
              % (d, k, got, ref, abs(got - ref) / scale))
        assert abs(got - ref) <= 1e-9 * scale, "draw %d d/dmu_%d: %r vs %r (scale %r)" % (d, k, got, ref, scale)


def check_fold(c, out, rows, draws=None):
    """Contract 2: out[d] is partition_combine_host of its rows, bit for bit."""
    draws = list(range(len(out))) if draws is None else list(draws)
    for i, d in enumerate(draws):
        np.testing.assert_array_equal(out[i], pt.partition_combine_host(rows[i], c.blens[d], c.mu[d]))
