"""The edge draws of the exact partitioned tests (tests/test_part_exact_cpu.py
on the CPU, tests/test_part_exact_gpu.py on the GPU): the parameter points of
tests/exact_cases.py -- spectral ties, near ties, ill-conditioned models,
extreme and zero site rates -- given to the three partitions of a draw, each
draw with its own branch lengths and relative rates (short, zero and saturated
branches, mu = (1e-4, 1, 200), mu = 1 exactly), and the complex-step truth of
every (draw, partition) row (oracle/complex_step.py on the partition's own
sub-alignment at the rounded product mu_k t), computed once per process.

Two alignments, because the model is a context's: the data of
``exact_cases._hky3()`` (HKY) and of ``exact_cases._gtr7()`` (GTR), both S = 12,
P = 130, C = 4, cut into K = 3 partitions of 64, 65 and 1 columns: one ending
on a block boundary, one a column past it (two blocks at one column per lane:
its dL/dP slots take the first block's store and the later block's add), one
of a single column.  A context holds one tree of
``forest_cases.forest_peels(12, rooted, [301, 302])``: 0 the caterpillar (no
deep entries), 1 balanced (two), 2 random301 (one); balanced unless a form
says otherwise.  Branch b is the branch above node b, so one ``t`` vector
serves every peel; an unrooted context takes its first 2S - 3 entries.

A draw's truth is the plain sum of its partitions': log L = sum_k log L_k,
d/dt = sum_k mu_k g_k, and d/dmu_k = Im log L_k((mu_k + i h) t) / h, h = 1e-30.
"""
import functools

import numpy as np

from oracle import complex_step as cs
from phylostan_amd import models, partition as pt
from tests import cases
from tests import exact_cases as ec
from tests import forest_cases as fc
from tests import forest_exact_cases as fx

S, P, C, K = 12, 130, 4, 3
WIDTHS = (64, 65, 1)
SEEDS = fx.SEEDS
TREES = ("caterpillar", "balanced", "random301")
BALANCED, CATERPILLAR = 1, 0
TIE, NEAR, GENERIC, OTHER = fx.TIE, fx.NEAR, fx.GENERIC, fx.OTHER

# point -> (its kind, the maker of its parameters): the forest file's entries, parameters only
_POINT = {name: (kind, make) for model in ("HKY", "GTR") for name, kind, make, _ in fx.POINTS[model]}

# Partition k of draw d carries ORDER[(d + k) % len(ORDER)]: every point sits on all three partitions (the
# one-column one among them) once the draws are at least as many as the points.  HKY opens (generic, near
# tie, exact tie).
ORDER = {
    "HKY": ("ctl_hky3", "near_5e-13", "tie2_hky3", "near_1e-11", "tie3_f81_hky7", "near_1e-9", "cond_kappa1000",
            "near_1e-7", "near_kappa1"),
    "GTR": ("ctl_gtr7", "tie3_jc_as_gtr7", "cond_freq1e-6", "cond_rates", "rs_weibull005", "rs0_gtr7"),
}
MU_EXTREME = (1e-4, 1.0, 200.0)  # partition 0 all short, partition 2 (the single column) saturated
# draw -> what its branch lengths and rates are (every other draw: generic t and mu, as part_cases.PartCase's)
SPECIAL = {
    "HKY": {3: "mu_extreme", 5: "mu_one"},
    "GTR": {2: "short_1e-4", 3: "short_1e-8", 4: "long_50", 5: "zero_internal", 6: "mu_extreme", 7: "mu_one"},
}
N_DRAWS = 9
# the C = 10 context (the 1,024-thread one-column forms): HKY, two draws over four points
DRAWS_C10 = (("ctl_hky3", "near_5e-13", "tie2_hky3"), ("near_1e-9", "tie2_hky3", "near_5e-13"))
C10_SHAPE = fx.C10_SHAPE
SHORT_T = {"short_1e-4": 1e-4, "short_1e-8": 1e-8}

ROW_ARRAYS = ec.ARRAYS + ("dmu",)
DRAW_ARRAYS = ("loglik", "grad_blens")


def _draw_t_mu(kind, t, mu):
    """The draw's branch lengths (all 2S - 2 of them) and rates from the generic ones."""
    t, mu = t.copy(), mu.copy()
    if kind in SHORT_T:
        t[::3] = SHORT_T[kind]
    elif kind == "long_50":
        t[1::5] = 50.0
    elif kind == "zero_internal":  # internal branches only: a zero tip branch makes a site impossible
        t[S::3] = 0.0
    elif kind == "mu_extreme":
        mu[:] = MU_EXTREME
    elif kind == "mu_one":
        mu[:] = 1.0
    else:
        assert kind == "generic", kind
    return t, mu


class Row:
    """Partition ``k`` of draw ``d``: its point and the single-alignment case at the scaled lengths."""

    def __init__(self, d, k, point, kind, draw_kind, case, short):
        self.d, self.k, self.point, self.kind, self.draw_kind, self.case, self.short = (d, k, point, kind, draw_kind,
                                                                                        case, short)

    @property
    def name(self):
        return "draw %d (%s) partition %d %s" % (self.d, self.draw_kind, self.k, self.point)


class EdgePart:
    """One alignment in three partitions on one tree, and the edge draws:
    ``blens [n, B]``, ``mu [n, 3]``, ``model_vecs [n, 3, 10 + 2C]`` as
    ``PartitionedLikelihood.evaluate_rows`` takes them; ``rows[d][k]`` is what
    the truth and the bounds of partition k of draw d are computed from."""

    def __init__(self, model, rooted, C_, tree):
        base = ec._hky3() if model == "HKY" else ec._gtr7()
        assert (base.S, base.P, base.model) == (S, P, model)
        self.model, self.rooted, self.C, self.tree, self.K = model, rooted, C_, tree, K
        self.widths = WIDTHS
        self.off = np.concatenate([[0], np.cumsum(WIDTHS)])
        self.parts = [(base.tipcodes[:, self.off[k]:self.off[k + 1]].copy(),
                       base.weights[self.off[k]:self.off[k + 1]].copy()) for k in range(K)]
        self.peel0 = fc.forest_peels(S, rooted, list(SEEDS))[tree]
        self.B = 2 * S - 2 if rooted else 2 * S - 3
        self.rowlen = 1 + self.B + 2 * C_ + 14
        self.outlen = 1 + self.B + K * (1 + 2 * C_ + 14)
        if C_ == 10:
            assert model == "HKY"
            points, special = DRAWS_C10, {}
        else:
            order = ORDER[model]
            points = [tuple(order[(d + k) % len(order)] for k in range(K)) for d in range(N_DRAWS)]
            special = SPECIAL[model]
        self.n = len(points)
        rng = np.random.default_rng(2024 if model == "HKY" else 2025)  # the same draws rooted and unrooted
        t_all = rng.uniform(0.01, 0.3, (N_DRAWS, 2 * S - 2))
        mu_all = rng.uniform(0.3, 2.5, (N_DRAWS, K))
        self.draw_kinds = [special.get(d, "generic") for d in range(self.n)]
        blens, mu, self.rows = [], [], []
        for d in range(self.n):
            t, m = _draw_t_mu(self.draw_kinds[d], t_all[d], mu_all[d])
            t = t[:self.B]
            row = []
            for k in range(K):
                kind, make = _POINT[points[d][k]]
                c = make()
                rs, ps = (c.rs, c.ps) if C_ == c.C else models.weibull_site_rates(C10_SHAPE, C_)
                case = cases.Case("d%d_p%d_%s" % (d, k, points[d][k]), self.parts[k][0], self.parts[k][1], self.peel0,
                                  rooted, model, C_, m[k] * t, c.freqs, c.rates, rs, ps)
                # the rows with branches of 1e-4 or less: the two short draws and the mu = 1e-4 partition
                short = self.draw_kinds[d] in SHORT_T or (self.draw_kinds[d] == "mu_extreme" and k == 0)
                row.append(Row(d, k, points[d][k], kind, self.draw_kinds[d], case, short))
            blens.append(t)
            mu.append(m)
            self.rows.append(row)
        self.blens, self.mu = np.array(blens), np.array(mu)
        self.model_vecs = np.array([[r.case.model_vec() for r in row] for row in self.rows])
        for a in (self.blens, self.mu, self.model_vecs):
            a.setflags(write=False)
        self._truth = self._bounds = None

    def flat_rows(self):
        return [r for row in self.rows for r in row]

    # ---------------------------------------------------------------- truth
    def truth(self):
        """[n][K] dicts: ``exact_cases.ARRAYS`` of the partition at mu_k t and
        ``dmu`` (with ``dmu_scale`` = sum_b |t_b g_kb|), all finite and
        read-only; computed once."""
        if self._truth is None:
            out = []
            for d, row in enumerate(self.rows):
                tr = []
                for r in row:
                    c = r.case
                    t = ec.truth_of(c)
                    bl = (self.mu[d, r.k] + 1j * cs.STEP) * self.blens[d].astype(complex)
                    t["dmu"] = float(cs.loglik(c, bl, c.freqs, c.rates, c.rs, c.ps)[0].imag / cs.STEP)
                    t["dmu_scale"] = float(np.sum(np.abs(self.blens[d] * t["grad_blens"])))
                    for name, v in t.items():
                        assert np.all(np.isfinite(v)), "the truth of %s has a non-finite %s" % (r.name, name)
                    tr.append(t)
                out.append(tr)
            self._truth = out
        return self._truth

    def draw_truth(self, d):
        """log L = sum_k log L_k and d/dt = sum_k mu_k g_k of draw d."""
        tr = self.truth()[d]
        return dict(loglik=sum(t["loglik"] for t in tr),
                    grad_blens=sum(self.mu[d, k] * tr[k]["grad_blens"] for k in range(K)))

    def row_errors(self, d, k, res):
        """``exact_cases.errors`` of a row result (ARRAYS' names, and ``dmu``) against the truth."""
        t = self.truth()[d][k]
        errs = ec.errors(res, t)
        if "dmu" in res:
            errs["dmu"] = abs(res["dmu"] - t["dmu"]) / t["dmu_scale"]
        return errs

    def numpy_oracle_errors(self, d, k):
        """The numpy oracle's own errors at the row (with the host chain rule, and d/dmu_k = sum_b t_b g_kb)."""
        res = ec.oracle_result(self.rows[d][k].case)
        res["dmu"] = float(np.dot(self.blens[d], res["grad_blens"]))
        return self.row_errors(d, k, res)

    def bounds(self):
        """Per row: the project's bars (``exact_cases.bars()``; d/dmu_k: 1e-9 of
        sum_b |t_b g_kb|), or on the rows with branches of 1e-4 or less
        ``exact_cases.short_branch_bounds``' rule: max(bar, 10 x the numpy
        oracle's own error at that row).  A draw's bound is the largest of
        its partitions'.  -> ([n][K] row bounds, [n] draw bounds)"""
        if self._bounds is None:
            rows, draws = [], []
            for d, row in enumerate(self.rows):
                br = []
                for r in row:
                    b = ec.bars()
                    b["dmu"] = ec.BAR_G
                    if r.short:
                        sb, _ = ec.short_branch_bounds(r.case, self.truth()[d][r.k])
                        b.update(sb)
                        b["dmu"] = max(b["dmu"], 10.0 * self.numpy_oracle_errors(d, r.k)["dmu"])
                    br.append(b)
                rows.append(br)
                draws.append({a: max(b[a] for b in br) for a in DRAW_ARRAYS})
            self._bounds = (rows, draws)
        return self._bounds

    # -------------------------------------------------------------- engines
    def engine(self, max_draws, device=0):
        return pt.PartitionedLikelihood(self.parts, self.peel0, self.rooted, self.model, self.C, max_draws=max_draws,
                                        device=device)

    def plan(self, max_draws, cu_count=256):
        return pt.plan_partitions([p[0] for p in self.parts], self.peel0, self.rooted, self.C, max_draws,
                                  model=self.model, cu_count=cu_count)

    def evaluators(self):
        from oracle import cpu
        kind = models.MODEL_IDS[self.model]

        def make(k):
            tip, w = self.parts[k]
            return lambda bl, mv, site_ll: cpu.evaluate(tip, w, self.peel0, self.rooted, kind, mv, bl, self.C,
                                                        site_ll=site_ll)
        return [make(k) for k in range(K)]

    def host(self):
        """``partition.partition_host`` over C-oracle evaluators."""
        return pt.partition_host(self.evaluators(), self.B, self.C, WIDTHS)


@functools.lru_cache(maxsize=None)
def edge_part(model, rooted, C_=C, tree=BALANCED):
    return EdgePart(model, rooted, C_, tree)


def check_call(e, out, rows, site, failures, what="", draws=None):
    """One call's results (``evaluate_rows(..., part_rows=True, site_ll=True)``
    on the draws ``draws`` of ``e``, all of them by default) against the truth
    at the bounds: every partition row with its site log-likelihoods, every
    d/dmu_k, and every draw row.  Failures are collected, not raised.
    -> ({(d, k): errors}, {d: errors})"""
    draws = list(range(e.n)) if draws is None else list(draws)
    brow, bdraw = e.bounds()
    B, C_ = e.B, e.C
    blk = 1 + 2 * C_ + 14
    assert out.shape == (len(draws), e.outlen) and rows.shape == (len(draws), K, e.rowlen)
    row_errs, draw_errs = {}, {}
    for i, d in enumerate(draws):
        for k in range(K):
            res = fx.row_dict(rows[i, k], B, C_, site[i, e.off[k]:e.off[k + 1]])
            res["dmu"] = float(out[i, 1 + B + k * blk])
            errs = e.row_errors(d, k, res)
            assert set(errs) == set(ROW_ARRAYS)
            for a, v in errs.items():
                if not v <= brow[d][k][a]:
                    failures.append("%s %s %s: %.3e > %.1e" % (what, e.rows[d][k].name, a, v, brow[d][k][a]))
            # the partition's block of the draw's row carries the row's own tail
            if not np.array_equal(out[i, 2 + B + k * blk:1 + B + (k + 1) * blk], rows[i, k, 1 + B:]):
                failures.append("%s %s: the draw's row does not carry the partition's tail" % (what, e.rows[d][k].name))
            row_errs[(d, k)] = errs
        t = e.draw_truth(d)
        errs = dict(loglik=abs(out[i, 0] - t["loglik"]) / abs(t["loglik"]),
                    grad_blens=ec.rel_err(out[i, 1:1 + B], t["grad_blens"]))
        for a, v in errs.items():
            if not v <= bdraw[d][a]:
                failures.append("%s draw %d (%s) %s: %.3e > %.1e" % (what, d, e.draw_kinds[d], a, v, bdraw[d][a]))
        draw_errs[d] = errs
    return row_errs, draw_errs


def worst(e, row_errs, draw_errs):
    """(error / bound, which row or draw, array) of the worst ratio of a call."""
    brow, bdraw = e.bounds()
    best = (0.0, "-", "-")
    for (d, k), errs in row_errs.items():
        for a, v in errs.items():
            if not v / brow[d][k][a] <= best[0]:  # a NaN wins
                best = (v / brow[d][k][a], e.rows[d][k].name, a)
    for d, errs in draw_errs.items():
        for a, v in errs.items():
            if not v / bdraw[d][a] <= best[0]:
                best = (v / bdraw[d][a], "draw %d (%s)" % (d, e.draw_kinds[d]), "draw " + a)
    return best


def largest(e, row_errs, kinds):
    """Per array, the largest error among the rows of the given kinds."""
    out = {}
    for (d, k), errs in row_errs.items():
        if e.rows[d][k].kind not in kinds:
            continue
        for a, v in errs.items():
            out[a] = v if a not in out or not v <= out[a] else out[a]
    return out
