"""The edge forests of the exact forest tests (tests/test_forest_exact_cpu.py
on the CPU, tests/test_forest_exact_gpu.py on the GPU): the parameter points
of tests/exact_cases.py -- spectral ties, near ties, ill-conditioned models,
extreme and zero site rates, short, zero and saturated branches -- put on two
fixed alignments and on four trees each, and the complex-step truth of every
row (oracle/complex_step.py, on the row's own peel), computed once per process.

Two alignments, because the model is a context's: the data of
``exact_cases._hky3()`` (HKY) and of ``exact_cases._gtr7()`` (GTR), both S = 12,
P = 130, C = 4.  The trees are ``forest_cases.forest_peels(12, rooted,
[301, 302])``: caterpillar, balanced and two random peels (both seeds satisfy
the unrooted last-row rule).  Branch b is the branch above node b, so one
``blens`` vector serves every peel; an unrooted forest takes its first 2S - 3
entries.
"""
import functools

import numpy as np

from phylostan_amd import models
from tests import cases
from tests import exact_cases as ec
from tests import forest_cases as fc

S, P, C = 12, 130, 4
SEEDS = (301, 302)
TREES = ("caterpillar", "balanced", "random301", "random302")

TIE, NEAR, GENERIC, OTHER = "tie", "near", "generic", "other"


def _params_of(name):
    """The parameter point of an edge-list entry (its data and tree are not used)."""
    return lambda: ec.CASES[name]()


def _rs0():
    c = ec._gtr7()
    c.rs = c.rs.copy()
    c.rs[0] = 0.0
    return c


def _long():
    c = ec._gtr7()
    c.blens[1::5] = 50.0
    return c


def _zero():
    # internal branches only: a zero tip branch between two different observed
    # states is an impossible site (truth -inf)
    c = ec._gtr7()
    c.blens[S::3] = 0.0
    return c


# model -> [(point, its kind, the maker of its parameters, the trees that carry it)]; every point on at least
# two different trees, every tree with a tie, a near tie (HKY: the GTR list has none) and a generic row
POINTS = {
    "HKY": [
        ("ctl_hky3", GENERIC, _params_of("ctl_hky3"), (0, 1, 2, 3)),
        ("tie2_hky3", TIE, _params_of("tie2_hky3"), (0, 2)),
        ("near_5e-13", NEAR, _params_of("near_5e-13"), (1, 3)),
        ("near_1e-11", NEAR, _params_of("near_1e-11"), (0, 2)),
        ("near_1e-9", NEAR, _params_of("near_1e-9"), (1, 3)),
        ("near_1e-7", NEAR, _params_of("near_1e-7"), (0, 1)),
        ("near_kappa1", NEAR, _params_of("near_kappa1"), (2, 3)),
        ("tie3_f81_hky7", TIE, _params_of("tie3_f81_hky7"), (1, 3)),
        ("cond_kappa1000", OTHER, _params_of("cond_kappa1000"), (0, 2)),
    ],
    "GTR": [
        ("ctl_gtr7", GENERIC, _params_of("ctl_gtr7"), (0, 1, 2, 3)),
        ("tie3_jc_as_gtr7", TIE, _params_of("tie3_jc_as_gtr7"), (0, 1, 2, 3)),
        ("cond_freq1e-6", OTHER, _params_of("cond_freq1e-6"), (0, 2)),
        ("cond_rates", OTHER, _params_of("cond_rates"), (1, 3)),
        ("rs_weibull005", OTHER, _params_of("rs_weibull005"), (0, 3)),
        ("rs0_gtr7", OTHER, _rs0, (1, 2)),
        ("short_1e-4", OTHER, _params_of("short_1e-4"), (0, 3)),
        ("short_1e-8", OTHER, _params_of("short_1e-8"), (1, 2)),
        ("long_50", OTHER, _long, (1, 3)),
        ("zero_internal", OTHER, _zero, (0, 1, 2, 3)),
    ],
}
# the C = 10 context (the 1,024-thread one-column form): HKY, four points on two trees
POINTS_C10 = [
    ("ctl_hky3", GENERIC, _params_of("ctl_hky3"), (0, 2)),
    ("tie2_hky3", TIE, _params_of("tie2_hky3"), (0, 2)),
    ("near_5e-13", NEAR, _params_of("near_5e-13"), (2, 0)),
    ("near_1e-9", NEAR, _params_of("near_1e-9"), (0, 2)),
]
C10_SHAPE = 0.5
SHORT = tuple(ec.SHORT)


class Row:
    def __init__(self, point, kind, tree, case):
        self.point, self.kind, self.tree, self.case = point, kind, tree, case

    @property
    def name(self):
        return "%s@%s" % (self.point, TREES[self.tree])


class EdgeForest:
    """One alignment, four peels and the edge rows: ``rows[k].case`` is the
    row's point as a ``cases.Case`` on its own peel (what the truth and the
    short-branch bounds are computed from)."""

    def __init__(self, model, rooted, C_, points):
        base = ec._hky3() if model == "HKY" else ec._gtr7()
        assert (base.S, base.P, base.model) == (S, P, model)
        self.model, self.rooted, self.C = model, rooted, C_
        self.tipcodes, self.weights = base.tipcodes, base.weights
        self.peels = fc.forest_peels(S, rooted, list(SEEDS))
        self.B = 2 * S - 2 if rooted else 2 * S - 3
        self.outlen = 1 + self.B + 2 * C_ + 14
        # round-robin over the points: consecutive rows are different points, mostly on different trees
        order = [(j, p) for j in range(4) for p in points if len(p[3]) > j]
        rows = []
        for j, (name, kind, make, trees) in order:
            c = make()
            rs, ps = (c.rs, c.ps) if C_ == c.C else models.weibull_site_rates(C10_SHAPE, C_)
            case = cases.Case("%s_%s" % (name, TREES[trees[j]]), self.tipcodes, self.weights, self.peels[trees[j]],
                              rooted, model, C_, c.blens[:self.B], c.freqs, c.rates, rs, ps)
            rows.append(Row(name, kind, trees[j], case))
        # the call opens generic / near tie / generic on three different trees where the points allow it
        near = next((r for r in rows if r.kind == NEAR and r.tree != rows[0].tree), None)
        after = near and next((r for r in rows[1:] if r.kind == GENERIC and r.tree not in (rows[0].tree, near.tree)),
                              None)
        if rows[0].kind == GENERIC and near and after:
            rows = [rows[0], near, after] + [r for r in rows[1:] if r is not near and r is not after]
        self.rows = rows
        self.tree_of_row = np.array([r.tree for r in self.rows], dtype=np.int32)
        self.blens = np.array([r.case.blens for r in self.rows])
        self.model_vecs = np.array([r.case.model_vec() for r in self.rows])
        self._check(points)
        self._truth = self._bounds = None

    def _check(self, points):
        for name, _, _, trees in points:
            assert len(set(trees)) >= 2, "%s sits on one tree only" % name
        used = sorted(set(int(t) for t in self.tree_of_row))
        kinds = {k for _, k, _, _ in points} & {TIE, NEAR, GENERIC}
        for t in used:
            have = {r.kind for r in self.rows if r.tree == t}
            assert kinds <= have, "tree %d lacks a %s row" % (t, sorted(kinds - have))
        # the leak case: a near-tie row whose neighbours in the call are generic rows on other trees
        if NEAR in kinds and len(used) >= 3:
            assert any(self.rows[k].kind == NEAR and self.rows[k - 1].kind == GENERIC and
                       self.rows[k + 1].kind == GENERIC and
                       len({self.rows[k - 1].tree, self.rows[k].tree, self.rows[k + 1].tree}) == 3
                       for k in range(1, len(self.rows) - 1)), "no near-tie row between generic rows on other trees"

    def truth(self):
        """The complex-step truth of every row (``exact_cases.truth_of`` on the
        row's own peel), all finite; computed once."""
        if self._truth is None:
            out = [ec.truth_of(r.case) for r in self.rows]
            for r, t in zip(self.rows, out):
                for k, v in t.items():
                    assert np.all(np.isfinite(v)), "the truth of %s has a non-finite %s" % (r.name, k)
            self._truth = out
        return self._truth

    def bounds(self):
        """Per row: ``exact_cases.bars()``, or for the two short-branch points
        ``exact_cases.short_branch_bounds`` at that row (max(bar, 10 x the
        numpy oracle's own error there)).  -> [(bounds, oracle errors or None)]"""
        if self._bounds is None:
            self._bounds = [ec.short_branch_bounds(r.case, t) if r.point in SHORT else (ec.bars(), None)
                            for r, t in zip(self.rows, self.truth())]
        return self._bounds

    def engine(self, max_rows):
        from phylostan_amd.forest import ForestLikelihood
        return ForestLikelihood(self.tipcodes, self.weights, self.peels, self.rooted, self.model, self.C,
                                max_rows=max_rows)

    def plan(self, max_rows, cu_count=256):
        from phylostan_amd.forest import plan_forest
        return plan_forest(self.tipcodes, self.peels, self.rooted, self.C, max_rows, self.model, cu_count)


@functools.lru_cache(maxsize=None)
def edge_forest(model, rooted, C_=C):
    if C_ == 10:
        assert model == "HKY"
        return EdgeForest(model, rooted, 10, POINTS_C10)
    return EdgeForest(model, rooted, C_, POINTS[model])


def row_dict(row, B, C_, site_ll=None):
    """A compact output row (include/phylo_hip.h: 1 + B + 2C + 4 + 6 + 4) and
    its site log-likelihoods as the dict ``exact_cases.errors`` takes."""
    row = np.asarray(row, dtype=np.float64)
    assert row.shape[0] >= 1 + B + 2 * C_ + 14
    o = 1 + B + 2 * C_
    out = dict(loglik=float(row[0]), grad_blens=row[1:1 + B], grad_rs=row[1 + B:1 + B + C_], grad_ps=row[1 + B + C_:o],
               grad_freq_root=row[o:o + 4], grad_rates=row[o + 4:o + 10], grad_freqs=row[o + 10:o + 14])
    if site_ll is not None:
        out["site_ll"] = np.asarray(site_ll, dtype=np.float64)
    return out


def check_rows(f, rows, site, failures, what=""):
    """Every row of ``f`` against its truth at its bounds; failures are
    collected per row and array.  -> the errors per row (``exact_cases.errors``)."""
    out = []
    for k, (r, t, (b, _)) in enumerate(zip(f.rows, f.truth(), f.bounds())):
        errs = ec.errors(row_dict(rows[k], f.B, f.C, site[k]), t)
        assert set(errs) == set(ec.ARRAYS)
        for a, v in errs.items():
            if not v <= b[a]:
                failures.append("%s row %d %s %s: %.3e > %.1e" % (what, k, r.name, a, v, b[a]))
        out.append(errs)
    return out


def worst(f, errs, kinds=None, points=None):
    """(error / bound, row name, array) of the worst ratio among the rows chosen."""
    best = (0.0, "-", "-")
    for e, row, (b, _) in zip(errs, f.rows, f.bounds()):
        if (kinds is not None and row.kind not in kinds) or (points is not None and row.point not in points):
            continue
        for a, v in e.items():
            if not v / b[a] <= best[0]:  # a NaN wins
                best = (v / b[a], row.name, a)
    return best


def largest(f, errs, kinds=None, points=None):
    """Per array, the largest error among the rows chosen (for ``exact_cases.fmt``)."""
    out = {}
    for e, row in zip(errs, f.rows):
        if (kinds is not None and row.kind not in kinds) or (points is not None and row.point not in points):
            continue
        for a, v in e.items():
            out[a] = v if a not in out or not v <= out[a] else out[a]
    return out
