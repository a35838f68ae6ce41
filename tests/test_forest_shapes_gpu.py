"""GPU: the forest engine at the shapes where a sweep goes wrong -- pattern
counts on the 64-column block edges, three- and four-taxon trees, the plans a
large forest takes by itself (a deep stack split between LDS and global
memory, chunk counts that differ per tree), and the clean refusal of a forest
that underflows -- every row against ``oracle.cpu.evaluate`` on its own peel at
the parity bars (``rows_vs_truth`` of tests/test_forest_gpu.py).  Every plan a
test is about is asserted from ``forest.plan_forest`` and the live context
before anything is evaluated.
"""
import functools
import os

import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

from phylostan_amd.forest import plan_forest
from tests import cases, exact_cases as ec, forest_cases as fc
from tests.test_forest_gpu import rows_vs_truth

pytestmark = pytest.mark.gpu

ROOTED = pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])


@pytest.fixture(autouse=True)
def no_phy_environment(monkeypatch):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)


def planned(f, max_rows, eng):
    """The planner's facts of the context, which are the live context's."""
    plan = plan_forest(f.tipcodes, f.peels, f.rooted, f.C, max_rows, f.model)
    info = eng.info()
    assert {k: plan[k] for k in info} == info, (plan, info)
    return plan


def permuted_and_alone(f, eng, rows, site):
    n = len(f.tree_of_row)
    perm = np.random.default_rng(5).permutation(n)
    r2, s2 = eng.evaluate_rows(f.tree_of_row[perm], f.blens[perm], f.model_vecs[perm], site_ll=True)
    np.testing.assert_array_equal(r2, rows[perm])
    np.testing.assert_array_equal(s2, site[perm])
    for k in range(n):
        r1, s1 = eng.evaluate_rows(f.tree_of_row[k:k + 1], f.blens[k:k + 1], f.model_vecs[k:k + 1], site_ll=True)
        np.testing.assert_array_equal(r1[0], rows[k])
        np.testing.assert_array_equal(s1[0], site[k])


# ---------------------------------------------------------------- block edges
@functools.lru_cache(maxsize=None)
def block_edge_forest(P, C, rooted):
    """``forest_cases.random_forest``'s data (ambiguity codes included) with
    taxon 5 all gaps and, past one column, the last column all 15 -- the
    column on the block edge."""
    base = fc.random_forest(3, 8, P, C, "GTR", rooted)
    tip = base.tipcodes.copy()
    tip[5, :] = 15
    if P > 1:
        tip[:, P - 1] = 15
    return fc.Forest(tip, base.weights, base.peels, rooted, "GTR", C, base.tree_of_row, base.blens, base.model_vecs)


@pytest.mark.parametrize("max_rows", [16, 600])
@ROOTED
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P", [1, 63, 64, 65, 128, 129])
def test_pattern_counts_on_the_block_edges(P, C, rooted, max_rows):
    f = block_edge_forest(P, C, rooted)
    assert sorted(set(f.tree_of_row)) == [0, 1, 2, 3]
    eng = f.engine(max_rows)
    planned(f, max_rows, eng)
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    eng.close()
    rows_vs_truth(rows, site, *f.truth(), what="P = %d" % P)
    if P > 1:
        assert np.all(np.abs(site[:, P - 1]) <= 1e-12)  # the all-15 column: L = 1


# -------------------------------------------------------------- minimal trees
@functools.lru_cache(maxsize=None)
def minimal_forest(S, P, rooted):
    """S = 3: one topology, so two identical peels and every point on both;
    S = 4: caterpillar, balanced and a random peel.  Unambiguous data: with it
    the S = 3 unrooted max_rows = 4 context leaves the chain rule out of the
    sweep by itself."""
    base = cases.random_case(10 * S + P, S=S, P=P, C=3, model="GTR", ambiguous=0.0)
    rng = np.random.default_rng(S + P)
    if S == 3:
        one = fc.forest_peels(3, rooted, [], shapes=True)[0]
        peels, tree = np.array([one, one]), (0, 1, 0, 1)
        bl, mv = fc.random_rows(rng, 2, 4 if rooted else 3, 3, "GTR")
        bl, mv = bl[[0, 0, 1, 1]], mv[[0, 0, 1, 1]]
    else:
        peels, tree = fc.forest_peels(4, rooted, [7]), (2, 0, 1, 2)
        bl, mv = fc.random_rows(rng, 4, 6 if rooted else 5, 3, "GTR")
    return fc.Forest(base.tipcodes, base.weights, peels, rooted, "GTR", 3, tree, bl, mv)


@functools.lru_cache(maxsize=None)
def minimal_truth(S, P, rooted):
    f = minimal_forest(S, P, rooted)
    out = []
    for t, bl, mv in zip(f.tree_of_row, f.blens, f.model_vecs):
        out.append(ec.truth_of(cases.Case("min", f.tipcodes, f.weights, f.peels[t], rooted, "GTR", 3, bl, mv[:4],
                                          mv[4:10], mv[10:13], mv[13:16])))
    return out


@pytest.mark.parametrize("max_rows", [4, 600])
@pytest.mark.parametrize("P", [1, 65])
@ROOTED
@pytest.mark.parametrize("S", [3, 4])
def test_three_and_four_taxon_trees(S, rooted, P, max_rows):
    from tests import forest_exact_cases as fx
    f = minimal_forest(S, P, rooted)
    assert f.peels.shape[0] == (2 if S == 3 else 3)
    eng = f.engine(max_rows)
    plan = planned(f, max_rows, eng)
    if S == 3 and not rooted and max_rows == 4:
        # qgrad_kernel after the sweep's own finalize, with no knob set
        assert (plan["fin"], plan["qf"], plan["fin_qf"]) == (1, 0, 0), plan
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    eng.close()
    rows_vs_truth(rows, site, *f.truth(), what="S = %d" % S)
    failures = []
    for k, t in enumerate(minimal_truth(S, P, rooted)):
        for a, v in ec.errors(fx.row_dict(rows[k], f.B, 3, site[k]), t).items():
            if not v <= ec.bars()[a]:
                failures.append("row %d %s: %.3e > %.1e" % (k, a, v, ec.bars()[a]))
    assert not failures, failures
    if S == 3:  # the same point on two identical peels
        for a, b in ((0, 1), (2, 3)):
            np.testing.assert_array_equal(rows[a], rows[b])
            np.testing.assert_array_equal(site[a], site[b])


# ------------------------------------------------------------ large, no knob
LARGE_S = 180  # at 200 taxa three of the four contexts give every tree the same chunk count at max_rows = 8


def large_forest(C, model, rooted):
    return fc.random_forest(5, LARGE_S, 70, C, model, rooted, tree_of_row=(3, 0, 1, 2, 0, 3))


@pytest.mark.parametrize("max_rows", [600, 8])
@ROOTED
@pytest.mark.parametrize("C,model", [(2, "GTR"), (4, "HKY")])
def test_large_forest_plans_taken_without_a_knob(C, model, rooted, max_rows):
    f = large_forest(C, model, rooted)
    eng = f.engine(max_rows)
    plan = planned(f, max_rows, eng)
    if max_rows == 600:
        # the deep stack split between LDS and global memory: the caterpillar has none, the random trees
        # sit on both sides of the boundary or straddle it
        assert plan["cols"] == 2 and 0 < plan["deep_in_lds"] < plan["max_depth"] and plan["min_depth"] == 0, plan
        assert any(d > plan["deep_in_lds"] for d in plan["depths"]), plan
    else:
        assert plan["cols"] == 1 and plan["latency"] == 1, plan
        assert plan["min_chunks"] != plan["max_chunks"] and plan["min_chunks"] >= 2, plan
    truth_rows, truth_site = f.truth()
    assert np.all(np.isfinite(truth_site)) and truth_site.min() > -700.0  # nothing underflows
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    rows_vs_truth(rows, site, truth_rows, truth_site, what="S = %d max_rows = %d" % (LARGE_S, max_rows))
    permuted_and_alone(f, eng, rows, site)
    eng.close()


# ------------------------------------------------------------------ underflow
def test_a_forest_that_underflows_is_refused_cleanly():
    """700 taxa without rescaling (the forest is unrescaled by design, DESIGN.md
    5g): every row is -inf with a zero gradient and site_ll holds no NaN, on
    every call -- what test_without_rescaling_the_same_tree_is_minus_inf pins
    for the single-tree engine."""
    S = 700
    base = cases.random_case(913, S=S, P=70, C=1, model="JC69", rooted=False)
    peels = fc.forest_peels(S, False, [913])
    assert peels.shape[0] == 3
    tree = (0, 1, 2, 1)
    bl, mv = fc.random_rows(np.random.default_rng(913), 4, 2 * S - 3, 1, "JC69")
    f = fc.Forest(base.tipcodes, base.weights, peels, False, "JC69", 1, tree, bl, mv)
    eng = f.engine(4)
    plan = planned(f, 4, eng)
    assert plan["max_chunks"] >= 2 and (plan["fin"], plan["fin_qf"]) == (0, 1), plan
    for _ in range(2):
        rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
        assert np.all(rows[:, 0] == -np.inf) and not rows[:, 1:].any()
        assert not np.isnan(site).any()
    eng.close()
