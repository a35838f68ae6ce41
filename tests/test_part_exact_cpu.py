"""CPU: the partitioned engine's references against the complex-step truth on
the edge draws of tests/part_exact_cases.py, and the plan facts the GPU tests
of tests/test_part_exact_gpu.py name their forms by.

* ``partition.partition_host`` over C-oracle evaluators stays inside the
  bounds on every partition row, every draw row and every d/dmu_k -- so a
  device row outside them is the device's.  The bounds are the project's bars
  except on the rows with branches of 1e-4 or less (the two short draws and the
  mu = 1e-4 partition), which take ``exact_cases.short_branch_bounds``' rule.
  On every other row -- the one-column partition's among them -- the numpy
  oracle itself is inside the plain bars (asserted below), so no further row
  takes the measured rule;
* the host stand-in's mixed call is its one-draw calls bit for bit;
* ``partition.plan_partitions`` gives the kernel form and the epilogue
  placement of every context the GPU file runs (256 CUs), without a device,
  and the forms together reach all six kernels of ``row_kernel_for<false, true>``.
"""
import os

import numpy as np
import pytest

from tests import exact_cases as ec, part_exact_cases as px, report
from tests.test_plan_host import needs_lib

CONTEXTS = [(m, r) for m in ("HKY", "GTR") for r in (True, False)]
IDS = ["%s-%s" % (m, "rooted" if r else "unrooted") for m, r in CONTEXTS]

HKY_POINTS = {"ctl_hky3", "tie2_hky3", "near_5e-13", "near_1e-11", "near_1e-9", "near_1e-7", "near_kappa1",
              "tie3_f81_hky7", "cond_kappa1000"}
GTR_POINTS = {"ctl_gtr7", "tie3_jc_as_gtr7", "cond_freq1e-6", "cond_rates", "rs_weibull005", "rs0_gtr7"}


def test_the_edge_draws_hold_the_listed_points():
    for model, rooted in CONTEXTS:
        e = px.edge_part(model, rooted)
        B = 22 if rooted else 21
        assert [p[0].shape for p in e.parts] == [(12, 64), (12, 65), (12, 1)] and e.C == 4
        assert (e.blens.shape, e.mu.shape, e.model_vecs.shape) == ((9, B), (9, 3), (9, 3, 18))
        assert e.peel0.shape == (11, 3) and e.tree == px.BALANCED
        if not rooted:
            assert e.peel0[-1, 1] == 2 * 12 - 3
        where = {}
        for r in e.flat_rows():
            where.setdefault(r.point, set()).add(r.k)
        assert set(where) == (HKY_POINTS if model == "HKY" else GTR_POINTS)
        for point, ks in where.items():  # on two partitions at least, the one-column one among them
            assert len(ks) >= 2 and 2 in ks, (point, ks)
        kinds = dict(zip(e.draw_kinds, range(e.n)))
        for d in (kinds["mu_extreme"], kinds["mu_one"]):
            assert np.all(e.mu[d] == (px.MU_EXTREME if d == kinds["mu_extreme"] else 1.0))
        generic = [d for d in range(e.n) if e.draw_kinds[d] not in ("mu_extreme", "mu_one")]
        assert np.all((e.mu[generic] >= 0.3) & (e.mu[generic] <= 2.5))
        plain_t = [d for d in range(e.n) if e.draw_kinds[d] in ("generic", "mu_extreme", "mu_one")]
        assert np.all((e.blens[plain_t] >= 0.01) & (e.blens[plain_t] <= 0.3))
        assert [(d, r.k) for d in range(e.n) for r in e.rows[d] if r.short] == \
            [(d, k) for d in range(e.n) for k in range(3)
             if e.draw_kinds[d] in px.SHORT_T or (e.draw_kinds[d] == "mu_extreme" and k == 0)]
        for row in e.rows:  # a row's case sits at the rounded product mu_k t
            for r in row:
                np.testing.assert_array_equal(r.case.blens, e.mu[r.d, r.k] * e.blens[r.d])
                assert np.all(r.case.blens[:12] > 0)  # never a zero tip branch
                if r.short:  # the draw's own t, or the row's mu_k t
                    assert min(e.blens[r.d].min(), r.case.blens.min()) <= 1e-4
        if model == "HKY":
            assert [r.kind for r in e.rows[0]] == [px.GENERIC, px.NEAR, px.TIE]
            assert sorted(e.draw_kinds) == sorted(["generic"] * 7 + ["mu_extreme", "mu_one"])
        else:
            assert sorted(e.draw_kinds) == sorted(["generic"] * 3 + ["short_1e-4", "short_1e-8", "long_50",
                                                                    "zero_internal", "mu_extreme", "mu_one"])
            for name, t in px.SHORT_T.items():
                assert np.all(e.blens[kinds[name], ::3] == t)
            assert np.all(e.blens[kinds["long_50"], 1::5] == 50.0)
            z = e.blens[kinds["zero_internal"]]
            assert np.all(z[:12] > 0) and np.all(z[12::3] == 0.0)
            rs0 = [r for r in e.flat_rows() if r.point == "rs0_gtr7"]
            assert all(r.case.rs[0] == 0.0 and np.all(r.case.rs[1:] > 0) for r in rs0)
    for tree, name in ((0, "caterpillar"), (2, "random301")):
        assert px.TREES[tree] == name
    cat = px.edge_part("HKY", True, 4, px.CATERPILLAR)
    assert np.all(cat.peel0[1:, 0] == cat.peel0[:-1, 2])  # a chain: every internal node joins the last one and a tip
    np.testing.assert_array_equal(cat.blens, px.edge_part("HKY", True).blens)
    c10 = px.edge_part("HKY", False, 10)
    assert c10.C == 10 and c10.n == 2 and c10.model_vecs.shape == (2, 3, 30)
    assert {r.point for r in c10.flat_rows()} == {"ctl_hky3", "tie2_hky3", "near_5e-13", "near_1e-9"}
    assert [r.kind for r in c10.rows[0]] == [px.GENERIC, px.NEAR, px.TIE]


def oracle_against_the_truth(e, what):
    out, rows, site = e.host().evaluate_rows(e.blens, e.mu, e.model_vecs, part_rows=True, site_ll=True)
    failures = []
    row_errs, draw_errs = px.check_call(e, out, rows, site, failures, what="oracle " + what)
    # the rows outside the short-branch rule: the numpy oracle itself is inside the plain bars there
    plain = dict(ec.bars(), dmu=ec.BAR_G)
    for r in e.flat_rows():
        if r.short:
            continue
        for a, v in e.numpy_oracle_errors(r.d, r.k).items():
            if not v <= plain[a]:
                failures.append("numpy oracle %s %s %s: %.3e > %.1e" % (what, r.name, a, v, plain[a]))
    return row_errs, draw_errs, failures


@pytest.mark.parametrize("model,rooted", CONTEXTS, ids=IDS)
def test_c_oracle_against_the_truth(model, rooted):
    e = px.edge_part(model, rooted)
    tag = "%s-%s" % (model, "rooted" if rooted else "unrooted")
    row_errs, draw_errs, failures = oracle_against_the_truth(e, tag)
    report.record("part-exact[oracle  %s] worst error/bound %.2g (%s %s); ties and near ties, any array %.1e"
                  % (tag, *px.worst(e, row_errs, draw_errs),
                     max(px.largest(e, row_errs, (px.TIE, px.NEAR)).values())))
    assert not failures, failures


@pytest.mark.parametrize("model,rooted,C,tree", [("HKY", True, 10, px.BALANCED), ("HKY", False, 10, px.BALANCED),
                                                 ("HKY", True, 4, px.CATERPILLAR), ("GTR", True, 4, px.CATERPILLAR)],
                         ids=["C10-rooted", "C10-unrooted", "caterpillar-HKY", "caterpillar-GTR"])
def test_c_oracle_against_the_truth_of_the_other_contexts(model, rooted, C, tree):
    """Ten categories, and the caterpillar the no-deep-entries form evaluates on."""
    _, _, failures = oracle_against_the_truth(px.edge_part(model, rooted, C, tree), "C = %d %s" % (C, px.TREES[tree]))
    assert not failures, failures


@pytest.mark.parametrize("model,rooted", CONTEXTS, ids=IDS)
def test_host_stand_in_mixed_call_equals_its_draws(model, rooted):
    e = px.edge_part(model, rooted)
    host = e.host()
    out, rows, site = host.evaluate_rows(e.blens, e.mu, e.model_vecs, part_rows=True, site_ll=True)
    for d in range(e.n):
        o1, r1, s1 = host.evaluate_rows(e.blens[d:d + 1], e.mu[d:d + 1], e.model_vecs[d:d + 1], part_rows=True,
                                        site_ll=True)
        np.testing.assert_array_equal(o1[0], out[d])
        np.testing.assert_array_equal(r1[0], rows[d])
        np.testing.assert_array_equal(s1[0], site[d])
    perm = np.random.default_rng(5).permutation(e.n)
    np.testing.assert_array_equal(host.evaluate_rows(e.blens[perm], e.mu[perm], e.model_vecs[perm]), out[perm])


# ------------------------------------------------------------------ the plans
# form -> (environment, max_draws, C, tree, the plan facts at 256 CUs beyond DEFAULT_FACTS).  The kernel a plan
# launches is row_kernel_for<false, true>(cols, latency, deep_all_in_lds): <512, 2, DL>, the 512-thread one-column latency form
# <512, 1, DL>, or <1024, 1, DL>.  The chain rule of the Q parameters runs: fin 1 qf 1 in the sweep; fin_qf 1 in
# finalize_kernel; fin 0 qf 0 fin_qf 0 in qgrad_kernel after finalize_kernel; fin 1 qf 0 in qgrad_kernel after the
# sweep's own finalize.
DEFAULT_FACTS = dict(fin=1, qf=1, fin_qf=0, chunks=1)
COLS2 = dict(cols=2, latency=0, deep_in_lds=2, deep_all_in_lds=1, chunks=1)
BLOCKS1 = [[0, 1], [2, 4], [4, 5]]  # one column per lane: the 65-column partition walks two blocks
BLOCKS2 = [[0, 1], [1, 2], [2, 3]]
B_, C_ = px.BALANCED, px.CATERPILLAR
FORMS = {
    "cols2": ({}, 600, 4, B_, dict(COLS2, blocks=BLOCKS2)),
    "cols2-deep-global": ({"PHY_DEEP": "2"}, 600, 4, B_, dict(cols=2, latency=0, deep_in_lds=0, deep_all_in_lds=0)),
    "no-deep-entries": ({}, 600, 4, C_, dict(cols=2, latency=0, deep_in_lds=0, deep_all_in_lds=0)),
    "cols1-latency": ({}, 9, 4, B_, dict(cols=1, latency=1, deep_all_in_lds=1, blocks=BLOCKS1)),
    "cols1-latency-deep-global": ({"PHY_DEEP": "2"}, 9, 4, B_, dict(cols=1, latency=1, deep_all_in_lds=0)),
    "C10": ({}, 600, 10, B_, dict(cols=1, latency=0, deep_all_in_lds=1)),
    "C10-deep-global": ({"PHY_DEEP": "2"}, 600, 10, B_, dict(cols=1, latency=0, deep_all_in_lds=0)),
    # one deep entry in LDS and one in global memory
    "cols1-split-stack": ({"PHY_COLS": "1"}, 600, 4, B_, dict(cols=1, latency=0, deep_in_lds=1, deep_all_in_lds=0)),
    # the matrix records staged in three chunks while a row walks its partition's blocks only
    "lds16k": ({"PHY_LDS_BUDGET": "16384"}, 600, 4, B_, dict(cols=2, chunks=3, cap_m=9)),
    "lds16k-latency": ({"PHY_LDS_BUDGET": "16384"}, 9, 4, B_, dict(cols=1, latency=1)),
    "norecompute": ({"PHY_RECOMPUTE": "0"}, 600, 4, B_, dict(COLS2)),
    "fin0": ({"PHY_FIN": "0"}, 600, 4, B_, dict(cols=2, fin=0, qf=0, fin_qf=1)),
    "qgrad-after-finalize": ({"PHY_FIN": "0", "PHY_QFUSE": "0"}, 600, 4, B_, dict(cols=2, fin=0, qf=0, fin_qf=0)),
    "qgrad-after-sweep": ({"PHY_QFUSE": "0"}, 600, 4, B_, dict(cols=2, fin=1, qf=0, fin_qf=0)),
}
del B_, C_
# (cols, latency, deep_all_in_lds) of the six kernels of row_kernel_for<false, true> (row_engine.inc)
KERNELS = {(2, 0, 1): "<512,2,true>", (2, 0, 0): "<512,2,false>", (1, 1, 1): "<512,1,true>",
           (1, 1, 0): "<512,1,false>", (1, 0, 1): "<1024,1,true>", (1, 0, 0): "<1024,1,false>"}
KERNEL_OF = {
    "cols2": (2, 0, 1), "cols2-deep-global": (2, 0, 0), "no-deep-entries": (2, 0, 0), "cols1-latency": (1, 1, 1),
    "cols1-latency-deep-global": (1, 1, 0), "C10": (1, 0, 1), "C10-deep-global": (1, 0, 0),
    "cols1-split-stack": (1, 0, 0), "lds16k": (2, 0, 0), "lds16k-latency": (1, 1, 0), "norecompute": (2, 0, 1),
    "fin0": (2, 0, 1), "qgrad-after-finalize": (2, 0, 1), "qgrad-after-sweep": (2, 0, 1),
}


def models_of(form):
    return ("HKY",) if FORMS[form][2] == 10 else ("HKY", "GTR")


def set_form(form, monkeypatch):
    """The form's environment and nothing else of PHY_*.  -> (max_draws, C, tree, facts)"""
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    env, max_draws, C, tree, facts = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    facts = dict(DEFAULT_FACTS, **facts)
    if form == "lds16k-latency":  # at least two chunks (assert_form): three rooted, two unrooted
        del facts["chunks"]
    return max_draws, C, tree, facts


def assert_form(e, form, max_draws, facts, info=None):
    """The planner's facts of the context are the form's (and the live context's, if given)."""
    plan = e.plan(max_draws)
    assert {k: plan[k] for k in facts} == facts, (form, plan)
    kernel = (plan["cols"], plan["latency"], plan["deep_all_in_lds"])
    assert kernel == KERNEL_OF[form], (form, KERNELS[kernel], KERNELS[KERNEL_OF[form]])
    if form == "lds16k":
        assert plan["chunks"] == 3 and plan["lds_bytes"] <= 16384, plan
    if form == "lds16k-latency":
        assert plan["chunks"] >= 2 and plan["lds_bytes"] <= 16384, plan
    if info is not None:
        assert {k: plan[k] for k in info} == info, (form, plan, info)
    return plan


def test_the_forms_cover_the_six_kernels():
    assert set(KERNEL_OF) == set(FORMS)
    assert set(KERNEL_OF.values()) == set(KERNELS) and len(KERNELS) == 6


@needs_lib
@pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_plan_table(form, rooted, monkeypatch):
    max_draws, C, tree, facts = set_form(form, monkeypatch)
    for model in models_of(form):
        e = px.edge_part(model, rooted, C, tree)
        plan = assert_form(e, form, max_draws, facts)
        assert plan["blocks"] == (BLOCKS2 if plan["cols"] == 2 else BLOCKS1)
        assert plan["P"] == 257 and plan["R"] == 9  # 64 | 64 padding | 65 | 63 padding | 1; the four states + 5 codes


@needs_lib
def test_the_planned_kernels_cover_all_six(monkeypatch):
    """The (cols, latency, deep_all_in_lds) triples the planner itself returns for the forms, not the table's."""
    seen = {}
    for form in sorted(FORMS):
        max_draws, C, tree, _ = set_form(form, monkeypatch)
        plan = px.edge_part("HKY", True, C, tree).plan(max_draws)
        seen.setdefault((plan["cols"], plan["latency"], plan["deep_all_in_lds"]), []).append(form)
    assert set(seen) == set(KERNELS), seen
