"""CPU: the forest's references against the complex-step truth on the edge
forests of tests/forest_exact_cases.py, and the plan facts the GPU tests of
tests/test_forest_exact_gpu.py and tests/test_forest_shapes_gpu.py name their
forms by.

* the C oracle (``oracle.cpu.evaluate`` on the row's peel) stays inside the
  project's bars on every row -- so a device row outside them is the device's;
* ``forest.forest_host`` over oracle evaluators: one mixed call is the
  row-by-row results bit for bit;
* ``forest.plan_forest`` gives the epilogue placement and kernel form of every
  context the GPU files run (256 CUs), without a device.
"""
import os

import numpy as np
import pytest

from phylostan_amd import forest as fr, models
from tests import forest_exact_cases as fx, report
from tests.test_plan_host import needs_lib

FORESTS = [(m, r) for m in ("HKY", "GTR") for r in (True, False)]
IDS = ["%s-%s" % (m, "rooted" if r else "unrooted") for m, r in FORESTS]


def oracle_rows(f):
    from oracle import cpu
    rows, site = [], []
    for t, bl, mv in zip(f.tree_of_row, f.blens, f.model_vecs):
        out, sl = cpu.evaluate(f.tipcodes, f.weights, f.peels[t], f.rooted, models.MODEL_IDS[f.model], mv, bl, f.C,
                               site_ll=True)
        rows.append(out[:f.outlen])
        site.append(sl)
    return np.array(rows), np.array(site)


def test_the_edge_forests_hold_the_listed_points():
    for model, rooted in FORESTS:
        f = fx.edge_forest(model, rooted)
        assert (f.tipcodes.shape, f.C, f.peels.shape) == ((12, 130), 4, (4, 11, 3))
        assert f.blens.shape[1] == (22 if rooted else 21)
        assert sorted(set(f.tree_of_row)) == [0, 1, 2, 3]
        if not rooted:
            assert np.all(f.peels[:, -1, 1] == 2 * 12 - 3)
    hky = {r.point for r in fx.edge_forest("HKY", True).rows}
    gtr = {r.point: r for r in fx.edge_forest("GTR", True).rows}
    assert hky == {"ctl_hky3", "tie2_hky3", "near_5e-13", "near_1e-11", "near_1e-9", "near_1e-7", "near_kappa1",
                   "tie3_f81_hky7", "cond_kappa1000"}
    assert set(gtr) == {"ctl_gtr7", "tie3_jc_as_gtr7", "cond_freq1e-6", "cond_rates", "rs_weibull005", "rs0_gtr7",
                        "short_1e-4", "short_1e-8", "long_50", "zero_internal"}
    assert gtr["rs0_gtr7"].case.rs[0] == 0.0 and np.all(gtr["rs0_gtr7"].case.rs[1:] > 0)
    assert np.all(gtr["long_50"].case.blens[1::5] == 50.0)
    z = gtr["zero_internal"].case.blens
    assert np.all(z[:12] > 0) and np.all(z[12::3] == 0.0)
    for name, t in (("short_1e-4", 1e-4), ("short_1e-8", 1e-8)):
        assert np.all(gtr[name].case.blens[::3] == t)
    c10 = fx.edge_forest("HKY", False, 10)
    assert c10.C == 10 and {r.point for r in c10.rows} == {"ctl_hky3", "tie2_hky3", "near_5e-13", "near_1e-9"}
    assert sorted(set(c10.tree_of_row)) == [0, 2] and c10.model_vecs.shape[1] == 30


@pytest.mark.parametrize("model,rooted", FORESTS, ids=IDS)
def test_c_oracle_against_the_truth(model, rooted):
    f = fx.edge_forest(model, rooted)
    rows, site = oracle_rows(f)
    failures = []
    errs = fx.check_rows(f, rows, site, failures, what="oracle")
    report.record("forest-exact[oracle  %s] worst error/bar %.2g (%s %s); ties and near ties %.2g"
                  % ("%s-%s" % (model, "rooted" if rooted else "unrooted"), *fx.worst(f, errs),
                     fx.worst(f, errs, kinds=(fx.TIE, fx.NEAR))[0]))
    assert not failures, failures


def test_c_oracle_against_the_truth_at_ten_categories():
    f = fx.edge_forest("HKY", True, 10)
    rows, site = oracle_rows(f)
    failures = []
    fx.check_rows(f, rows, site, failures, what="oracle C = 10")
    assert not failures, failures


@pytest.mark.parametrize("model,rooted", FORESTS, ids=IDS)
def test_host_stand_in_mixed_call_equals_its_rows(model, rooted):
    from oracle import cpu
    f = fx.edge_forest(model, rooted)
    kind = models.MODEL_IDS[model]

    def evaluator(t):
        return lambda bl, mv, site_ll: cpu.evaluate(f.tipcodes, f.weights, f.peels[t], rooted, kind, mv, bl, f.C,
                                                    site_ll=site_ll)
    host = fr.forest_host([evaluator(t) for t in range(4)], f.B, f.C, 130)
    rows, site = host.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    want_rows, want_site = oracle_rows(f)
    np.testing.assert_array_equal(rows, want_rows)
    np.testing.assert_array_equal(site, want_site)
    for k in range(len(f.rows)):
        r1, s1 = host.evaluate_rows(f.tree_of_row[k:k + 1], f.blens[k:k + 1], f.model_vecs[k:k + 1], site_ll=True)
        np.testing.assert_array_equal(r1[0], rows[k])
        np.testing.assert_array_equal(s1[0], site[k])
    perm = np.random.default_rng(5).permutation(len(f.rows))
    np.testing.assert_array_equal(host.evaluate_rows(f.tree_of_row[perm], f.blens[perm], f.model_vecs[perm]),
                                  rows[perm])


# ------------------------------------------------------------------ the plans
# form -> (environment, max_rows, C, the plan facts at 256 CUs).  The chain
# rule of the Q parameters runs: fin 1 qf 1 in the sweep; fin_qf 1 in
# finalize_kernel; fin 0 qf 0 fin_qf 0 in qgrad_kernel after finalize_kernel;
# fin 1 qf 0 in qgrad_kernel after the sweep's own finalize.
FORMS = {
    "cols2": ({}, 600, 4, dict(cols=2, fin=1, qf=1, fin_qf=0)),
    "cols1-latency": ({}, 16, 4, dict(cols=1, latency=1, fin=1, qf=1, fin_qf=0)),
    "fin0": ({"PHY_FIN": "0"}, 600, 4, dict(cols=2, fin=0, qf=0, fin_qf=1)),
    "qgrad-after-finalize": ({"PHY_FIN": "0", "PHY_QFUSE": "0"}, 600, 4, dict(cols=2, fin=0, qf=0, fin_qf=0)),
    "qgrad-after-sweep": ({"PHY_QFUSE": "0"}, 600, 4, dict(cols=2, fin=1, qf=0, fin_qf=0)),
    "C10": ({}, 600, 10, dict(cols=1, latency=0, fin=1, qf=1, fin_qf=0)),
}


def set_form(form, monkeypatch):
    """The form's environment and nothing else of PHY_*.  -> (max_rows, C, facts)"""
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    env, max_rows, C, facts = FORMS[form]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return max_rows, C, facts


def assert_form(f, form, max_rows, facts, info=None):
    """The planner's facts of the context are the form's (and the live context's, if given)."""
    plan = f.plan(max_rows)
    assert {k: plan[k] for k in facts} == facts, (form, plan)
    if info is not None:
        assert {k: plan[k] for k in info} == info, (form, plan, info)
    return plan


@needs_lib
@pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])
@pytest.mark.parametrize("form", sorted(FORMS))
def test_plan_table(form, rooted, monkeypatch):
    max_rows, C, facts = set_form(form, monkeypatch)
    for model in ("HKY",) if C == 10 else ("HKY", "GTR"):
        plan = assert_form(fx.edge_forest(model, rooted, C), form, max_rows, facts)
        if form == "C10":
            assert_form(fx.edge_forest(model, rooted, C), form, 16, facts)  # the same form at either size
        if C == 4:  # S = 12, P = 130: three 64-column blocks walked in turn at K = 1, two blocks at K = 2
            assert plan["min_depth"] == 0 and plan["max_depth"] >= 1


@needs_lib
def test_plan_qgrad_after_sweep_without_a_knob(monkeypatch):
    """S = 3 unrooted, C = 3, max_rows = 4: fin 1, qf 0 with no environment --
    the form of ``PHY_QFUSE=0`` alone, reached by the planner itself.  The
    data holds no ambiguity code: each one adds to the plan's LDS, and with
    enough of it the chain rule fits into the sweep again."""
    from tests import forest_cases as fc
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    for P in (1, 65):
        tip = np.random.default_rng(P).choice([1, 2, 4, 8], size=(3, P)).astype(np.uint8)
        plan = fr.plan_forest(tip, fc.forest_peels(3, False, []), False, 3, 4, "GTR", 256)
        assert (plan["fin"], plan["qf"], plan["fin_qf"]) == (1, 0, 0), plan
