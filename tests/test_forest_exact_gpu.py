"""GPU: the forest engine against the complex-step reference (oracle/
complex_step.py) -- not against the C oracle, which runs the device's Jacobi
eigensolver and divided-difference tie rule operation for operation -- on the
edge forests of tests/forest_exact_cases.py: spectral ties, near ties,
ill-conditioned models, extreme and zero site rates, short, zero and saturated
branches, each point on at least two of four trees, all rows of a forest in
ONE mixed call.

The forest launches only the six ``sweep_kernel<., ., ., false, false, true>``
instantiations, one workgroup per row, and places the finalize and the
Q-parameter chain rule (``qgrad_body``, which holds the tie marks and the near
window) in one of four ways; every form below is named by its
``forest.plan_forest`` facts before it evaluates (the table of
tests/test_forest_exact_cpu.py):

  cols2                 K = 2, the chain rule inside the sweep
  cols1-latency         K = 1 latency form (three blocks walked in turn), the same epilogue
  fin0                  PHY_FIN=0: the chain rule in finalize_kernel
  qgrad-after-finalize  PHY_FIN=0 PHY_QFUSE=0: qgrad_kernel after finalize_kernel
  qgrad-after-sweep     PHY_QFUSE=0: qgrad_kernel after the sweep's own finalize
  C10                   ten categories: the 1,024-thread K = 1 form (HKY, its own truth)

Bars as tests/test_gpu_exact_gradients.py: log L and site_ll 1e-10, gradients
1e-9, Q-parameter gradients 1e-8 of each array's largest entry; the two
short-branch points at max(bar, 10 x the numpy oracle's own error at that row).
"""
import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

from tests import exact_cases as ec, forest_exact_cases as fx, report
from tests.test_forest_exact_cpu import FORMS, assert_form, set_form
from tests.test_gpu_parity import RTOL_G, RTOL_LL

pytestmark = pytest.mark.gpu

assert (ec.BAR_LL, ec.BAR_G) == (RTOL_LL, RTOL_G)

CONTEXTS = [(form, model, rooted) for form in FORMS for model in ("HKY", "GTR") for rooted in (True, False)
            if form != "C10" or model == "HKY"]


def _ctx_id(c):
    return "%s-%s-%s" % (c[0], c[1], "rooted" if c[2] else "unrooted")


def make_engine(form, model, rooted, monkeypatch):
    """A forest context that runs ``form``, with the evidence that it does."""
    max_rows, C, facts = set_form(form, monkeypatch)
    f = fx.edge_forest(model, rooted, C)
    eng = f.engine(max_rows)
    assert_form(f, form, max_rows, facts, info=eng.info())
    return f, eng


@pytest.mark.parametrize("ctx", CONTEXTS, ids=_ctx_id)
def test_edge_rows_in_one_mixed_call(ctx, monkeypatch):
    form, model, rooted = ctx
    f, eng = make_engine(form, model, rooted, monkeypatch)
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    eng.close()
    failures = []
    errs = fx.check_rows(f, rows, site, failures, what=form)
    tag = "forest-exact[%-20s %s %s]" % (form, model, "rooted  " if rooted else "unrooted")
    line = "%s worst error/bar %.2g (%s %s)" % (tag, *fx.worst(f, errs))
    if model == "HKY":
        near = fx.largest(f, errs, kinds=(fx.NEAR,))
        line += "; near ties: drates %.1e dfreqs %.1e, any array %.1e" % (near["grad_rates"], near["grad_freqs"],
                                                                          max(near.values()))
    else:
        for name in fx.SHORT:
            line += "; %s: %.1e (error/bound %.2g)" % (name, max(fx.largest(f, errs, points=(name,)).values()),
                                                       fx.worst(f, errs, points=(name,))[0])
    report.record(line)
    assert not failures, failures


@pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])
@pytest.mark.parametrize("model", ["HKY", "GTR"])
@pytest.mark.parametrize("form", ["cols2", "cols1-latency"])
def test_edge_rows_are_their_own(form, model, rooted, monkeypatch):
    """The tie marks and the near window are a row's own: the mixed call's
    rows (a near-tie row between generic rows on other trees among them) are,
    bit for bit, the rows of one-row calls and of a permuted call."""
    f, eng = make_engine(form, model, rooted, monkeypatch)
    if model == "HKY":
        assert (f.rows[0].kind, f.rows[1].kind, f.rows[2].kind) == (fx.GENERIC, fx.NEAR, fx.GENERIC)
        assert len({r.tree for r in f.rows[:3]}) == 3
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    n = len(f.rows)
    for k in range(n):
        r1, s1 = eng.evaluate_rows(f.tree_of_row[k:k + 1], f.blens[k:k + 1], f.model_vecs[k:k + 1], site_ll=True)
        np.testing.assert_array_equal(r1[0], rows[k], err_msg="row %d %s alone" % (k, f.rows[k].name))
        np.testing.assert_array_equal(s1[0], site[k], err_msg="row %d %s alone" % (k, f.rows[k].name))
    for perm in (np.random.default_rng(5).permutation(n), np.arange(n)[::-1]):
        r2, s2 = eng.evaluate_rows(f.tree_of_row[perm], f.blens[perm], f.model_vecs[perm], site_ll=True)
        np.testing.assert_array_equal(r2, rows[perm])
        np.testing.assert_array_equal(s2, site[perm])
    eng.close()
