"""GPU: the HIP path against the complex-step reference (oracle/
complex_step.py) -- not against the oracle or the host chain rule, which
share the kernels' algebra (the Jacobi eigensolver, the divided differences
Phi_kl and their tie rule) -- on the edge list of tests/exact_cases.py:
spectral ties, near ties, ill-conditioned models, extreme site rates, short
branches.

Every case runs through the three places that hold the Phi rule and a
Q-parameter epilogue:
  column  the one / two column sweeps, qgrad_body (PHY_QUAD=0, two columns)
  quad    the quad sweep, qfin_kernel (the default for a call of <= 32 draws)
  class   the class sweep, cls_epi_kernel

Bars as tests/test_gpu_parity.py: log L 1e-10, gradients 1e-9, Q-parameter
gradients 1e-8 of each array's largest entry.  Short branches: at most
max(bar, 10 x the numpy oracle's own error against the truth) -- see
exact_cases.short_branch_bounds.
"""
import os

import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

from tests import cases, report
from tests import exact_cases as ec
from tests.test_gpu_parity import RTOL_G, RTOL_LL, _close, _engine

pytestmark = pytest.mark.gpu

FORMS = ["column", "quad", "class"]
assert (ec.BAR_LL, ec.BAR_G) == (RTOL_LL, RTOL_G)


def make_engine(case, form, monkeypatch, max_draws=1):
    """An engine that runs ``form``, with the evidence that it does."""
    monkeypatch.setenv("PHY_QUAD", "0" if form == "column" else "1")
    eng = _engine(case, max_draws=max_draws)
    if form == "class":
        eng.set_engine("class")
        assert eng.engine() == "class"
        return eng
    assert eng.engine() == "pattern"  # (the automatic choice on alignments this small)
    if form == "column":
        eng.set_tuning(0, 2, 0)  # a column preference also keeps the quad sweep off
        assert eng.lds_plan()["cols"] == 2
    else:
        assert eng.quad_plan()["waves"] >= 1, "the quad sweep does not apply to this context"
    return eng


def device_errors(case, truth, form, monkeypatch):
    eng = make_engine(case, form, monkeypatch)
    res = eng.evaluate(case.blens, case.model_vec(), site_ll=True)
    return ec.errors(res.as_dict(), truth)


def _check(failures, name, errs, bounds):
    for k, v in errs.items():
        if not v <= bounds[k]:
            failures.append("%s %s: %.3e > %.1e" % (name, k, v, bounds[k]))


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("group", sorted(ec.GROUPS))
def test_edge_list(group, form, monkeypatch):
    failures = []
    for name in ec.GROUPS[group]:
        case, truth = ec.get(name)
        errs = device_errors(case, truth, form, monkeypatch)
        if group == "near_tie":
            report.record("exact[%-6s] %-12s %s" % (form, name, ec.fmt(errs)))
        _check(failures, name, errs, ec.bars())
    assert not failures, failures


@pytest.mark.parametrize("form", FORMS + ["column-one-workgroup-per-draw"])
def test_near_tie_draw_inside_a_batch(form, monkeypatch):
    """One 4-draw call: the delta = 5e-13 near tie at index 2 between three
    generic draws.  The tie marks are per draw: every draw meets the bars.
    The quad form runs its multi-wave sweep here (4 waves per category); the
    last form folds the finalize and qgrad_body into the sweep (one workgroup
    per draw: qgrad_body reads the finished dL/dP rows, not the slots)."""
    cs, truths = ec.batch_draws()
    eng = make_engine(cs[0], form.split("-")[0], monkeypatch, max_draws=4)
    if form == "quad":
        assert eng.quad_plan()["waves"] >= 2, eng.quad_plan()
    if form == "column-one-workgroup-per-draw":
        eng.set_tuning(4, 2, 0)
        assert eng.lds_plan()["cols"] == 2
    res = eng.evaluate_batch(np.array([c.blens for c in cs]), np.array([c.model_vec() for c in cs]), site_ll=True)
    failures = []
    for k, (r, t) in enumerate(zip(res, truths)):
        _check(failures, "draw %d" % k, ec.errors(r.as_dict(), t), ec.bars())
    assert not failures, failures


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", ec.SHORT)
def test_short_branches_no_worse_than_reference_algorithm(name, form, monkeypatch):
    """Branches of length t = 1e-4 / 1e-8: V e^{Lambda t} V^-1 loses eps / t,
    in the reference's algorithm as on the device.  The device against the
    truth: at most max(bar, 10 x the numpy oracle's error at the same point)."""
    case, truth = ec.get(name)
    bounds, oerr = ec.short_branch_bounds(case, truth)
    errs = device_errors(case, truth, form, monkeypatch)
    report.record("exact[oracle] %-12s %s" % (name, ec.fmt(oerr)))
    report.record("exact[%-6s] %-12s %s" % (form, name, ec.fmt(errs)))
    failures = []
    _check(failures, name, errs, bounds)
    assert not failures, failures


PARENT_ROWS = os.path.join(cases.GOLDEN, "device_rows_before_near_rule.npz")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("make", [cases.fluA_case, cases.hcv_case], ids=["fluA", "HCV"])
def test_rows_outside_the_near_window_keep_their_bits(make, form, monkeypatch):
    """fluA (every gap well separated) and HCV (K80 spectrum: an exact double
    tie, the tie rule) have no pair inside the near window: their compact rows
    are bit for bit the rows the MI355X gave before the near rule existed
    (tests/golden/device_rows_before_near_rule.npz, recorded at that commit
    with this test's calls).  A change of the epilogues' arithmetic made on
    purpose re-records the file; one made by accident shows here."""
    case = make()
    eng = make_engine(case, form, monkeypatch)
    eng.set_output(compact=True)
    row = eng.evaluate_rows(case.blens[None], case.model_vec()[None])[0]
    want = np.load(PARENT_ROWS, allow_pickle=False)["%s_%s" % (case.name, form)]
    if not np.array_equal(row, want):
        _close(row, want, 0.0, "%s %s row against the recorded row" % (case.name, form))
