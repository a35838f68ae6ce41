"""CPU: the complex-step reference (oracle/complex_step.py: Taylor expm, no
eigendecomposition, exact derivatives) pinned to the real reference's
recorded data, then the numpy oracle, the host chain rule
(models.q_param_gradients, its batch form) and the C port held to it on the
edge list of tests/exact_cases.py -- spectral ties, near ties, ill-conditioned
models, extreme site rates, short branches.

Bars: the fixtures at tests/test_oracle.py's tolerances; the edge list at the
project's (log L 1e-10, gradients 1e-9, Q-parameter gradients 1e-8 of each
array's largest entry).  Short branches: see test_short_branches_*.
"""
import os

import numpy as np
import pytest

from oracle import complex_step
from oracle import numpy_pruner as npr
from phylostan_amd import models
from phylostan_amd.engine import EvalResult
from tests import cases, report
from tests import exact_cases as ec
from tests.test_oracle import REF_GRAD_RTOL, reference_grad_errors, reference_grad_points

EDGE = [n for g in ec.GROUPS.values() for n in g]
HAVE_C_PORT = os.path.exists(os.path.join(os.path.dirname(os.path.abspath(npr.__file__)), "liboracle_cpu.so"))
needs_c_port = pytest.mark.skipif(not HAVE_C_PORT, reason="oracle/liboracle_cpu.so not built")


# ---- the new reference against the real reference's recorded values

@pytest.mark.parametrize("k", [0, 1])
def test_value_vs_kat_closed_form(k):
    pt = cases.load_kat()["points"][k]
    case = cases.kat_case(pt)
    ll, _ = complex_step.value(case)
    assert abs(ll - pt["loglik"]) < 1e-13
    g = complex_step.gradients(case, only=("blens",))["blens"] * 0.75
    np.testing.assert_allclose(g[[0, 1, 3, 2]], pt["grad_fd"], rtol=2e-7)


def _fixture_points():
    out = [("gtr%d" % k, cases.phylo_case, p) for k, p in enumerate(cases.load_phylo_points())]
    out += [("mixture%d" % k, cases.mixture_case, p) for k, p in enumerate(cases.load_mixture_points())]
    out += [("zero_rate%d" % k, cases.zero_rate_case, p) for k, p in enumerate(cases.load_zero_rate_points())]
    return out


@pytest.mark.parametrize("name,make,pt", _fixture_points(), ids=[p[0] for p in _fixture_points()])
def test_value_vs_reference_fixtures(name, make, pt):
    """Total and per-pattern log L at every phylo_gtr / phylo_mixture /
    phylo_zero_rate point (the reference's scripts/phylo.py)."""
    ll, site = complex_step.value(make(pt))
    atol = 0.0 if name.startswith("zero_rate") else 1e-12  # as tests/test_oracle.py for each fixture
    np.testing.assert_allclose(site, pt["site_ll"], rtol=1e-10, atol=atol)
    assert abs(ll - pt["loglik"]) <= 1e-10 * abs(pt["loglik"])


@pytest.mark.parametrize("k", range(3), ids=["fluA_HKY_W4", "HCV_GTR_W4", "DS1_JC69_unrooted"])
def test_gradients_vs_reference_fd(k):
    """phylo_grad.json: the reference's central differences (branch lengths,
    kappa or exchangeabilities, frequencies, Weibull shape through rs)."""
    pt = reference_grad_points()[k]
    mp = [p for p in cases.load_mixture_points() if p["dataset"] == pt["dataset"]][0]
    case = cases.mixture_case(mp)
    only = ("blens", "rs") if case.model == "JC69" else ("blens", "rs", "rates", "freqs")
    g = complex_step.gradients(case, only=only, branches=pt["branches"])
    gb = np.full(case.blens.size, np.nan)
    gb[pt["branches"]] = g["blens"]
    errs = reference_grad_errors({"grad_blens": gb, "grad_rs": g["rs"], "grad_rates": g.get("rates"),
                                  "grad_freqs": g.get("freqs")}, pt, case)
    assert all(v <= REF_GRAD_RTOL for v in errs.values()), errs


@pytest.mark.parametrize("k", range(4), ids=["fluA_HKY_I_W4", "HCV_GTR_I_W4", "HCV_GTR_I", "fluA_HKY_discrete"])
def test_gradients_vs_reference_zero_rate(k):
    """phylo_zero_rate.json: d/drs, d/dps, d/dblens (and d/dpinv through rs
    and ps) with a zero-rate or free-weight category."""
    pt = cases.load_zero_rate_points()[k]
    case = cases.zero_rate_case(pt)
    g = complex_step.gradients(case, only=("blens", "rs", "ps"), branches=pt["branches"])
    gb = np.full(case.blens.size, np.nan)
    gb[pt["branches"]] = g["blens"]
    errs = cases.zero_rate_errors({"grad_blens": gb, "grad_rs": g["rs"], "grad_ps": g["ps"]}, pt)
    assert all(v <= REF_GRAD_RTOL for v in errs.values()), errs


def test_expm_is_not_an_eigendecomposition():
    """The reference's P-matrix at an exact tie, a defective-looking near tie
    and t = 0, against the JC69 closed form and the semigroup property."""
    t = np.array([0.0, 1e-9, 0.3, 7.0])
    P = complex_step.expm(npr.jc69_q()[None] * t[:, None, None]).real
    e = np.exp(-t / 0.75)
    np.testing.assert_allclose(P[:, 0, 0], 0.25 + 0.75 * e, rtol=0, atol=2e-16 * 8)
    np.testing.assert_allclose(P[:, 0, 1], -0.25 * np.expm1(-t / 0.75), rtol=1e-14, atol=0)  # relative, also at 1e-9
    Q = complex_step.rate_matrix([0.3, 0.2, 0.2 + 5e-13, 0.3 - 5e-13], models.hky_exchangeabilities(4.0))
    a, b, ab = complex_step.expm(np.stack([0.4 * Q, 1.1 * Q, 1.5 * Q]))
    np.testing.assert_allclose((a @ b).real, ab.real, rtol=0, atol=4e-15)


# ---- the oracle, the host chain rule and the C port against the new reference

def _assert_within(errs, bounds, what):
    bad = {k: (v, bounds[k]) for k, v in errs.items() if not v <= bounds[k]}
    assert not bad, "%s: relative error (got, bound) %s" % (what, bad)


@pytest.mark.parametrize("name", EDGE)
def test_numpy_oracle_and_host_chain_rule(name):
    case, truth = ec.get(name)
    errs = ec.errors(ec.oracle_result(case), truth)
    if name.startswith("near"):
        report.record("exact[host] %-16s %s" % (name, ec.fmt(errs)))
    _assert_within(errs, ec.bars(), name)


def test_host_chain_rule_batch_mixes_tie_near_tie_and_generic():
    """q_param_gradients_batch on three draws -- an exact double tie, the
    delta = 5e-13 near tie and a generic point: each draw's rule is its own."""
    names = ["tie2_hky3", "near_5e-13", "ctl_hky3"]
    cs, truths, refs = [], [], []
    for n in names:
        c, t = ec.get(n)
        cs.append(c)
        truths.append(t)
        refs.append(c.oracle())
    gr, gf = models.q_param_gradients_batch(
        np.array([r["dLdP"] for r in refs]), np.array([c.blens for c in cs]), np.array([c.rs for c in cs]),
        np.array([c.freqs for c in cs]), np.array([c.rates for c in cs]),
        np.array([r["grad_freq_root"] for r in refs]))
    for k, n in enumerate(names):
        errs = ec.errors({"grad_rates": gr[k], "grad_freqs": gf[k]}, truths[k])
        _assert_within(errs, ec.bars(), "batch draw %d (%s)" % (k, n))


def _c_port(case):
    from oracle import cpu
    out, sl = cpu.evaluate(case.tipcodes, case.weights, case.peel0, case.rooted, npr.MODEL_IDS[case.model],
                           case.model_vec(), case.blens, case.C, site_ll=True)
    return EvalResult(out, case.blens.size, case.C, sl).as_dict()


@needs_c_port
@pytest.mark.parametrize("name", EDGE)
def test_c_port_and_host_chain_rule(name):
    """oracle/cpu.py: the C port (the device's Jacobi eigensolver, operation
    for operation) plus the host chain rule on its dL/dP."""
    case, truth = ec.get(name)
    _assert_within(ec.errors(_c_port(case), truth), ec.bars(), name)


# ---- short branches: the accuracy limit of V e^{Lambda t} V^-1, stated

EPS = np.finfo(np.float64).eps


@pytest.mark.parametrize("name,t", [("short_1e-4", 1e-4), ("short_1e-8", 1e-8)])
def test_short_branches_numpy_oracle_limit(name, t):
    """P = V e^{Lambda t} V^-1 carries an absolute error of about eps, so its
    off-diagonal entries (of size t) lose eps / t of relative accuracy, and
    with them every output: the reference's own algorithm and accuracy (its
    eigen path), not a defect -- but stated.  Bound: max(project bar, 10 eps /
    t) per output array, the 10 for the handful of short branches and terms
    that add up; a P-matrix path that loses more than that is worse than the
    algorithm."""
    case, truth = ec.get(name)
    errs = ec.errors(ec.oracle_result(case), truth)
    report.record("exact[numpy oracle] %-10s %s" % (name, ec.fmt(errs)))
    _assert_within(errs, {k: max(b, 10.0 * EPS / t) for k, b in ec.bars().items()}, name)


@needs_c_port
@pytest.mark.parametrize("name", ec.SHORT)
def test_short_branches_c_port_no_worse_than_numpy_oracle(name):
    """The C port (Jacobi) against the truth: at most max(project bar, 10 x
    the numpy (LAPACK) oracle's own error at the same point)."""
    case, truth = ec.get(name)
    bounds, oerr = ec.short_branch_bounds(case, truth)
    errs = ec.errors(_c_port(case), truth)
    report.record("exact[C port]       %-10s %s" % (name, ec.fmt(errs)))
    _assert_within(errs, bounds, name)
