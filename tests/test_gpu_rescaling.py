"""GPU: the rescaled pattern sweep (phy_set_rescaling) against the
extended-range oracle (tests/extended_oracle.py) on trees whose per-site
likelihood leaves fp64, at the parity bars of tests/test_gpu_parity.py;
no harm where nothing underflows; off means untouched."""
import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

from tests import cases
from tests.extended_oracle import extended_oracle, require_extended
from tests.test_gpu_parity import RTOL_G, RTOL_LL, _close, check_case

pytestmark = pytest.mark.gpu


def _zero_rate(case):
    case.rs = case.rs.copy()
    case.rs[0] = 0.0  # a +I-like category: P = I on every branch
    return case


# 700 taxa: every site is -inf without rescaling
UNDERFLOWING = {
    "gtr_c2_p130": lambda: cases.random_case(911, S=700, P=130, C=2, model="GTR"),
    "hky_c4": lambda: cases.random_case(912, S=700, P=70, C=4, model="HKY"),
    "jc69_unrooted": lambda: cases.random_case(913, S=700, P=70, C=1, model="JC69", rooted=False),
    "caterpillar": lambda: cases.random_case(918, S=700, P=70, C=2, model="GTR", caterpillar=True),
    "zero_rate": lambda: _zero_rate(cases.random_case(917, S=700, P=70, C=3, model="GTR")),
}

_REFS = {}


def _case_and_ref(name):
    """The case and its extended-range reference, computed once per session."""
    require_extended()
    if name not in _REFS:
        case = UNDERFLOWING[name]()
        _REFS[name] = (case, extended_oracle(case))
    return _REFS[name]


def _engine(case, max_draws=1, rescaling=True, **kw):
    from phylostan_amd.engine import TreeLikelihood
    return TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                          max_draws=max_draws, rescaling=rescaling, **kw)


def check_against(case, ref, res):
    """check_case's comparisons and bars (tests/test_gpu_parity.py) against a
    given reference dict; a compact row has no dL/dP block and a raw row no
    per-site values to compare."""
    if res.site_ll is not None:
        np.testing.assert_allclose(res.site_ll, ref["site_ll"], rtol=RTOL_LL, atol=1e-12)
    assert abs(res.loglik - ref["loglik"]) <= RTOL_LL * abs(ref["loglik"]) + 1e-12
    if res.dLdP is not None:
        _close(res.dLdP, ref["dLdP"], RTOL_G, "dLdP")
    _close(res.grad_blens, ref["grad_blens"], RTOL_G, "grad_blens")
    _close(res.grad_rs, ref["grad_rs"], RTOL_G, "grad_rs")
    _close(res.grad_ps, ref["grad_ps"], RTOL_G, "grad_ps")
    _close(res.grad_freq_root, ref["grad_freq_root"], RTOL_G, "grad_freq_root")
    if case.model == "JC69":
        assert not np.any(res.grad_rates) and not np.any(res.grad_freqs)
    else:
        from phylostan_amd import models
        gr, gf = models.q_param_gradients(ref["dLdP"], case.blens, case.rs, case.freqs, case.rates,
                                          ref["grad_freq_root"])
        _close(res.grad_rates, gr, 1e-8, "grad_rates")
        _close(res.grad_freqs, gf, 1e-8, "grad_freqs")


# ---- 1. underflowing trees --------------------------------------------------

@pytest.mark.parametrize("name", list(UNDERFLOWING))
def test_underflowing_single_draw(name):
    """One draw over several workgroups (the finalize / gsum path)."""
    case, ref = _case_and_ref(name)
    eng = _engine(case)
    assert eng.rescaling() and eng.engine() == "pattern"
    check_against(case, ref, eng.evaluate(case.blens, case.model_vec(), site_ll=True))


@pytest.mark.parametrize("n", [4, 40])
@pytest.mark.parametrize("name", list(UNDERFLOWING))
def test_underflowing_batched_rows(name, n):
    """Perturbed branch lengths through evaluate_rows, first and last draw
    (as test_large_cb_batched_rows_vs_oracle)."""
    case, _ = _case_and_ref(name)
    eng = _engine(case, n)
    rng = np.random.default_rng(5)
    bl = case.blens[None, :] * rng.uniform(0.8, 1.25, (n, case.blens.size))
    mv = np.repeat(case.model_vec()[None], n, axis=0)
    rows = eng.evaluate_rows(bl, mv)
    assert np.all(np.isfinite(rows))
    for k in (0, n - 1):
        ref = extended_oracle(case, bl[k])
        assert abs(rows[k, 0] - ref["loglik"]) <= RTOL_LL * abs(ref["loglik"])
        _close(rows[k, 1:1 + eng.B], ref["grad_blens"], RTOL_G, "grad_blens draw %d" % k)


def test_without_rescaling_the_same_tree_is_minus_inf():
    case, _ = _case_and_ref("gtr_c2_p130")
    eng = _engine(case, rescaling=False)
    assert not eng.rescaling()
    res = eng.evaluate(case.blens, case.model_vec(), site_ll=True)
    assert res.loglik == -np.inf and np.all(np.isneginf(res.site_ll))


# ---- 2. the silent-error band ------------------------------------------------

def test_silent_error_band():
    """450 taxa: without rescaling most sites are finite but subnormal, and
    wrong far beyond the parity bar with no warning; rescaled, all 130 sites
    meet it."""
    require_extended()
    case = cases.random_case(916, S=450, P=130, C=2, model="GTR")
    ref = extended_oracle(case)
    check_against(case, ref, _engine(case).evaluate(case.blens, case.model_vec(), site_ll=True))
    off = _engine(case, rescaling=False).evaluate(case.blens, case.model_vec(), site_ll=True)
    with np.errstate(invalid="ignore"):
        err = np.abs(off.site_ll - ref["site_ll"]) / np.abs(ref["site_ll"])
    print("unscaled: %d non-finite sites, worst finite site off by %.3e relative"
          % (np.sum(~np.isfinite(off.site_ll)), np.max(err[np.isfinite(err)], initial=0.0)))
    assert np.any(~np.isfinite(off.site_ll)) or np.max(err) > 1e-6


# ---- 3. every plan -----------------------------------------------------------

def _plan_cols1(eng):
    eng.set_tuning(cols=1)
    assert eng.lds_plan()["cols"] == 1


def _plan_cols2(eng):
    eng.set_tuning(cols=2)
    assert eng.lds_plan()["cols"] == 2


def _plan_deep_lds(eng):
    eng.set_deep_stack(1)
    assert eng.lds_plan()["deep_lds_entries"] == eng.program_info()["depth"]


def _plan_deep_global(eng):
    eng.set_deep_stack(2)
    assert eng.lds_plan()["deep_lds_entries"] == 0


def _plan_cols1_deep_global(eng):
    eng.set_tuning(cols=1)
    _plan_deep_global(eng)


def _plan_cols2_deep_global(eng):
    eng.set_tuning(cols=2)
    _plan_deep_global(eng)


def _plan_no_recompute(eng):
    eng.set_recompute(False)
    assert eng.lds_plan()["recomputed"] == 0


def _plan_chunked(eng):
    eng.set_tuning(lds_budget=48 * 1024)
    assert eng.lds_plan()["n_chunks"] >= 3


def _plan_compact(eng):
    eng.set_output(compact=True)


PLANS = {"cols1": _plan_cols1, "cols2": _plan_cols2, "deep_lds": _plan_deep_lds, "deep_global": _plan_deep_global,
         "cols1_deep_global": _plan_cols1_deep_global, "cols2_deep_global": _plan_cols2_deep_global,
         "no_recompute": _plan_no_recompute, "chunked": _plan_chunked, "compact": _plan_compact}


@pytest.mark.parametrize("plan", list(PLANS))
def test_every_plan(plan):
    case, ref = _case_and_ref("gtr_c2_p130")
    eng = _engine(case)
    PLANS[plan](eng)
    assert eng.rescaling()
    check_against(case, ref, eng.evaluate(case.blens, case.model_vec(), site_ll=True))


def test_two_shards_on_one_device():
    case, ref = _case_and_ref("gtr_c2_p130")
    eng = _engine(case, devices=[0, 0])
    assert eng.rescaling()
    check_against(case, ref, eng.evaluate(case.blens, case.model_vec(), site_ll=True))


@pytest.mark.parametrize("cols", [1, 2])
def test_one_workgroup_per_draw(cols):
    """A workgroup budget of one per draw: the sweep loops over its draw's
    blocks (dL/dP slots by atomic adds) and runs the fused epilogue."""
    case, ref = _case_and_ref("gtr_c2_p130")
    n = 4
    eng = _engine(case, n)
    eng.set_tuning(wg_budget=n, cols=cols)
    rows = eng.evaluate_rows(np.repeat(case.blens[None], n, axis=0), np.repeat(case.model_vec()[None], n, axis=0))
    from phylostan_amd.engine import EvalResult
    for k in (0, n - 1):
        check_against(case, ref, EvalResult(rows[k], eng.B, case.C))


# ---- 4. no harm where nothing underflows -------------------------------------

@pytest.mark.parametrize("make", [cases.fluA_case, cases.hcv_case, cases.ds1_case,
                                  lambda: cases.random_case(901, S=12)],
                         ids=["fluA", "HCV", "DS1", "rand901"])
def test_no_harm_where_nothing_underflows(make):
    case = make()
    on = check_case(case, _engine(case))
    off = _engine(case, rescaling=False).evaluate(case.blens, case.model_vec(), site_ll=True)
    np.testing.assert_allclose(on.site_ll, off.site_ll, rtol=1e-13, atol=0)
    assert abs(on.loglik - off.loglik) <= 1e-13 * abs(off.loglik)
    for k in ("dLdP", "grad_blens", "grad_rs", "grad_ps", "grad_freq_root"):
        _close(getattr(on, k), getattr(off, k), 1e-13, "scaled vs unscaled " + k)


# ---- 5. off means untouched ---------------------------------------------------

@pytest.mark.parametrize("n", [4, 64])
def test_toggled_off_is_bitwise_untouched(n):
    """4 draws: the quad sweep; 64: the column sweep."""
    case = cases.fluA_case()
    rng = np.random.default_rng(3)
    bl = case.blens[None, :] * rng.uniform(0.8, 1.25, (n, case.blens.size))
    mv = np.repeat(case.model_vec()[None], n, axis=0)
    plain = _engine(case, n, rescaling=False).evaluate_rows(bl, mv)
    eng = _engine(case, n, rescaling=False)
    eng.set_rescaling(True)
    assert eng.rescaling()
    eng.set_rescaling(False)
    assert not eng.rescaling()
    assert np.array_equal(eng.evaluate_rows(bl, mv), plain)


def test_rescaling_keeps_the_pattern_sweep():
    from phylostan_amd import _lib
    case = cases.random_case(901, S=12)
    eng = _engine(case, rescaling=False)
    eng.set_engine("class")
    assert eng.engine() == "class"
    eng.set_rescaling(True)
    assert eng.engine() == "pattern" and eng.prefer_latency_engine() == "pattern"
    with pytest.raises(_lib.PhyloHipError, match="rescaling needs the pattern sweep"):
        eng.set_engine("class")
    eng.set_rescaling(False)  # the preference set before comes back
    assert eng.engine() == "class"
    check_case(case, eng)
