"""The edge list of the exact-gradient tests (tests/test_complex_step.py on
the CPU, tests/test_gpu_exact_gradients.py on the GPU) and the complex-step
truth of each case (oracle/complex_step.py), computed once per process.

Seeds and sizes are fixed: the near-tie and short-branch error tables of
DESIGN.md ("Accuracy against an exact reference") reproduce from them.
"""
import numpy as np

from oracle import complex_step
from phylostan_amd import models
from tests import cases

# the project's bars (tests/test_gpu_parity.py): log L, gradients, Q-parameter gradients
BAR_LL, BAR_G, BAR_Q = 1e-10, 1e-9, 1e-8


def _hky3():
    return cases.random_case(3, S=12, P=130, C=4, model="HKY")


def _gtr7():
    return cases.random_case(7, S=12, P=130, C=4, model="GTR")


def _hky7():
    return cases.random_case(7, S=12, P=130, C=4, model="HKY")


def split_purine_pyrimidine(delta):
    """HKY case 3 with piR - piY = 2 delta: delta = 0 is an exact double
    eigenvalue (-1/s twice), delta > 0 splits it by about 3.6 delta."""
    c = _hky3()
    c.freqs = np.array([0.3, 0.2, 0.2 + delta, 0.3 - delta])
    return c


def _with(make, **kw):
    c = make()
    for k, v in kw.items():
        setattr(c, k, np.asarray(v, dtype=np.float64))
    return c


def _weibull_005():
    c = _gtr7()
    c.rs, c.ps = models.weibull_site_rates(0.05, 4)  # rs from 6e-24 to 4.0
    return c


def _zero_rate():
    return cases.zero_rate_case(cases.load_zero_rate_points()[0])  # fluA HKY +I +W4: rs[0] = 0


def short_branches(t):
    c = _gtr7()
    c.blens[::3] = t
    return c


CASES = {
    # 1. generic controls
    "ctl_hky3": _hky3,
    "ctl_gtr7": _gtr7,
    "ctl_gtr4_unrooted": lambda: cases.random_case(4, S=17, P=257, C=5, model="GTR", rooted=False),
    # 2. exact double tie
    "tie2_hky3": lambda: split_purine_pyrimidine(0.0),
    "tie2_hcv": cases.hcv_case,
    # 3. exact triple tie
    "tie3_jc_as_gtr7": lambda: _with(_gtr7, rates=np.ones(6), freqs=np.full(4, 0.25)),
    "tie3_f81_hky7": lambda: _with(_hky7, rates=np.ones(6)),
    # 4. near ties
    "near_5e-13": lambda: split_purine_pyrimidine(5e-13),
    "near_1e-11": lambda: split_purine_pyrimidine(1e-11),
    "near_1e-9": lambda: split_purine_pyrimidine(1e-9),
    "near_1e-7": lambda: split_purine_pyrimidine(1e-7),
    "near_kappa1": lambda: _with(_hky7, rates=models.hky_exchangeabilities(1.0 + 1e-10)),
    # 5. conditioning
    "cond_freq1e-6": lambda: _with(_gtr7, freqs=[1e-6, 0.3, 0.3, 0.4 - 1e-6]),
    "cond_kappa1000": lambda: _with(_hky7, rates=models.hky_exchangeabilities(1000.0)),
    "cond_rates": lambda: _with(_gtr7, rates=[1e-3, 10.0, 1e-2, 1.0, 100.0, 0.1]),
    # 6. site rates
    "rs_weibull005": _weibull_005,
    "rs_zero": _zero_rate,
    # 7. short branches (bound measured in the test, see short_branch_bounds)
    "short_1e-4": lambda: short_branches(1e-4),
    "short_1e-8": lambda: short_branches(1e-8),
}

GROUPS = {
    "controls": ["ctl_hky3", "ctl_gtr7", "ctl_gtr4_unrooted"],
    "double_tie": ["tie2_hky3", "tie2_hcv"],
    "triple_tie": ["tie3_jc_as_gtr7", "tie3_f81_hky7"],
    "near_tie": ["near_5e-13", "near_1e-11", "near_1e-9", "near_1e-7", "near_kappa1"],
    "conditioning": ["cond_freq1e-6", "cond_kappa1000", "cond_rates"],
    "site_rates": ["rs_weibull005", "rs_zero"],
}
SHORT = ["short_1e-4", "short_1e-8"]

ARRAYS = ("loglik", "site_ll", "grad_blens", "grad_rs", "grad_ps", "grad_freq_root", "grad_rates", "grad_freqs")

_TRUTH = {}


def truth_of(case):
    """Complex-step log L, site_ll and gradients of a case, as a dict with
    the names of ARRAYS (no grad_rates / grad_freqs for JC69)."""
    ll, site = complex_step.value(case)
    g = complex_step.gradients(case, only=("blens", "rs", "ps", "freq_root") if case.model == "JC69" else None)
    out = dict(loglik=ll, site_ll=site, grad_blens=g["blens"], grad_rs=g["rs"], grad_ps=g["ps"],
               grad_freq_root=g["freq_root"])
    if case.model != "JC69":
        out["grad_rates"], out["grad_freqs"] = g["rates"], g["freqs"]
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


def get(name):
    """(case, truth) of an edge-list entry; the truth is computed once."""
    case = CASES[name]()
    if name not in _TRUTH:
        _TRUTH[name] = truth_of(case)
    return case, _TRUTH[name]


def batch_draws():
    """Four draws of HKY case 3 for one batched call: three generic points
    and, at index 2, the delta = 5e-13 near tie.  -> (cases, truths)."""
    rng = np.random.default_rng(43)
    cs = []
    for k in range(4):
        if k == 2:
            cs.append(split_purine_pyrimidine(5e-13))
            continue
        c = _hky3()
        c.freqs = rng.dirichlet(np.full(4, 5.0))
        c.rates = models.hky_exchangeabilities(rng.uniform(1.5, 8.0))
        c.blens = c.blens * rng.uniform(0.7, 1.4, c.blens.size)
        cs.append(c)
    if "batch" not in _TRUTH:
        _TRUTH["batch"] = [truth_of(c) for c in cs]
    return cs, _TRUTH["batch"]


def rel_err(got, ref):
    """Max |got - ref| over the array / the largest |ref| (tests/test_gpu_parity._close's measure)."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref)) / max(np.max(np.abs(ref)), 1e-300))


def errors(res, truth):
    """Relative error per output array of a result (a dict with ARRAYS' names)
    against the truth; site_ll per entry, relative with the parity tests'
    absolute floor of 1e-12 taken off first."""
    out = {}
    for k in ARRAYS:
        if k not in truth or k not in res:
            continue
        if k == "loglik":
            out[k] = abs(res[k] - truth[k]) / abs(truth[k])
        elif k == "site_ll":
            d = np.maximum(np.abs(np.asarray(res[k]) - truth[k]) - 1e-12, 0.0)
            out[k] = float(np.max(d / np.maximum(np.abs(truth[k]), 1e-300)))
        else:
            out[k] = rel_err(res[k], truth[k])
    return out


def bars():
    """The project's bar of each output array."""
    b = {k: BAR_G for k in ARRAYS}
    b["loglik"] = b["site_ll"] = BAR_LL
    b["grad_rates"] = b["grad_freqs"] = BAR_Q
    return b


def oracle_result(case):
    """The numpy oracle plus the host chain rule, in ARRAYS' names."""
    ref = case.oracle()
    out = {k: ref[k] for k in ARRAYS if k in ref}
    if case.model != "JC69":
        out["grad_rates"], out["grad_freqs"] = models.q_param_gradients(
            ref["dLdP"], case.blens, case.rs, case.freqs, case.rates, ref["grad_freq_root"])
    return out


def short_branch_bounds(case, truth):
    """Per output array: max(project bar, 10 x the numpy oracle's own error
    against the truth at this point) -- V e^{Lambda t} V^-1 loses eps / t of
    relative accuracy in P's off-diagonal at a branch of length t, in the
    reference's algorithm as in ours; the 10 covers LAPACK-versus-Jacobi
    rounding in an error that is not deterministic in its last digit.
    -> (bounds, the oracle's errors)."""
    oerr = errors(oracle_result(case), truth)
    b = bars()
    return {k: max(b[k], 10.0 * v) for k, v in oerr.items()}, oerr


def fmt(errs):
    return " ".join("%s %.1e" % (k.replace("grad_", "d"), v) for k, v in errs.items())
