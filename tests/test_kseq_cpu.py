"""CPU: the K-state sequence likelihood on the host (``phylostan_amd.kseq``)
against the exact reference of ``tests/kseq_truth.py`` over the shape list,
against the 4-state oracle at K = 4, on a tree whose likelihood leaves the fp64
range, and its refusals.  The bars are the project's: log L and site log L
1e-10 relative, each gradient array 1e-9 of its largest entry."""
import numpy as np
import pytest

from phylostan_amd import models
from phylostan_amd.kseq import HostKStateLikelihood, kseq_host, onehot_masks, param_len, row_len
from tests import cases, kseq_truth as kt

CASES = kt.small_cases()


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_against_the_truth(case):
    rows, site = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None],
                           case.C)
    assert rows.shape == (1, row_len(case.B, case.K, case.C)) and site.shape == (1, case.P)
    ref = kt.load_truth(case)
    err = kt.compare(case, rows[0], site[0], ref)
    print(case.name, {k: "%.2e" % v for k, v in err.items()})
    assert not kt.bars(err), err
    if case.through:  # codon cases: kappa and omega through codon_rates' Jacobian transpose
        from phylostan_amd import codon
        g = case.split_row(rows[0])["rates"]
        kappa, omega = case.through["kappa"][0], case.through["omega"][0]
        g_x6, g_om = codon.codon_rates_backward(np.asarray([1.0, kappa, 1.0, 1.0, kappa, 1.0]), omega, g)
        scale = max(abs(ref["through_kappa"]), abs(ref["through_omega"]))
        assert abs(g_x6[1] + g_x6[4] - ref["through_kappa"]) <= 1e-9 * scale
        assert abs(g_om - ref["through_omega"]) <= 1e-9 * scale


EDGES = kt.edge_cases()


def check_edge_case(case, rows, site):
    """Shared with the GPU tests: one draw of an edge case against its recorded truth, every array at the bars."""
    ref = kt.shared_truth(case)
    assert np.isfinite(rows).all() and not np.isnan(site).any()
    err = kt.compare(case, rows[0], site[0], ref)
    print(case.name, {k: "%.2e" % v for k, v in err.items()})
    if case.name.endswith("deep_inv"):
        # columns 1 and 2 vary: the +I category is exactly 0 there, unshifted, and the live one's shift is past
        # the 1023 bits of fp64's exponent
        assert case.args["rs"][0] == 0.0 and np.all(ref["site"][1:] < -1023 * np.log(2.0))
        for name in kt.NAMES:
            assert name in ref or name + "_dd" in ref
    assert not kt.bars(err), err
    return err


@pytest.mark.parametrize("case", EDGES, ids=[c.name for c in EDGES])
def test_host_on_the_edge_cases(case):
    rows, site = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None],
                           case.C)
    check_edge_case(case, rows, site)


def test_zero_length_branch_is_the_identity():
    # r_c = 0: every message is the child's partial itself, so a constant column's L_c is pi_state exactly
    case = CASES[1]
    masks = np.repeat(onehot_masks(np.full((case.S, 1), 2)), 1, axis=1)
    p = case.params.copy()
    p[case.R + case.K:case.R + case.K + case.C] = 0.0
    _, site = kseq_host(masks, np.ones(1), case.peel, case.rooted, case.blens[None], p[None], case.C)
    assert site[0, 0] == np.log(np.sum(case.args["ps"] * case.args["freqs"][2]))


def test_all_unknown_column_and_invariant_category():
    case = CASES[1]  # K = 4, C = 4, rs[0] = 0, the last column all unknown
    assert case.args["rs"][0] == 0.0
    _, site = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None], case.C)
    assert abs(site[0, -1]) < 1e-14  # L_i = 1


def test_rescaling_on_a_400_tip_caterpillar():
    case = kt.caterpillar400()
    ref = kt.load_truth(case, only=("blens",))
    rows, site = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None],
                           case.C)
    assert ref["loglik"] < -1500.0  # exp of a site's share is far below the fp64 range's 1e-308
    got = case.split_row(rows[0])
    assert abs(got["loglik"] - ref["loglik"]) <= 1e-10 * abs(ref["loglik"])
    assert np.max(np.abs(got["blens"] - ref["blens"])) <= 1e-9 * np.max(np.abs(ref["blens"]))


def _nucleotide_masks(tipcodes):
    return np.asarray(tipcodes, np.uint64)  # A=1 C=2 G=4 T=8: states 0..3 in the oracle's order


def _against_oracle(case):
    ref = case.oracle()
    gr, gf = models.q_param_gradients(ref["dLdP"], case.blens, case.rs, case.freqs, case.rates, ref["grad_freq_root"])
    # exchangeabilities AC AG AT CG CT GT are the strict lower triangle column by column of (A, C, G, T)
    params = np.concatenate([case.rates, case.freqs, case.rs, case.ps])
    rows, site = kseq_host(_nucleotide_masks(case.tipcodes), case.weights, case.peel0, case.rooted, case.blens[None],
                           params[None], case.C)
    B, C = case.blens.size, case.C
    row = rows[0]
    unk = np.all(np.asarray(case.tipcodes) == 15, axis=0)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))  # noqa: E731
    err = {"loglik": abs(row[0] - ref["loglik"]) / abs(ref["loglik"]),
           # a column of gaps has log L_i = 0 exactly: those columns alone absolutely, as kseq_truth.compare
           "site": float(np.max(np.abs(site[0][~unk] - ref["site_ll"][~unk]) / np.abs(ref["site_ll"][~unk]))),
           "site_unknown": float(np.max(np.abs(site[0][unk]))) if unk.any() else 0.0,
           "blens": rel(row[1:1 + B], ref["grad_blens"]), "rs": rel(row[1 + B:1 + B + C], ref["grad_rs"]),
           "ps": rel(row[1 + B + C:1 + B + 2 * C], ref["grad_ps"])}
    o = 1 + B + 2 * C
    if case.model != "JC69":
        err["rates"] = rel(row[o:o + 6], gr)
        err["freqs"] = rel(row[o + 6:o + 10], gf)
    print(case.name, {k: "%.2e" % v for k, v in err.items()})
    return err


def test_k4_fluA_gtr_against_the_4_state_oracle():
    base = cases.fluA_case()
    rates = np.asarray([1.1, 5.58, 0.7, 1.3, 4.9, 1.0])
    case = cases.Case("fluA-GTR", base.tipcodes, base.weights, base.peel0, True, "GTR", 4, base.blens, base.freqs,
                      rates / rates.sum(), base.rs, base.ps)
    assert not kt.bars(_against_oracle(case))


def test_k4_ds1_jc69_against_the_4_state_oracle():
    assert not kt.bars(_against_oracle(cases.ds1_case()))


def test_bad_draws_leave_their_neighbours_alone():
    case = CASES[4]
    good = case.params
    R, K = case.R, case.K
    zero_freq = good.copy()
    zero_freq[R + 2] = 0.0
    neg_rate = good.copy()
    neg_rate[3] = -0.1
    nan_ps = good.copy()
    nan_ps[-1] = np.nan
    lik = HostKStateLikelihood(case.masks, case.weights, case.peel, case.rooted, K, case.C)
    alone = lik.evaluate_rows(case.blens[None], good[None])
    batch, site = lik.evaluate_rows(np.repeat(case.blens[None], 5, 0), np.stack([good, zero_freq, neg_rate, nan_ps, good]),
                                    site_ll=True)
    for k in (1, 2, 3):
        assert batch[k, 0] == -np.inf and not batch[k, 1:].any() and np.all(site[k] == -np.inf)
    np.testing.assert_array_equal(batch[0], alone[0])
    np.testing.assert_array_equal(batch[4], alone[0])


def test_zero_likelihood_pattern_is_a_bad_draw():
    # two tips in different states joined by zero-length branches, no path between them: L_i = 0
    masks = onehot_masks(np.asarray([[0], [1], [0]]))
    peel = np.asarray([[0, 1, 3], [2, 3, 4]], np.int32)
    params = np.concatenate([[1.0], [0.5, 0.5], [1.0], [1.0]])
    rows, site = kseq_host(masks, np.ones(1), peel, False, np.zeros((1, 3)), params[None], 1)
    assert rows[0, 0] == -np.inf and not rows[0, 1:].any() and site[0, 0] == -np.inf
    assert params.size == param_len(2, 1)
