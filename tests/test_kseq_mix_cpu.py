"""CPU: the mixture of M K-state models over sites on the host (``kseq.kseq_mix_host``,
``HostKStateMixLikelihood``) against the independent complex-step truth of
``tests/kseq_mix_truth.py``, at the project's bars (``mt.bars``): log L and site
log L 1e-10 relative, each gradient array 1e-9 of its largest entry, the class
posteriors 1e-9 absolute and their sum 1 to 1e-12."""
import numpy as np
import pytest

from phylostan_amd import kseq
from phylostan_amd.kseq import HostKStateMixLikelihood, kseq_host, kseq_mix_host, mix_param_len, mix_row_len
from tests import kseq_mix_truth as mt
from tests import kseq_truth as kt

CASES = mt.small_cases()


def _host(case):
    return HostKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C)


def check_against_truth(lik, case):
    """Shared with the GPU tests: one draw of ``case`` on ``lik`` against the truth; the errors."""
    rows, site, post = lik.evaluate_rows(case.blens[None], case.params[None], site_ll=True, class_post=True)
    assert rows.shape == (1, mix_row_len(case.B, case.K, case.M, case.C))
    assert site.shape == (1, case.P) and post.shape == (1, case.M, case.P)
    err = mt.compare(case, rows[0], site[0], post[0], mt.shared_truth(case))
    print(case.name, {k: "%.2e" % v for k, v in err.items()})
    return err, rows, site, post


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_host_against_the_truth(case):
    err, _, _, post = check_against_truth(_host(case), case)
    assert not mt.bars(err), err
    if case.name.endswith("dead1"):  # a component whose weights are all 0 is never alive, and no refusal
        assert not post[0, 1].any()
        assert np.all(post[0, 0] > 0)


EDGES = mt.edge_cases()


@pytest.mark.parametrize("case", EDGES, ids=[c.name for c in EDGES])
def test_host_on_the_edge_cases(case):
    assert case.M == kseq.MMAX and case.M * case.C == kseq.CMAX
    err, _, _, _ = check_against_truth(_host(case), case)
    assert not mt.bars(err), err


def zero_weight_case():
    """K = 5, M = 2, C = 2, P = 15 with the weight of column 3 set to 0: a column of positive likelihood that counts
    for nothing in log L and its gradient, and still has its site log L and class posteriors."""
    case = mt.random_mix("K5_S7_P15_M2_C2_rooted_w0", 7, 5, 15, 2, 2, True, 9)
    case.weights[3] = 0.0
    assert not kt.unknown_columns(case.masks, case.K)[3]
    return case


def check_zero_weight_column(lik, case):
    """Shared with the GPU tests: the row, the site log L and the posteriors against the truth of the case as given."""
    ref = mt.shared_truth(case)
    err, rows, site, post = check_against_truth(lik, case)
    assert not mt.bars(err), err
    assert np.isfinite(ref["site"][3]) and abs(site[0, 3] - ref["site"][3]) <= 1e-10 * abs(ref["site"][3])
    want = np.exp(ref["class"][:, 3] - ref["site"][3])
    assert np.all(want > 0) and np.max(np.abs(post[0][:, 3] - want)) <= 1e-9
    # the column counts for nothing: the row is that of the alignment without it (to the rounding of the sums)
    rest = np.arange(case.P) != 3
    less = type(lik)(case.masks[:, rest], case.weights[rest], case.peel, case.rooted, case.K, case.M, case.C)
    rows2 = less.evaluate_rows(case.blens[None], case.params[None])
    less.close()
    np.testing.assert_allclose(rows[0], rows2[0], rtol=1e-12, atol=1e-12 * np.max(np.abs(rows2[0])))


def dead_column_cases():
    """K = 2, every branch of length 0.  Column 0's tips conflict (no path: L_i = 0 exactly) and its weight is 0;
    column 1 is constant with weight 2.  The case as given, and the alignment without column 0."""
    masks = kseq.onehot_masks(np.asarray([[0, 1], [1, 1], [0, 1]]))
    peel = np.asarray([[0, 1, 3], [2, 3, 4]], np.int32)
    comps = [(np.asarray([1.0]), np.asarray([0.5, 0.5])), (np.asarray([2.5]), np.asarray([0.3, 0.7]))]
    rs, ps = [[1.0], [0.5]], [[0.4], [0.6]]
    full = mt.MixCase("K2_S3_P2_M2_C1_dead_column", masks, [0.0, 2.0], peel, False, np.zeros(3), comps, rs, ps)
    live = mt.MixCase("K2_S3_P1_M2_C1_live_column", masks[:, 1:], [2.0], peel, False, np.zeros(3), comps, rs, ps)
    return full, live


def check_dead_zero_weight_column(lik, full, live):
    """Shared with the GPU tests: a zero-weight column of zero likelihood is not a bad draw."""
    rows, site, post = lik.evaluate_rows(full.blens[None], full.params[None], site_ll=True, class_post=True)
    assert np.isfinite(rows).all()
    assert site[0, 0] == -np.inf and not post[0][:, 0].any()
    err = mt.compare(live, rows[0], site[0, 1:], post[0][:, 1:], mt.shared_truth(live))
    print(full.name, {k: "%.2e" % v for k, v in err.items()})
    assert not mt.bars(err), err


def test_zero_weight_column_of_positive_likelihood():
    case = zero_weight_case()
    check_zero_weight_column(_host(case), case)


def test_zero_weight_column_of_zero_likelihood():
    full, live = dead_column_cases()
    check_dead_zero_weight_column(_host(full), full, live)
    # with a weight the same column refuses the draw
    lik = HostKStateMixLikelihood(full.masks, np.asarray([1.0, 2.0]), full.peel, full.rooted, full.K, full.M, full.C)
    rows, site, post = lik.evaluate_rows(full.blens[None], full.params[None], site_ll=True, class_post=True)
    assert rows[0, 0] == -np.inf and not rows[0, 1:].any() and np.all(site == -np.inf) and not post.any()


def test_lengths():
    assert mix_param_len(61, 3, 4) == 3 * (1830 + 61) + 24 and mix_row_len(10, 5, 2, 2) == 1 + 10 + 8 + 2 * 15
    assert mix_param_len(5, 1, 4) == kseq.param_len(5, 4) and mix_row_len(7, 5, 1, 4) == kseq.row_len(7, 5, 4)


def test_one_component_is_kseq_host():
    case = kt.small_cases()[4]  # K = 17, C = 4
    rows, site = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None],
                           case.C)
    mrows, msite, post = kseq_mix_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None],
                                       case.params[None], case.K, 1, case.C)
    np.testing.assert_array_equal(mrows, rows)
    np.testing.assert_array_equal(msite, site)
    assert np.max(np.abs(post - 1.0)) <= 1e-15


def two_identical(case1, w=(0.3, 0.7)):
    """The M = 2 params of a C = 1 single-model case's component taken twice with weights ``w``."""
    a = case1.args
    comp = np.concatenate([a["rates"], a["freqs"]])
    return np.concatenate([comp, comp, [a["rs"][0], a["rs"][0]], list(w)])


def check_two_identical(one, two, case1):
    """Two identical components: the posteriors split as their weights, log L and d/dblens are the single
    model's (to rounding: the sum over components is reassociated), the component blocks split as the weights."""
    w = (0.3, 0.7)
    r1, s1 = one.evaluate_rows(case1.blens[None], case1.params[None], site_ll=True)
    r2, s2, post = two.evaluate_rows(case1.blens[None], two_identical(case1, w)[None], site_ll=True, class_post=True)
    B, R, K = case1.B, case1.R, case1.K
    assert abs(r2[0, 0] - r1[0, 0]) <= 1e-13 * abs(r1[0, 0])
    np.testing.assert_allclose(s2, s1, rtol=1e-13, atol=1e-15)
    for m in range(2):
        np.testing.assert_allclose(post[0, m], w[m], rtol=1e-13)
    np.testing.assert_allclose(r2[0, 1:1 + B], r1[0, 1:1 + B], rtol=1e-9, atol=1e-12 * np.max(np.abs(r1[0, 1:1 + B])))
    g1 = r1[0, 1 + B + 2:]
    for m in range(2):
        gm = r2[0, 1 + B + 4 + m * (R + K):1 + B + 4 + (m + 1) * (R + K)]
        np.testing.assert_allclose(gm, w[m] * g1, rtol=1e-9, atol=1e-11 * np.max(np.abs(g1)))


def test_two_identical_components():
    case1 = kt.small_cases()[2]  # K = 5, S = 7, P = 17, C = 1
    one = kseq.HostKStateLikelihood(case1.masks, case1.weights, case1.peel, case1.rooted, case1.K, 1)
    two = HostKStateMixLikelihood(case1.masks, case1.weights, case1.peel, case1.rooted, case1.K, 2, 1)
    check_two_identical(one, two, case1)


def bad_and_good(case):
    """Five draws: good, a zero frequency in the last component, a negative rate in component 0, a NaN weight,
    good."""
    good = case.params
    R, K, M = case.R, case.K, case.M
    zero_freq = good.copy()
    zero_freq[(M - 1) * (R + K) + R + 2] = 0.0
    neg_rate = good.copy()
    neg_rate[3] = -0.1
    nan_ps = good.copy()
    nan_ps[-1] = np.nan
    return np.stack([good, zero_freq, neg_rate, nan_ps, good]), np.repeat(case.blens[None], 5, 0)


def check_bad_draws(rows, site, post, alone):
    for k in (1, 2, 3):
        assert rows[k, 0] == -np.inf and not rows[k, 1:].any()
        assert np.all(site[k] == -np.inf) and not post[k].any()
    for k in (0, 4):
        for got, want in zip((rows[k], site[k], post[k]), alone):
            np.testing.assert_array_equal(got, want[0])


def test_a_bad_component_refuses_the_draw_alone():
    case = CASES[1]  # K = 5, M = 2, C = 2
    lik = _host(case)
    five, bl5 = bad_and_good(case)
    alone = lik.evaluate_rows(case.blens[None], case.params[None], site_ll=True, class_post=True)
    assert np.isfinite(alone[0]).all()
    check_bad_draws(*lik.evaluate_rows(bl5, five, site_ll=True, class_post=True), alone)


def check_shifted_caterpillar(lik, case):
    sh = mt.shift_counts(case)
    assert np.any(sh.min(axis=0) != sh.max(axis=0))  # shmin differs from a live shift
    ref = mt.load_truth(case, only=("blens", "rs", "ps"))
    assert ref["loglik"] == pytest.approx(-416.66594326217455, rel=1e-12)  # the recorded file
    err, _, _, post = check_against_truth(lik, case)
    assert not mt.bars(err), err
    assert np.all(post[0] > 1e-4)  # both components count at every pattern


def test_shifts_that_differ_between_components():
    case = mt.shifted_caterpillar()
    check_shifted_caterpillar(_host(case), case)


def test_refusals_of_the_host():
    case = CASES[1]
    with pytest.raises(ValueError, match="M \\* C <= 16"):
        HostKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, 3, 6)
    with pytest.raises(ValueError, match="M 1..8"):
        HostKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, 9, 1)
    with pytest.raises(ValueError, match="params must be"):
        _host(case).evaluate_rows(case.blens[None], case.params[None, :-1])
    with pytest.raises(ValueError, match="blens must be"):
        _host(case).evaluate_rows(case.blens[None, :-1], case.params[None])
    rows = _host(case).evaluate_rows(case.blens[None], case.params[None])
    assert isinstance(rows, np.ndarray) and rows.shape[0] == 1
