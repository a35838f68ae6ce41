"""GPU: the K-state engine's posterior summaries on the device
(``kseq.DeviceKStateSummaries``, ``phy_kseq_sum_*``, ``csrc/kseq_sum.inc``): node
posteriors and labelled substitution counts per branch against the exact
reference of ``tests/kseq_sum_truth.py`` over its shape list, the tied codon case
and the deep caterpillar; log L bit for bit ``phy_kseq_mix_eval``'s; a draw's
outputs bit for bit across batches, contexts, chunks and repeats; the running
sum bit for bit the left-to-right sum of the rows; the plain engine's rows
untouched by a summary context; and ``run --codon --codon_ancestral`` on the
device.  The bars are ``st.bars``: log L 1e-10 relative, node_post 1e-9
absolute, bcounts 1e-9 of the array's largest entry."""
import os

import numpy as np
import pytest

from phylostan_amd.kseq import (DeviceKStateLikelihood, DeviceKStateMixLikelihood, DeviceKStateSummaries,
                                plan_kseq_mix)
from tests import kseq_mix_truth as mt
from tests import kseq_sum_truth as st
from tests import kseq_truth as kt

pytestmark = pytest.mark.gpu

CASES = st.small_cases()


def _device(case, **kw):
    return DeviceKStateSummaries(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C,
                                 case.labels, **kw)


def _check(case):
    ref = st.shared_truth(case)
    dev = _device(case, max_draws=2)
    ll, bc, npost = dev.evaluate(case.blens[None], case.params[None])
    dev.close()
    err = st.compare(case, ll[0], bc[0], npost[0], ref)
    print(case.name, {k: "%.2e" % v for k, v in err.items()})
    assert not st.bars(err), err
    return bc[0], npost[0]


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_against_the_truth(case):
    bc, npost = _check(case)
    zero = np.flatnonzero(case.blens == 0.0)
    assert not bc[:, zero].any()  # a zero-length branch: exactly 0
    w0 = np.flatnonzero(case.weights == 0.0)
    if w0.size:  # a zero-weight column keeps its posterior
        np.testing.assert_allclose(npost[:, :, w0].sum(axis=1), 1.0, rtol=0, atol=st.SUM_BAR)
    if not case.rooted:  # the root and the merged child: the same point
        np.testing.assert_allclose(npost[case.S - 2], npost[case.S - 3], rtol=0, atol=1e-13)


def test_tied_codon_case():
    _check(st.tied_codon())


def test_deep_caterpillar_with_many_shifts():
    case = st.deep_caterpillar()
    shifts = mt.shift_counts(case.mix)
    assert shifts[1, 1:].min() >= 2 * 64  # the live category is rescaled more than once at the varying patterns
    _check(case)


def _five(case):
    """Draw 0 and 4 the case's own; 1 and 3 refused (a negative frequency, a non-finite branch); 2 another."""
    bl = np.repeat(case.blens[None], 5, 0)
    pr = np.repeat(case.params[None], 5, 0)
    bl[2] *= 0.7
    pr[1, case.R + 1] = -1.0
    bl[3, 1] = np.inf
    return bl, pr


def test_loglik_is_the_mixture_engines_bit_for_bit():
    case = CASES[3]  # K = 17, M = 2, C = 4
    bl, pr = _five(case)
    mix = DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C,
                                    max_draws=5)
    rows = mix.evaluate_rows(bl, pr)
    mix.close()
    dev = _device(case, max_draws=5)
    ll, bc, npost = dev.evaluate(bl, pr)
    dev.close()
    np.testing.assert_array_equal(ll, rows[:, 0])
    assert np.isfinite(ll[[0, 2, 4]]).all() and np.all(ll[[1, 3]] == -np.inf)
    assert not bc[[1, 3]].any() and not npost[[1, 3]].any()


def test_bits_across_batches_contexts_and_repeats():
    case = CASES[1]  # K = 5, C = 4 with rs_0 = 0, two labels
    bl, pr = _five(case)
    wide = _device(case, max_draws=8)
    alone = wide.evaluate(case.blens[None], case.params[None])
    batch = wide.evaluate(bl, pr)
    again = wide.evaluate(bl, pr)
    no_post = wide.evaluate(bl, pr, node_post=False)
    wide.close()
    narrow = _device(case, max_draws=2)  # three calls of the library, the last a short one
    split = narrow.evaluate(bl, pr)
    narrow.close()
    for a, b, c, one in zip(batch, again, split, alone):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(a[0], one[0])  # first
        np.testing.assert_array_equal(a[4], one[0])  # and last of five, refused draws between
    for a, b in zip(batch[:2], no_post):
        np.testing.assert_array_equal(a, b)


def test_bits_across_chunks_of_one_call():
    # S = 400 at K = 17, M = 2: 9.8 MB of workspace an item, two items a draw: 70 draws run in two chunks
    rng = np.random.default_rng(5)
    S, K, P, M, C = 400, 17, 1, 2, 1
    masks = kt.random_masks(S, P, K, rng, unknown_column=False)
    peel = kt.caterpillar_peel(S)
    plan = plan_kseq_mix(masks, np.ones(P), peel, False, K, M, C, max_draws=70)
    assert 1 <= plan["chunk_draws"] < 69
    dev = DeviceKStateSummaries(masks, np.ones(P), peel, False, K, M, C, st.dense_labels(K, 2, 9), max_draws=70)
    base = mt.random_mix("x", 3, K, 1, M, C, False, 3)
    params = np.repeat(base.params[None], 70, 0)
    blens = np.repeat(rng.exponential(0.05, 2 * S - 3)[None], 70, 0)
    blens[1:69] *= rng.uniform(0.5, 1.5, (68, 1))
    got = dev.evaluate(blens, params)
    one = dev.evaluate(blens[:1], params[:1])
    dev.reset()
    dev.add(blens, params)
    total, nf = dev.read()
    dev.close()
    assert np.isfinite(got[0]).all() and nf == 70
    for g, w in zip(got, one):
        np.testing.assert_array_equal(g[0], w[0])
        np.testing.assert_array_equal(g[69], w[0])  # the same draw, in the second chunk
    np.testing.assert_allclose(got[2].sum(axis=2), 1.0, rtol=0, atol=st.SUM_BAR)
    want = np.zeros_like(total)
    for d in range(70):
        want = want + got[2][d]
    np.testing.assert_array_equal(total, want)


def test_running_sum_is_the_left_to_right_sum_of_the_rows():
    case = CASES[3]
    bl, pr = _five(case)
    pr[3], bl[3] = case.params, 1.3 * case.blens  # one refused draw (1) among five
    dev = _device(case, max_draws=5)
    ll, bc, npost = dev.evaluate(bl, pr)
    want = np.zeros_like(npost[0])
    for d in range(5):
        if np.isfinite(ll[d]):
            want = want + npost[d]
    for split in ((1, 4), (5,), (2, 2, 1)):
        dev.reset()
        at = 0
        for n in split:
            l2, b2 = dev.add(bl[at:at + n], pr[at:at + n])
            np.testing.assert_array_equal(l2, ll[at:at + n])
            np.testing.assert_array_equal(b2, bc[at:at + n])
            at += n
        total, nf = dev.read()
        assert nf == 4 and ll[1] == -np.inf
        np.testing.assert_array_equal(total, want)
    dev.reset()
    total, nf = dev.read()
    dev.close()
    assert nf == 0 and not total.any()


def test_plain_rows_before_and_after_a_summary_context():
    case = kt.small_cases()[9]  # K = 61, C = 4, the codon structure
    bl = np.stack([case.blens, 0.5 * case.blens])
    pr = np.stack([case.params, case.params])
    args = (case.masks, case.weights, case.peel, case.rooted, case.K, case.C)
    one = DeviceKStateLikelihood(*args, max_draws=2)
    before = one.evaluate_rows(bl, pr, site_ll=True)
    one.close()
    sc = CASES[6]
    dev = _device(sc, max_draws=1)
    dev.evaluate(sc.blens[None], sc.params[None])
    two = DeviceKStateLikelihood(*args, max_draws=2)
    after = two.evaluate_rows(bl, pr, site_ll=True)
    dev.close()
    two.close()
    assert np.isfinite(before[0]).all()
    for a, b in zip(before, after):
        np.testing.assert_array_equal(a, b)


def test_run_codon_ancestral_on_the_device(tmp_path):
    from tests import test_kseq_sum_cpu as tc
    out = tc.run_codon_ancestral(tmp_path, ["-a", "vb", "-S", "3"], device=True)
    tc.check_outputs(out)
    assert os.path.exists(out["stem"] + ".ancestral.fasta")
