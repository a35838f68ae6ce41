"""GPU: the mixture of M K-state models over sites on the device
(``kseq.DeviceKStateMixLikelihood``, ``phy_kseq_mix_*``: the kernels of
``csrc/kseq_engine.inc`` with the component index) against the exact reference
of ``tests/kseq_mix_truth.py`` over its shape list and the recorded shifted
caterpillar, bit for bit against ``phy_kseq_eval`` at M = 1, bit for bit across
batches, chunks and repeats, under ``CodonSitesPosterior`` and from the command
line.  The bars are ``mt.bars``: log L and site log L 1e-10 relative, each
gradient array 1e-9 of its largest entry, class posteriors 1e-9 absolute, their
sum 1 to 1e-12."""
import os
import subprocess
import sys

import numpy as np
import pytest

from phylostan_amd import codon, stan_io
from phylostan_amd.kseq import (DeviceKStateLikelihood, DeviceKStateMixLikelihood, HostKStateMixLikelihood,
                                mix_row_len)
from tests import kseq_mix_truth as mt
from tests import kseq_truth as kt
from tests import test_kseq_mix_cpu as tm

pytestmark = pytest.mark.gpu

CASES = mt.small_cases()
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _device(case, **kw):
    return DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C, **kw)


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_against_the_truth(case):
    lik = _device(case, max_draws=2)
    err, _, _, post = tm.check_against_truth(lik, case)
    lik.close()
    assert not mt.bars(err), err
    if case.name.endswith("dead1"):
        assert not post[0, 1].any() and np.all(post[0, 0] > 0)


def test_shifts_that_differ_between_components():
    case = mt.shifted_caterpillar()
    lik = _device(case, max_draws=1)
    tm.check_shifted_caterpillar(lik, case)
    lik.close()


@pytest.mark.parametrize("at", [1, 4, 9], ids=["K4_C4_inv", "K17_C4", "K61_C4_codon"])
def test_one_component_is_phy_kseq_eval_bit_for_bit(at):
    case = kt.small_cases()[at]
    bl = np.stack([case.blens, 0.5 * case.blens, case.blens])
    pr = np.stack([case.params, case.params, case.params])
    pr[2, case.R + 1] = -1.0  # a refused draw
    one = DeviceKStateLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.C, max_draws=3)
    rows, site = one.evaluate_rows(bl, pr, site_ll=True)
    one.close()
    mix = DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, 1, case.C, max_draws=3)
    mrows, msite, post = mix.evaluate_rows(bl, pr, site_ll=True, class_post=True)
    mix.close()
    assert np.isfinite(rows[:2]).all() and rows[2, 0] == -np.inf
    np.testing.assert_array_equal(mrows, rows)
    np.testing.assert_array_equal(msite, site)
    assert np.max(np.abs(post[:2] - 1.0)) <= 1e-15 and not post[2].any()


def test_two_identical_components():
    case1 = kt.small_cases()[2]  # K = 5, S = 7, P = 17, C = 1
    one = DeviceKStateLikelihood(case1.masks, case1.weights, case1.peel, case1.rooted, case1.K, 1, max_draws=1)
    two = DeviceKStateMixLikelihood(case1.masks, case1.weights, case1.peel, case1.rooted, case1.K, 2, 1, max_draws=1)
    tm.check_two_identical(one, two, case1)
    one.close()
    two.close()


def test_bits_across_batches_and_repeats():
    case = CASES[1]  # K = 5, M = 2, C = 2, P = 15
    five, bl5 = tm.bad_and_good(case)
    wide = _device(case, max_draws=8)
    alone = wide.evaluate_rows(case.blens[None], case.params[None], site_ll=True, class_post=True)
    batch = wide.evaluate_rows(bl5, five, site_ll=True, class_post=True)
    again = wide.evaluate_rows(bl5, five, site_ll=True, class_post=True)
    wide.close()
    narrow = _device(case, max_draws=2)  # three calls of the library, the last a short one
    split = narrow.evaluate_rows(bl5, five, site_ll=True, class_post=True)
    narrow.close()
    assert all(np.isfinite(x).all() for x in alone)
    tm.check_bad_draws(*batch, alone)
    for a, b, c in zip(batch, again, split):
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a, c)


def test_bits_across_chunks_of_one_call():
    # S = 400 at K = 17, M = 2: 9.8 MB of workspace an item, two items a draw: 70 draws run in two chunks
    rng = np.random.default_rng(5)
    S, K, P, M, C = 400, 17, 1, 2, 1
    masks = kt.random_masks(S, P, K, rng, unknown_column=False)
    lik = DeviceKStateMixLikelihood(masks, np.ones(P), kt.caterpillar_peel(S), False, K, M, C, max_draws=70)
    info = lik.info()
    assert 1 <= info["chunk_draws"] < 69 and info["items_per_draw"] == 2
    base = mt.random_mix("x", 3, K, 1, M, C, False, 3)
    params = np.repeat(base.params[None], 70, 0)
    blens = np.repeat(rng.exponential(0.05, 2 * S - 3)[None], 70, 0)
    blens[1:69] *= rng.uniform(0.5, 1.5, (68, 1))
    rows, site, post = lik.evaluate_rows(blens, params, site_ll=True, class_post=True)
    one = lik.evaluate_rows(blens[:1], params[:1], site_ll=True, class_post=True)
    sweeps = lik.info(1)["sweeps"]
    lik.close()
    assert np.isfinite(rows).all() and len(sweeps) == 1 and len(sweeps[0]) == M and min(sweeps[0]) > 0
    for got, want in zip((rows, site, post), one):
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[69], want[0])  # the same draw, in the second chunk
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=0, atol=1e-12)


def test_class_post_is_optional_and_changes_nothing():
    case = CASES[2]
    lik = _device(case, max_draws=1)
    rows = lik.evaluate_rows(case.blens[None], case.params[None])
    rows2, post = lik.evaluate_rows(case.blens[None], case.params[None], class_post=True)
    lik.close()
    np.testing.assert_array_equal(rows, rows2)
    assert rows.shape == (1, mix_row_len(case.B, case.K, case.M, case.C)) and post.shape == (1, case.M, case.P)


def test_codon_sites_posterior_on_the_device():
    from tests import test_codon_sites_cpu as ts
    host = ts._posterior(21, "M2a", "HKY", "F3x4", 1, "strict", "constant", S=7, P=20)
    hl = host.lik
    assert isinstance(hl, HostKStateMixLikelihood) and hl.masks.shape == (7, 20) and hl.M == 3
    dev = DeviceKStateMixLikelihood(hl.masks, hl.weights, hl.peel, hl.rooted, 61, hl.M, hl.C, max_draws=2)
    post = codon.CodonSitesPosterior(host.spec, host.tree, dev, "F3x4", "M2a",
                                     counts=codon.codon_counts(hl.masks, hl.weights))
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (3, host.dim))
    if host.param("rate") is not None:
        U[:, host.param("rate").sl] = np.log(0.3)
    lp_h, g_h = host.log_prob_grad(U)
    lp_d, g_d = post.log_prob_grad(U)
    cp_h = host.class_posteriors(U)
    cp_d = post.class_posteriors(U)
    dev.close()
    print("sites posterior: lp %.2e grad %.2e class %.2e" % (np.max(np.abs(lp_d - lp_h) / np.abs(lp_h)),
                                                             np.max(np.abs(g_d - g_h)) / np.max(np.abs(g_h)),
                                                             np.max(np.abs(cp_d - cp_h))))
    assert np.all(np.abs(lp_d - lp_h) <= 1e-10 * np.abs(lp_h))
    for k in range(3):
        assert np.max(np.abs(g_d[k] - g_h[k])) <= 1e-9 * np.max(np.abs(g_h[k]))
    assert np.max(np.abs(cp_d - cp_h)) <= 1e-9
    assert dev.calls > 0


def test_main_runs_codon_sites_on_the_device(tmp_path):
    """``python -m phylostan_amd run --codon --codon_sites M2a`` in a fresh child process under its own time limit."""
    from tests import test_codon_cpu as tc
    t, a = tc._dataset(tmp_path)
    out = str(tmp_path / "vb")
    cmd = [sys.executable, "-m", "phylostan_amd", "run", "-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon",
           "--codon_sites", "M2a", "-t", t, "-i", a, "-o", out, "-S", "3", "--iter", "30", "--elbo_samples", "5",
           "--samples", "8"]
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert run.returncode == 0, (run.stdout + run.stderr)[-3000:]
    header, data = stan_io.read_samples(out)
    for nm in ("omega.1", "omega.3", "pclass.1", "pclass.3", "kappa", "blens.1"):
        assert nm in header
    assert "omega.2" not in header  # fixed at 1
    assert data.shape[1] == len(header) and np.all(data[1:, header.index("omega.3")] > 1.0)
    tsv = [ln.split("\t") for ln in open(out + ".codon_sites.tsv").read().splitlines()]
    ncodon = len(tsv) - 1
    assert tsv[0][:4] == ["codon", "p.1", "p.2", "p.3"] and ncodon >= 1
    for r in tsv[1:]:
        assert abs(sum(float(x) for x in r[1:4]) - 1.0) < 1e-4
    assert os.path.exists(out + ".codon.tsv") and os.path.exists(out + ".diag")
