"""GPU: the K-state sequence likelihood engine (``kseq.DeviceKStateLikelihood``,
``csrc/kseq_engine.inc``) against the exact reference of ``tests/kseq_truth.py``
over the shape list, against the recorded 400-tip caterpillar, against the
4-state oracle at K = 4, bit for bit across batches, chunks and repeats, under
``CodonPosterior`` and from the command line.  The bars are the project's
(``kt.bars``): log L and site log L 1e-10 relative, each gradient array 1e-9 of
its largest entry, the K = 2 rate and all-unknown columns absolute."""
import os

import numpy as np
import pytest

from phylostan_amd import codon, models, stan_io
from phylostan_amd.kseq import DeviceKStateLikelihood, HostKStateLikelihood, kseq_host, onehot_masks, row_len
from tests import cases, kseq_truth as kt

pytestmark = pytest.mark.gpu

CASES = kt.small_cases()


def _device(case, **kw):
    return DeviceKStateLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.C, **kw)


def _host_minus_device(case, rows, site):
    hrows, hsite = kseq_host(case.masks, case.weights, case.peel, case.rooted, case.blens[None], case.params[None],
                             case.C)
    with np.errstate(invalid="ignore"):
        return {"row": float(np.max(np.abs(rows - hrows)) / max(np.max(np.abs(hrows)), 1e-300)),
                "site": float(np.max(np.abs(site - hsite)))}


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_device_against_the_truth(case):
    lik = _device(case, max_draws=2)
    rows, site = lik.evaluate_rows(case.blens[None], case.params[None], site_ll=True)
    lik.close()
    assert rows.shape == (1, row_len(case.B, case.K, case.C)) and site.shape == (1, case.P)
    ref = kt.load_truth(case)
    err = kt.compare(case, rows[0], site[0], ref)
    print(case.name, {k: "%.2e" % v for k, v in err.items()}, "device - host",
          {k: "%.2e" % v for k, v in _host_minus_device(case, rows, site).items()})
    assert not kt.bars(err), err
    if case.through:  # codon cases: kappa and omega through codon_rates' Jacobian transpose
        g = case.split_row(rows[0])["rates"]
        kappa, omega = case.through["kappa"][0], case.through["omega"][0]
        g_x6, g_om = codon.codon_rates_backward(np.asarray([1.0, kappa, 1.0, 1.0, kappa, 1.0]), omega, g)
        scale = max(abs(ref["through_kappa"]), abs(ref["through_omega"]))
        assert abs(g_x6[1] + g_x6[4] - ref["through_kappa"]) <= 1e-9 * scale
        assert abs(g_om - ref["through_omega"]) <= 1e-9 * scale


def test_rescaling_on_a_400_tip_caterpillar():
    case = kt.caterpillar400()
    ref = kt.load_truth(case, only=("blens",))
    lik = _device(case, max_draws=1)
    rows = lik.evaluate_rows(case.blens[None], case.params[None])
    lik.close()
    assert ref["loglik"] < -1500.0
    got = case.split_row(rows[0])
    print("caterpillar400 loglik", got["loglik"], ref["loglik"],
          "blens %.2e" % (np.max(np.abs(got["blens"] - ref["blens"])) / np.max(np.abs(ref["blens"]))))
    assert abs(got["loglik"] - ref["loglik"]) <= 1e-10 * abs(ref["loglik"])
    assert np.max(np.abs(got["blens"] - ref["blens"])) <= 1e-9 * np.max(np.abs(ref["blens"]))


def _against_oracle(case):
    ref = case.oracle()
    gr, gf = models.q_param_gradients(ref["dLdP"], case.blens, case.rs, case.freqs, case.rates, ref["grad_freq_root"])
    params = np.concatenate([case.rates, case.freqs, case.rs, case.ps])
    masks = np.asarray(case.tipcodes, np.uint64)  # A=1 C=2 G=4 T=8: states 0..3 in the oracle's order
    lik = DeviceKStateLikelihood(masks, case.weights, case.peel0, case.rooted, 4, case.C, max_draws=1)
    rows, site = lik.evaluate_rows(case.blens[None], params[None], site_ll=True)
    lik.close()
    B, C = case.blens.size, case.C
    row = rows[0]
    unk = np.all(np.asarray(case.tipcodes) == 15, axis=0)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))  # noqa: E731
    err = {"loglik": abs(row[0] - ref["loglik"]) / abs(ref["loglik"]),
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


def test_bits_across_batches_chunks_and_repeats():
    case = CASES[4]  # K = 17: a tile plus one state; P = 17: a tile plus one pattern; C = 4, unrooted
    good = case.params
    R = case.R
    zero_freq = good.copy()
    zero_freq[R + 2] = 0.0
    neg_rate = good.copy()
    neg_rate[3] = -0.1
    nan_ps = good.copy()
    nan_ps[-1] = np.nan
    five = np.stack([good, zero_freq, neg_rate, nan_ps, good])
    bl5 = np.repeat(case.blens[None], 5, 0)
    wide = _device(case, max_draws=8)
    alone, alone_site = wide.evaluate_rows(case.blens[None], good[None], site_ll=True)
    batch, site = wide.evaluate_rows(bl5, five, site_ll=True)
    again, again_site = wide.evaluate_rows(bl5, five, site_ll=True)
    wide.close()
    narrow = _device(case, max_draws=2)  # three calls of the library, the last a short one
    split, split_site = narrow.evaluate_rows(bl5, five, site_ll=True)
    narrow.close()
    assert np.isfinite(alone).all() and np.isfinite(alone_site).all()
    for k in (1, 2, 3):
        assert batch[k, 0] == -np.inf and not batch[k, 1:].any() and np.all(site[k] == -np.inf)
    for k in (0, 4):
        np.testing.assert_array_equal(batch[k], alone[0])
        np.testing.assert_array_equal(site[k], alone_site[0])
    np.testing.assert_array_equal(again, batch)
    np.testing.assert_array_equal(again_site, site)
    np.testing.assert_array_equal(split, batch)
    np.testing.assert_array_equal(split_site, site)


def test_bits_across_chunks_of_one_call():
    # S = 400 at K = 64: 19.7 MB of workspace an item, so a call of 70 draws runs in two chunks (54 and 16)
    rng = np.random.default_rng(5)
    S, K, P, C = 400, 64, 1, 1
    peel = kt.caterpillar_peel(S)
    masks = kt.random_masks(S, P, K, rng, unknown_column=False)
    lik = DeviceKStateLikelihood(masks, np.ones(P), peel, False, K, C, max_draws=70)
    info = lik.info()
    assert 1 <= info["chunk_draws"] < 69
    base = kt.random_case("x", 3, K, 1, 1, False, 3)
    params = np.repeat(base.params[None], 70, 0)
    blens = np.repeat(rng.exponential(0.05, 2 * S - 3)[None], 70, 0)
    blens[1:69] *= rng.uniform(0.5, 1.5, (68, 1))
    rows, site = lik.evaluate_rows(blens, params, site_ll=True)
    one, one_site = lik.evaluate_rows(blens[:1], params[:1], site_ll=True)
    lik.close()
    assert np.isfinite(rows).all()
    np.testing.assert_array_equal(rows[0], one[0])
    np.testing.assert_array_equal(rows[69], one[0])  # the same draw, in the second chunk
    np.testing.assert_array_equal(site[69], one_site[0])


def test_zero_likelihood_pattern_is_a_bad_draw():
    masks = onehot_masks(np.asarray([[0], [1], [0]]))
    peel = np.asarray([[0, 1, 3], [2, 3, 4]], np.int32)
    params = np.concatenate([[1.0], [0.5, 0.5], [1.0], [1.0]])
    lik = DeviceKStateLikelihood(masks, np.ones(1), peel, False, 2, 1, max_draws=1)
    rows, site = lik.evaluate_rows(np.zeros((1, 3)), params[None], site_ll=True)
    lik.close()
    assert rows[0, 0] == -np.inf and not rows[0, 1:].any() and site[0, 0] == -np.inf


def test_all_unknown_column_and_invariant_category():
    case = CASES[1]  # K = 4, C = 4, rs[0] = 0, the last column all unknown
    assert case.args["rs"][0] == 0.0
    lik = _device(case, max_draws=1)
    _, site = lik.evaluate_rows(case.blens[None], case.params[None], site_ll=True)
    lik.close()
    assert abs(site[0, -1]) < 1e-14  # L_i = 1


def test_codon_posterior_on_the_device():
    from tests import test_codon_cpu as tc
    host = tc._posterior(21, "HKY", "F3x4", 4, "strict", "constant", S=6, P=30)
    hl = host.lik
    assert isinstance(hl, HostKStateLikelihood) and hl.masks.shape == (6, 30)
    dev = DeviceKStateLikelihood(hl.masks, hl.weights, hl.peel, hl.rooted, 61, hl.C, max_draws=2)
    post = codon.CodonPosterior(host.spec, host.tree, dev, "F3x4", counts=codon.codon_counts(hl.masks, hl.weights))
    U = np.random.default_rng(5).uniform(-1.0, 1.0, (3, host.dim))
    if host.param("rate") is not None:
        U[:, host.param("rate").sl] = np.log(0.3)
    lp_h, g_h = host.log_prob_grad(U)
    lp_d, g_d = post.log_prob_grad(U)
    dev.close()
    print("posterior: lp %.2e grad %.2e" % (np.max(np.abs(lp_d - lp_h) / np.abs(lp_h)),
                                            np.max(np.abs(g_d - g_h)) / np.max(np.abs(g_h))))
    assert np.all(np.abs(lp_d - lp_h) <= 1e-10 * np.abs(lp_h))
    for k in range(3):
        assert np.max(np.abs(g_d[k] - g_h[k])) <= 1e-9 * np.max(np.abs(g_h[k]))
    assert dev.calls > 0


def test_main_runs_codon_on_the_device(tmp_path):
    from phylostan_amd import cli
    from tests import test_codon_cpu as tc
    t, a = tc._dataset(tmp_path)
    out = str(tmp_path / "vb")
    cli.main(["run", "-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon", "-t", t, "-i", a, "-o", out, "-S", "3",
              "--iter", "30", "--elbo_samples", "5", "--samples", "8"])
    header, data = stan_io.read_samples(out)
    for nm in ("omega", "kappa", "freqs_pos1.1", "blens.1"):
        assert nm in header
    assert data.shape == (9, len(header)) and np.all(data[:, header.index("omega")] > 0)
    tsv = [ln.split("\t") for ln in open(out + ".codon.tsv").read().splitlines()]
    assert tsv[0] == ["parameter", "mean", "2.5%", "97.5%"]
    assert [r[0] for r in tsv[1:3]] == ["omega", "kappa"] and len(tsv) == 1 + 2 + 61
    assert abs(sum(float(r[1]) for r in tsv[3:]) - 1.0) < 1e-4
    assert os.path.exists(out + ".diag")
