"""CPU: codon site models (``codon.CodonSitesPosterior``, ``--codon_sites``): the
s_m / sbar map and its transpose against complex step, the posterior's gradient
against central differences of its own ``log_prob`` at the bar
``test_codon_cpu.py`` uses (1e-6), and ``run --codon --codon_sites`` on the host
mixture likelihood: columns, files, refusals."""
import math
import os

import numpy as np
import pytest

from phylostan_amd import cli, codon, stan_io
from phylostan_amd.kseq import HostKStateLikelihood, HostKStateMixLikelihood
from phylostan_amd.posterior import ModelSpec, TreeData
from tests import cases
from tests import test_codon_cpu as tc
from tests.test_posterior import check_grad, preorder_map


def _posterior(seed, sites, model, freqs, C, clock, coalescent=None, S=6, P=12):
    """``test_codon_cpu._posterior`` with a site model: sites drawn from one-nucleotide neighbours."""
    rooted = clock is not None
    peel0 = cases.random_peel(S, np.random.default_rng(seed))
    if not rooted:
        peel0 = cases.make_unrooted(peel0)
    masks, w = tc._codon_data(seed + 1, S, P)
    tree = TreeData(S, peel0, preorder_map(peel0), None, None)
    spec = ModelSpec(model=model, categories=C, invariant=False, clock=clock, estimate_rate=clock is not None,
                     coalescent=coalescent)
    M = codon.parse_site_model(sites)[1]
    lik = HostKStateMixLikelihood(masks, w, peel0, rooted, 61, M, spec.C)
    return codon.CodonSitesPosterior(spec, tree, lik, freqs, sites, counts=codon.codon_counts(masks, w))


def test_parse_site_model():
    assert codon.parse_site_model("M1a") == ("M1a", 2) and codon.parse_site_model("M2a") == ("M2a", 3)
    assert [codon.parse_site_model("M3:%d" % k) for k in (2, 3, 4)] == [("M3", 2), ("M3", 3), ("M3", 4)]
    for bad in ("M3", "M3:1", "M3:5", "M7", "m2a", None):
        with pytest.raises(ValueError, match="codon_sites must be"):
            codon.parse_site_model(bad)


def test_class_scale_and_its_transpose_against_complex_step():
    rng = np.random.default_rng(3)
    n, M = 2, 3
    x6 = rng.uniform(0.5, 3.0, (n, 6))
    om = np.sort(rng.uniform(0.05, 3.0, (n, M)), axis=1)
    rates = np.stack([codon.codon_rates(x6, om[:, m]) for m in range(M)], axis=1)
    pi = rng.dirichlet(np.ones(61) * 3.0, n)
    p = rng.dirichlet(np.ones(M) * 2.0, n)
    ratio = codon.class_scale(rates, pi, p)
    # the mean rate over the classes is one: sum_m p_m s_m / sbar
    assert np.max(np.abs((p * ratio).sum(axis=1) - 1.0)) <= 4e-16
    g = rng.standard_normal((n, M))
    g_rates, g_pi, g_p = codon.class_scale_backward(rates, pi, p, g)
    f = lambda r, q, w: (codon.class_scale(r, q, w) * g).sum(axis=1)  # noqa: E731
    h = 1e-30
    worst = 0.0
    for name, x, got in (("rates", rates, g_rates), ("pi", pi, g_pi), ("p", p, g_p)):
        for _ in range(8):
            d = rng.standard_normal(x.shape)
            z = x + 1j * h * d
            dd = (f(z, pi, p) if name == "rates" else f(rates, z, p) if name == "pi" else f(rates, pi, z)).imag / h
            mine = (got * d).reshape(n, -1).sum(axis=1)
            worst = max(worst, float(np.max(np.abs(mine - dd) / np.maximum(np.abs(dd), 1.0))))
    print("class_scale transpose: %.2e" % worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("sites,model,freqs,C,clock,coalescent", [("M1a", "HKY", "F3x4", 1, "strict", "constant"),
                                                                  ("M2a", "GTR", "F1x4", 1, None, None),
                                                                  ("M3:2", "JC69", "F61", 4, None, None)],
                         ids=["M1a+HKY+F3x4-strict-constant", "M2a+GTR+F1x4-unrooted", "M3:2+JC69+F61+W4"])
def test_codon_sites_posterior_gradient_fd(sites, model, freqs, C, clock, coalescent):
    post = _posterior(21, sites, model, freqs, C, clock, coalescent)
    names = [p.name for p in post.params]
    assert "omega" not in names and "pclass" in names
    assert ("omega2" in names) == (sites == "M2a") and ("omega_delta" in names) == sites.startswith("M3")
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, post.dim)
    if post.param("rate") is not None:
        u[post.param("rate").sl] = math.log(0.3)
    check_grad(post, u, tol=1e-6)
    a = post.log_prob(u[None], propto=False)[0] - post.log_prob(u[None])[0]
    assert abs(a - post.const) < 1e-9


def test_mean_rate_is_one_and_omegas_are_ordered():
    post = _posterior(22, "M3:3", "HKY", "F3x4", 2, None)
    U = np.random.default_rng(1).uniform(-1, 1, (4, post.dim))
    vals, _, _ = post.constrain(U)
    om = post.omegas(vals)
    assert np.all(np.diff(om, axis=1) > 0) and np.all(om > 0)
    mv, positive, sub = post._subst_forward(vals, 4)
    r, q, x6, _, rates, pi, ratio = sub
    assert mv.shape == (4, post.lik.M * (1830 + 61) + 2 * 3 * 2) and positive.all()
    assert np.max(np.abs((vals["pclass"] * ratio).sum(axis=1) - 1.0)) <= 4e-16
    # the engine's effective weights sum to one, and its mean effective rate is the site model's (one)
    M, C = 3, 2
    rs, ps = mv[:, -2 * M * C:-M * C], mv[:, -M * C:]
    assert np.max(np.abs(ps.sum(axis=1) - 1.0)) <= 1e-15


def test_m2a_with_equal_omegas_is_the_single_omega_model():
    """M1a at omega0 -> 1: both classes have omega 1, the mixture is GY94 with omega = 1 whatever pclass is."""
    post = _posterior(23, "M1a", "HKY", "F3x4", 1, None)
    one = tc._posterior(23, "HKY", "F3x4", 1, None)
    u = np.random.default_rng(2).uniform(-0.5, 0.5, post.dim)
    u[post.param("omega0").sl] = 40.0  # omega0 = 1 - 4e-18 -> 1.0
    vals, _, _ = post.constrain(u[None])
    assert vals["omega0"][0] == 1.0
    u1 = np.zeros(one.dim)
    for p in one.params:
        u1[p.sl] = u[post.param(p.name).sl] if p.name != "omega" else 0.0  # omega = e^0 = 1
    rows = post.lik.evaluate_rows(post.blens(u[None]), post.model_vectors(u[None]))
    rows1 = one.lik.evaluate_rows(one.blens(u1[None]), one.model_vectors(u1[None]))
    assert abs(rows[0, 0] - rows1[0, 0]) <= 1e-12 * abs(rows1[0, 0])


def test_columns_summary_and_class_posteriors():
    post = _posterior(24, "M2a", "HKY", "F3x4", 1, "strict", "constant")
    names = post.column_names()
    for nm in ("omega.1", "omega.3", "pclass.1", "pclass.2", "pclass.3", "kappa", "freqs_pos1.1", "heights.5"):
        assert nm in names
    assert "omega.2" not in names and "omega" not in names and "omega0" not in names
    U = np.random.default_rng(1).uniform(-1, 1, (3, post.dim))
    flat = post.flat_rows(U)
    assert flat.shape == (3, len(names))
    assert np.all(flat[:, names.index("omega.1")] < 1.0) and np.all(flat[:, names.index("omega.3")] > 1.0)
    s = post.codon_summary(U)
    assert s["omegas"].shape == (3, 3) and np.all(s["omegas"][:, 1] == 1.0) and s["pclass"].shape == (3, 3)
    cp = post.class_posteriors(U)
    assert cp.shape == (3, 3, 12) and np.max(np.abs(cp.sum(axis=1) - 1.0)) <= 1e-12
    pat = np.asarray([0, 0, 5, 11, 5])
    cls, mean_om, p_pos = codon.site_summary(s["omegas"], cp, pat)
    assert cls.shape == (5, 3) and np.max(np.abs(cls.sum(axis=1) - 1.0)) <= 1e-12
    np.testing.assert_array_equal(cls[0], cls[1])
    np.testing.assert_allclose(p_pos, cls[:, 2], rtol=0, atol=1e-15)  # only omega2 is above 1
    assert np.all(mean_om > 0)
    with pytest.raises(ValueError, match="no draw has a finite likelihood"):
        codon.site_summary(s["omegas"], np.zeros_like(cp), pat)


def test_too_many_classes_times_categories():
    with pytest.raises(ValueError, match="M \\* C <= 16"):  # the likelihood's own refusal comes first
        _posterior(21, "M2a", "HKY", "F3x4", 6, None)
    post = _posterior(21, "M2a", "HKY", "F3x4", 1, None)
    spec6 = ModelSpec(model="HKY", categories=6, invariant=False, clock=None, estimate_rate=False, coalescent=None)
    with pytest.raises(ValueError, match="classes times categories must be <= 16"):
        codon.CodonSitesPosterior(spec6, post.tree, post.lik, "F3x4", "M2a")


# ------------------------------------------------------------------ the CLI
def test_run_codon_sites_vb(tmp_path):
    t, a = tc._dataset(tmp_path)
    out = str(tmp_path / "vb")
    post, lines = tc._run(["-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon", "--codon_sites", "M2a", "-t", t,
                           "-i", a, "-o", out, "-S", "3", "--iter", "30", "--elbo_samples", "5", "--samples", "8"],
                          factory=HostKStateMixLikelihood)
    assert isinstance(post, codon.CodonSitesPosterior) and post.lik.M == 3
    assert any(s == "Codon site model: M2a (3 classes)" for s in lines)
    header, data = stan_io.read_samples(out)
    for nm in ("omega.1", "omega.3", "pclass.1", "pclass.2", "pclass.3", "kappa", "blens.1"):
        assert nm in header
    assert "omega.2" not in header and "omega" not in header
    tsv = [ln.split("\t") for ln in open(out + ".codon.tsv").read().splitlines()]
    assert [r[0] for r in tsv[1:8]] == ["omega.1", "omega.2", "omega.3", "pclass.1", "pclass.2", "pclass.3", "kappa"]
    assert float(tsv[2][1]) == 1.0 and len(tsv) == 1 + 7 + 61
    sites = [ln.split("\t") for ln in open(out + ".codon_sites.tsv").read().splitlines()]
    assert sites[0] == ["codon", "p.1", "p.2", "p.3", "mean_omega", "P(omega>1)"]
    assert len(sites) == 1 + 30 and [r[0] for r in sites[1:]] == [str(k) for k in range(1, 31)]
    for r in sites[1:]:
        assert abs(sum(float(x) for x in r[1:4]) - 1.0) < 1e-4
        assert 0.0 <= float(r[5]) <= 1.0 and abs(float(r[5]) - float(r[3])) < 1e-4 and float(r[4]) > 0.0
    assert os.path.exists(out + ".diag") and os.path.exists(out + ".trees")


def test_run_codon_sites_nuts(tmp_path):
    t, a = tc._dataset(tmp_path)
    out = str(tmp_path / "nuts")
    tc._run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "--codon", "--codon_sites", "M3:2", "--codon_freqs", "F61",
             "-a", "nuts", "-t", t, "-i", a, "-o", out, "-S", "3", "--iter", "6"], factory=HostKStateMixLikelihood)
    header, _ = stan_io.read_samples(out)
    assert "omega.1" in header and "omega.2" in header and "pclass.2" in header
    sites = open(out + ".codon_sites.tsv").read().splitlines()
    assert len(sites) == 31 and sites[0].split("\t")[:3] == ["codon", "p.1", "p.2"]


def test_run_codon_sites_refusals(tmp_path):
    t, a = tc._dataset(tmp_path)
    base = ["-s", str(tmp_path / "x.stan"), "-m", "HKY", "-t", t, "-i", a, "-o", str(tmp_path / "o"), "-S", "3"]
    with pytest.raises(SystemExit, match="--codon_sites needs --codon"):
        tc._run(base + ["--codon_sites", "M2a"], factory=HostKStateMixLikelihood)
    with pytest.raises(SystemExit, match="--codon_sites: codon_sites must be M1a, M2a or M3:k"):
        tc._run(base + ["--codon", "--codon_sites", "M8"], factory=HostKStateMixLikelihood)
    with pytest.raises(SystemExit, match="--codon is not supported with --rescaling"):
        tc._run(base + ["--codon", "--codon_sites", "M2a", "--rescaling"], factory=HostKStateMixLikelihood)
    with pytest.raises(SystemExit, match="classes times categories must be <= 16"):
        tc._run(base + ["--codon", "--codon_sites", "M2a", "-C", "6"], factory=HostKStateMixLikelihood)
    with pytest.raises(SystemExit, match="--codon: this build has no device engine"):
        tc._run(base + ["--codon", "--codon_sites", "M2a"], factory=None)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("o")]  # nothing was written


def test_main_binds_the_mixture_likelihood(monkeypatch):
    from phylostan_amd import kseq
    seen = {}
    monkeypatch.setattr(cli, "run", lambda arg, **kw: seen.update(kw, sites=arg.codon_sites))
    cli.main(["run", "-s", "x.stan", "-m", "HKY", "--codon", "--codon_sites", "M1a", "-t", "t", "-i", "a", "-o", "o"])
    assert seen == {"likelihood_factory": kseq.DeviceKStateMixLikelihood, "sites": "M1a"}
    seen.clear()
    cli.main(["run", "-s", "x.stan", "-m", "HKY", "--codon", "-t", "t", "-i", "a", "-o", "o"])
    assert seen == {"likelihood_factory": kseq.DeviceKStateLikelihood, "sites": None}


def test_a_run_without_codon_sites_is_what_it_was(tmp_path):
    """Fixed seed, no ``--codon_sites``: the sample file's values and OUT.codon.tsv against the values the single
    omega model is recorded to give in tests/golden/codon_sites/plain_vb.json (written before the flag existed)."""
    import json
    t, a = tc._dataset(tmp_path)
    out = str(tmp_path / "vb")
    tc._run(["-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon", "-t", t, "-i", a, "-o", out, "-S", "3", "--iter",
             "30", "--elbo_samples", "5", "--samples", "8"], factory=HostKStateLikelihood)
    want = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "codon_sites",
                                       "plain_vb.json")))
    strip = lambda text: [ln for ln in text.splitlines() if not ln.startswith("#")]  # noqa: E731
    assert strip(open(out).read()) == want["samples"]
    assert open(out + ".codon.tsv").read() == want["codon_tsv"]
    assert not os.path.exists(out + ".codon_sites.tsv")
