"""CPU: the trait clock rate of phylogeography (``P_b = exp(Q mu t_b)``): the
host restatements with ``clock=`` against the truth of tests/geo_clock_truth.py
(the existing expm truths at ``mu * blens``, d/dmu by the complex step on mu),
the posterior classes with an estimated and a fixed clock on host likelihood
doubles, the default prior, the command line, and a recovery check: data
simulated at a known mu Q on a tree whose time unit is then changed.

Bars (the project's): log L at relative 1e-10, each gradient array within 1e-9
of its largest entry, d/dmu at 1e-9 of max(|truth|, the size of the terms that
cancel in it) (tests/geo_clock_truth.py).
"""
import json
import math
import os

import numpy as np
import pytest

from phylostan_amd import cli, geo, stan_io
from tests import geo_clock_truth as gc
from tests import geo_oracle as go
from tests import geo_trees_truth as gt
from tests.test_geo_trees_cpu import write_dataset

CASES = gc.truth_cases()


# ---------------------------------------------------------------- the host restatements
@pytest.mark.parametrize("name", sorted(CASES))
def test_host_restatement_with_a_clock_against_the_truth(name):
    tips, peels, blens, params, logw, mus, extended, entries = CASES[name]
    for mu in mus:
        row, tll = gc.host_clock_row(tips, peels, blens, params, logw, mu)
        gc.check_clock_row(row, tll, tips, peels, blens, params, logw, mu, entries=entries, extended=extended)


def test_host_single_tree_with_a_clock():
    tips, peels, blens, params, logw, _, _, _ = CASES["mixed"]
    R, mu = geo.rate_count(5), 0.2
    ll, gb, gr, gf, gm = geo.geo_gradients_host(tips, peels[2], blens[2], params[:R], params[R:], clock=mu)
    tl, tg = go.truth_gradients(tips, peels[2], mu * blens[2], params[:R], params[R:])
    assert abs(ll - tl) <= gc.LL_BAR * abs(tl)
    want_gb = mu * tg["blens"][1]  # with respect to the tree's own lengths
    assert np.abs(gb - want_gb).max() <= gc.GRAD_BAR * np.abs(want_gb).max()
    want = go.truth(tips, peels[2], blens[2] * complex(mu, gc.STEP), params[:R], params[R:]).imag / gc.STEP
    assert abs(gm - want) <= gc.dmu_bar(want, min(1.0, mu) * np.abs(blens[2] * tg["blens"][1]).sum())
    # the summaries: those of the rescaled tree, the dwell times back in the tree's unit
    marg, jumps, bj = geo.geo_summaries_host(tips, peels[2], blens[2], params[:R], params[R:], clock=mu)
    m0, j0, b0 = geo.geo_summaries_host(tips, peels[2], mu * blens[2], params[:R], params[R:])
    off = ~np.eye(5, dtype=bool)
    assert np.array_equal(marg, m0) and np.array_equal(bj, b0) and np.array_equal(jumps[off], j0[off])
    assert np.array_equal(np.diag(jumps), np.diag(j0) / mu)
    assert abs(np.trace(jumps) - blens[2].sum()) <= 1e-9 * blens[2].sum()


def test_without_a_clock_the_host_restatements_are_unchanged():
    tips, peels, blens, params, logw, _, _, _ = CASES["mixed"]
    R = geo.rate_count(5)
    r, f = params[:R], params[R:]
    for a, b in zip(geo.geo_gradients_host(tips, peels[0], blens[0], r, f, clock=None),
                    geo.geo_gradients_host(tips, peels[0], blens[0], r, f)):
        assert np.array_equal(a, b)
    assert len(geo.geo_gradients_host(tips, peels[0], blens[0], r, f, clock=None)) == 4
    for a, b in zip(geo.geo_summaries_host(tips, peels[0], blens[0], r, f, clock=None),
                    geo.geo_summaries_host(tips, peels[0], blens[0], r, f)):
        assert np.array_equal(a, b)
    plain = geo.geo_trees_host(tips, peels, blens, r, f, logw)
    same = geo.geo_trees_host(tips, peels, blens, r, f, logw, clock=None)
    assert len(plain) == len(same) == 4 and all(np.array_equal(a, b) for a, b in zip(plain, same))
    for a, b in zip(geo.geo_trees_summaries_host(tips, peels, blens, r, f, logw, clock=None),
                    geo.geo_trees_summaries_host(tips, peels, blens, r, f, logw)):
        assert np.array_equal(a, b)
    # mu = 1 is the plain model
    one = geo.geo_trees_host(tips, peels, blens, r, f, logw, clock=1.0)
    assert all(np.array_equal(a, b) for a, b in zip(plain, one[:4]))


@pytest.mark.parametrize("mu", [0.0, -1.0, np.nan, np.inf])
def test_a_bad_rate_on_the_host(mu):
    tips, peels, blens, params, logw, _, _, _ = CASES["mixed"]
    R = geo.rate_count(5)
    ll, gr, gf, tll, gm = geo.geo_trees_host(tips, peels, blens, params[:R], params[R:], logw, clock=mu)
    assert ll == -np.inf and not gr.any() and not gf.any() and np.all(tll == -np.inf) and gm == 0.0
    jumps, root = geo.geo_trees_summaries_host(tips, peels, blens, params[:R], params[R:], logw, clock=mu)
    assert not jumps.any() and not root.any()
    assert geo.geo_gradients_host(tips, peels[0], blens[0], params[:R], params[R:], clock=mu)[0] == -np.inf


# ---------------------------------------------------------------- the posterior classes
def posteriors(clock, clock_prior=None):
    tips, peels, blens, _, logw, _, _, _ = CASES["mixed"]
    one = geo.GeoPosterior(5, blens[2], gc.HostGeoClockLikelihood(tips, peels[2]), clock=clock, clock_prior=clock_prior)
    lik = gc.HostGeoTreesClockLikelihood(tips, peels[:3], blens[:3], log_weights=logw[:3])
    return one, geo.GeoTreesPosterior(5, lik, clock=clock, clock_prior=clock_prior)


@pytest.mark.parametrize("which", [0, 1])
def test_posterior_with_an_estimated_clock(which):
    post = posteriors("estimate")[which]
    K, R = 5, 10
    assert post.dim == R + K - 1 + 1 and post.clock_estimated
    names = post.column_names()
    assert names[-2:] == ["freqs_geo.5", "rate_geo"] and len(names) == R + K + 1
    rng = np.random.default_rng(3 + which)
    U = rng.normal(0.0, 0.7, (3, post.dim))
    flat = post.flat_rows(U)
    assert flat.shape == (3, R + K + 1) and np.array_equal(flat[:, -1], np.exp(U[:, -1]))
    assert np.array_equal(post.constrain(U)[3][2], np.exp(U[:, -1]))
    lp, G = post.log_prob_grad(U)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(G))
    h = 1e-5
    for k in range(post.dim):
        e = np.zeros(post.dim)
        e[k] = h
        fd = (post.log_prob(U + e) - post.log_prob(U - e)) / (2 * h)
        assert np.all(np.abs(fd - G[:, k]) <= 1e-6 * np.maximum(1.0, np.abs(G).max(1))), k
    a, b = post.clock_prior
    full = post.log_prob(U, propto=False)
    assert np.allclose(full - lp, a * math.log(b) - math.lgamma(a) + math.lgamma(K), rtol=0, atol=1e-12)
    # a fixed clock: no coordinate, no column, the estimated posterior's likelihood part at that mu
    fixed = posteriors(0.5)[which]
    assert fixed.dim == R + K - 1 and "rate_geo" not in fixed.column_names() and fixed.flat_rows(U[:, :-1]).shape[1] == R + K
    V = U.copy()
    V[:, -1] = math.log(0.5)
    lpe, Ge = post.log_prob_grad(V)
    lpf, Gf = fixed.log_prob_grad(V[:, :-1])
    prior = a * math.log(0.5) - b * 0.5
    assert np.all(np.abs(lpe - prior - lpf) <= 1e-12 * np.abs(lpf)) and np.abs(Ge[:, :-1] - Gf).max() <= 1e-12 * np.abs(Gf).max()


@pytest.mark.parametrize("which", [0, 1])
def test_posterior_without_a_clock_calls_as_before(which):
    post = posteriors(None)[which]
    assert not post.has_clock and post.dim == 10 + 4
    tips, peels, blens, _, logw, _, _, _ = CASES["mixed"]
    U = np.random.default_rng(9).normal(0.0, 0.7, (2, post.dim))
    lp, G = post.log_prob_grad(U)
    rates, freqs, logj, (st_r, st_f) = post.constrain(U)
    params = np.concatenate([rates, freqs], axis=1)
    if which == 0:
        rows = go.HostGeoLikelihood(tips, peels[2]).evaluate_rows(np.tile(blens[2], (2, 1)), params)
        B = blens[2].size
        assert post.lik.clock_calls == 0
    else:
        rows = gt.HostGeoTreesLikelihood(tips, peels[:3], blens[:3], log_weights=logw[:3]).evaluate_rows(params)
        B = 0
    want = np.concatenate([post.t_rates.backward(st_r, rows[:, 1 + B:1 + B + 10], 1.0),
                           post.t_freqs.backward(st_f, rows[:, 1 + B + 10:], 1.0)], axis=1)
    assert np.array_equal(lp, rows[:, 0] + logj) and np.array_equal(G, want)
    assert post.column_names()[-1] == "freqs_geo.5"


def test_default_prior_and_its_refusals():
    tips, peels, blens, _, logw, _, _, _ = CASES["mixed"]
    one, many = posteriors("estimate")
    assert one.clock_prior == (0.5, float(blens[2].sum()))
    w = np.exp(logw[:3])
    assert len(set(w.tolist())) == 3  # unequal weights
    assert many.clock_prior[0] == 0.5
    assert abs(many.clock_prior[1] - np.dot(w, blens[:3].sum(1)) / w.sum()) <= 1e-14 * blens[:3].sum()
    assert geo.mean_tree_length(blens[:3]) == blens[:3].sum(1).mean()
    assert posteriors("estimate", (2.0, 3.0))[1].clock_prior == (2.0, 3.0)
    for bad in (dict(clock=0.0), dict(clock=-1.0), dict(clock="yes"), dict(clock=1.0, clock_prior=(1.0, 1.0)),
                dict(clock=None, clock_prior=(1.0, 1.0)), dict(clock="estimate", clock_prior=(0.0, 1.0))):
        with pytest.raises(ValueError):
            geo.GeoPosterior(5, blens[2], gc.HostGeoClockLikelihood(tips, peels[2]), **bad)


# ---------------------------------------------------------------- the command line
def test_clock_flag_refusals(tmp_path):
    tree, meta = go.write_geo_dataset(str(tmp_path), S=6, K=3, seed=7)
    base = ["-s", str(tmp_path / "m.stan"), "-t", tree, "-o", str(tmp_path / "o")]
    for flags in (["--geo_clock"], ["--geo_rate", "0.5"], ["--geo_clock_prior", "1,2"]):
        with pytest.raises(SystemExit, match="needs --geo"):
            go.run_geo(base + flags, factory=gc.HostGeoClockLikelihood)
    geo_base = base + ["--geo", "-M", meta]
    with pytest.raises(SystemExit, match="--geo_clock .*--geo_rate"):
        go.run_geo(geo_base + ["--geo_clock", "--geo_rate", "0.5"], factory=gc.HostGeoClockLikelihood)
    with pytest.raises(SystemExit, match="--geo_clock_prior .*needs --geo_clock"):
        go.run_geo(geo_base + ["--geo_rate", "0.5", "--geo_clock_prior", "1,2"], factory=gc.HostGeoClockLikelihood)
    with pytest.raises(SystemExit, match="SHAPE,RATE"):
        go.run_geo(geo_base + ["--geo_clock", "--geo_clock_prior", "1"], factory=gc.HostGeoClockLikelihood)
    with pytest.raises(SystemExit, match="positive"):
        go.run_geo(geo_base + ["--geo_rate", "-2"], factory=gc.HostGeoClockLikelihood)
    with pytest.raises(SystemExit, match="evaluate_rows_clock"):  # a likelihood that cannot take a clock
        go.run_geo(geo_base + ["--geo_clock"])
    assert not os.path.exists(str(tmp_path / "o"))


def test_build_records_the_clock_and_run_checks_it(tmp_path):
    tree, meta = go.write_geo_dataset(str(tmp_path), S=6, K=3, seed=7)
    script = str(tmp_path / "m.stan")
    assert cli.main(["build", "-s", script, "--geo", "--geo_clock", "--geo_clock_prior", "0.5,2"]) == 0
    assert json.load(open(script))["options"] == {"geo": True, "rescaling_geo": False, "geo_clock": "estimate",
                                                  "geo_clock_prior": [0.5, 2.0]}
    fixed = str(tmp_path / "f.stan")
    assert cli.main(["build", "-s", fixed, "--geo", "--geo_rate", "0.25"]) == 0
    assert json.load(open(fixed))["options"]["geo_clock"] == 0.25
    plain = str(tmp_path / "p.stan")
    assert cli.main(["build", "-s", plain, "--geo"]) == 0
    assert json.load(open(plain))["options"] == {"geo": True, "rescaling_geo": False}  # as it always was
    run = ["-t", tree, "-o", str(tmp_path / "o"), "--geo", "-M", meta]
    for script_, flags in ((script, []), (script, ["--geo_rate", "0.25"]), (plain, ["--geo_clock"]),
                           (fixed, ["--geo_rate", "0.5"]), (script, ["--geo_clock", "--geo_clock_prior", "1,2"])):
        with pytest.raises(SystemExit, match="geo_clock.* differs from the built model"):
            go.run_geo(["-s", script_] + run + flags, factory=gc.HostGeoClockLikelihood)
    with pytest.raises(SystemExit):
        cli.main(["build", "-s", script, "--geo_clock"])


def read_tsv(path):
    return [ln.rstrip("\n").split("\t") for ln in open(path)]


@pytest.mark.parametrize("algorithm", ["vb", "nuts"])
def test_run_geo_clock_end_to_end(tmp_path, capsys, algorithm):
    S, K = 10, 3
    tree, meta = go.write_geo_dataset(str(tmp_path), S=S, K=K, seed=11)
    out = str(tmp_path / "geo")
    argv = ["-s", str(tmp_path / "m.stan"), "--geo", "--geo_clock", "--ancestral", "-M", meta, "-t", tree, "-o", out,
            "-S", "5"]
    if algorithm == "vb":
        argv += ["--iter", "100", "--elbo_samples", "10", "--samples", "20", "--tol_rel_obj", "0.01", "--eta", "0.1"]
    else:
        argv += ["-a", "nuts", "--iter", "16"]
    post, lines = go.run_geo(argv, factory=gc.HostGeoClockLikelihood)
    assert post.clock_estimated and post.dim == 3 + 2 + 1
    header, data = stan_io.read_samples(out)
    assert header[-2:] == ["freqs_geo.3", "rate_geo"]
    mu = data[:, -1]
    assert np.all(np.isfinite(mu)) and np.all(mu > 0.0)
    rates = read_tsv(out + ".rates.tsv")
    states = read_tsv(out + ".jumps.tsv")[0][1:-1]  # the locations in the order the run numbers them
    assert sorted(states) == ["P0", "P1", "P2"]
    assert rates[0] == ["from\\to"] + states and [r[0] for r in rates[1:]] == states
    for i in range(K):
        row = rates[1 + i] + [""] * (K + 1 - len(rates[1 + i]))
        assert row[1 + i] == "" and all(float(row[1 + j]) > 0.0 for j in range(K) if j != i)
    jt = read_tsv(out + ".jumps.tsv")
    tree_len = geo.mean_tree_length(post.blens)
    assert abs(sum(float(r[-1]) for r in jt[1:]) - tree_len) <= 1e-8 * tree_len  # dwell times in the tree's unit
    assert len([s for s in lines if s.startswith("rate_geo: posterior mean")]) == 1
    assert [s for s in lines if s.startswith("Trait clock rate: estimated, Gamma(0.5, %g)" % tree_len)]
    assert os.path.exists(out + ".trees")
    capsys.readouterr()


def test_run_geo_trees_clock_fixed_and_estimated(tmp_path, capsys):
    S, K, T = 10, 3, 3
    tree, meta, sample = write_dataset(tmp_path, S, K, T, 12)
    base = ["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree, "--trees", sample, "-S", "5",
            "--iter", "60", "--elbo_samples", "5", "--samples", "10", "--tol_rel_obj", "0.01", "--eta", "0.1"]
    out = str(tmp_path / "est")
    gc.HostGeoTreesClockLikelihood.made = []
    post, lines = go.run_geo(base + ["-o", out, "--geo_clock", "--geo_clock_prior", "1,2"],
                             factory=gc.HostGeoTreesClockLikelihood)
    assert isinstance(post, geo.GeoTreesPosterior) and post.clock_prior == (1.0, 2.0)
    header, data = stan_io.read_samples(out)
    assert header[-2:] == ["freqs_geo.3", "rate_geo"] and np.all(data[:, -1] > 0.0)
    lik = gc.HostGeoTreesClockLikelihood.made[0]
    lengths = lik.blens.sum(1)
    probs = np.array([float(r[1]) for r in read_tsv(out + ".treeprob.tsv")[1:]])
    times = sum(float(r[-1]) for r in read_tsv(out + ".jumps.tsv")[1:])
    assert abs(times - probs @ lengths) <= 1e-8 * lengths.max()
    assert os.path.exists(out + ".rates.tsv")
    out = str(tmp_path / "fix")
    post, lines = go.run_geo(base + ["-o", out, "--geo_rate", "0.5"], factory=gc.HostGeoTreesClockLikelihood)
    header, _ = stan_io.read_samples(out)
    assert "rate_geo" not in header and header[-1] == "freqs_geo.3" and post.clock_fixed == 0.5
    assert os.path.exists(out + ".rates.tsv") and not [s for s in lines if s.startswith("rate_geo:")]
    assert [s for s in lines if s == "Trait clock rate: fixed at 0.5"]
    capsys.readouterr()


# ---------------------------------------------------------------- recovery
def test_the_rate_is_recovered_when_the_time_unit_changes(capsys):
    """Locations simulated down a 40-tip tree at a known mu Q (K = 3); the model
    sees the same tree in a unit 100 times finer (every branch times 100).
    mu_true t is 0.15 a branch: away from saturation, where the tips still say
    how many moves there were.  The default prior's rate is the tree's length,
    as strong as the data (it halves a Poisson count's estimate), which is what
    the factor of 3 allows for."""
    S, K, mu_true, unit = 40, 3, 0.5, 100.0
    rng = np.random.default_rng(2024)
    peel = go.random_peel(S, rng)
    node_blens = rng.exponential(0.3, 2 * S - 1)  # the edge above every node, rooted
    rates = np.array([1.0, 0.4, 2.0])
    freqs = np.array([0.5, 0.3, 0.2])
    Q = geo.rate_matrix(freqs, rates)[0]
    state = {2 * S - 2: rng.choice(K, p=freqs)}
    for a, b, p in peel[::-1]:
        for ch in (a, b):
            P = go.expm(Q * (mu_true * node_blens[ch])).real
            state[ch] = rng.choice(K, p=P[state[p]] / P[state[p]].sum())
    tips = np.eye(K)[[state[n] for n in range(S)]]
    blens = node_blens[:2 * S - 3].copy()
    a, b, _ = peel[-1]
    blens[a] += node_blens[b]  # the merged root branch
    lik = gc.HostGeoClockLikelihood(tips, peel)
    post = geo.GeoPosterior(K, unit * blens, lik, clock="estimate")
    assert post.clock_prior == (0.5, float((unit * blens).sum()))
    free = np.concatenate([np.ravel(post.t_rates.unconstrain(rates[None])), np.ravel(post.t_freqs.unconstrain(freqs[None]))])
    assert np.allclose(post.flat_rows(np.concatenate([free, [0.0]])[None])[0, :-1], np.concatenate([rates, freqs]))

    def lp_at(mu):
        u = np.concatenate([free, [math.log(mu)]])
        return float(post.log_prob(u[None])[0])

    grid = np.exp(np.linspace(math.log(1e-5), math.log(10.0), 57))  # one-dimensional search, then golden section
    vals = np.array([lp_at(m) for m in grid])
    k = int(np.argmax(vals))
    assert 0 < k < grid.size - 1
    lo, hi = math.log(grid[k - 1]), math.log(grid[k + 1])
    g = (math.sqrt(5.0) - 1.0) / 2.0
    for _ in range(30):
        c, d = hi - g * (hi - lo), lo + g * (hi - lo)
        if lp_at(math.exp(c)) > lp_at(math.exp(d)):
            hi = d
        else:
            lo = c
    mu_hat = math.exp(0.5 * (lo + hi))
    params = np.concatenate([post.flat_rows(np.concatenate([free, [0.0]])[None])[0, :-1]])

    def loglik(mu):
        return float(lik.evaluate_rows_clock(unit * blens, params, mu)[0, 0])

    gain = loglik(mu_hat) - loglik(1.0)
    print("mu_true / unit = %.5g, maximiser %.5g, log L(maximiser) - log L(mu = 1) = %.3f"
          % (mu_true / unit, mu_hat, gain))
    assert mu_true / unit / 3.0 <= mu_hat <= 3.0 * mu_true / unit
    assert gain > 0.0
