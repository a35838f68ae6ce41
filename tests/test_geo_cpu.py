"""CPU: phylogeography (``--geo``) above the kernel -- the two references
against each other, the host restatement of the device's derivation against
the complex-step truth, the metadata reader, the posterior, the planner under
the host sanitizers, and ``run --geo`` end to end on the oracle-backed
likelihood.  The device engine itself: tests/test_geo_gpu.py."""
import argparse
import json
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import cli, geo, stan_io
from tests import geo_oracle as go
from tests.geo_oracle import run_geo, write_geo_dataset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 2), (7, 5), (30, 17), (69, 40)]


def point(S, K, seed):
    rng = np.random.default_rng(seed)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=(0,))
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens[0, 1] = 0.0
    R = geo.rate_count(K)
    return tips, peel, blens[0], params[0, :R], params[0, R:]


@pytest.mark.parametrize("S,K", SHAPES)
def test_stan_restatement_agrees_with_the_truth(S, K):
    tips, peel, blens, rates, freqs = point(S, K, 10 * S + K)
    a = go.stan_loglik(tips, peel, blens, rates, freqs)
    b = go.truth(tips, peel, blens, rates, freqs).real
    assert abs(a - b) <= 1e-10 * abs(b)
    ext = go.truth(tips, peel, blens, rates, freqs, extended=True).real
    assert abs(ext - b) <= 1e-12 * abs(b)


@pytest.mark.parametrize("S,K", SHAPES)
def test_host_restatement_agrees_with_the_truth(S, K):
    tips, peel, blens, rates, freqs = point(S, K, 10 * S + K)
    ll, gb, gr, gf = geo.geo_gradients_host(tips, peel, blens, rates, freqs)
    tl, tg = go.truth_gradients(tips, peel, blens, rates, freqs, max_entries=8)
    assert abs(ll - tl) <= 1e-10 * abs(tl)
    for name, got in (("blens", gb), ("rates", gr), ("freqs", gf)):
        idx, want = tg[name]
        if name == "rates" and K == 2:  # the normalisation cancels the single rate: exactly zero
            assert np.abs(got).max() <= 1e-12 and np.abs(want).max() <= 1e-12
            continue
        assert np.abs(got[idx] - want).max() <= 1e-9 * np.abs(got).max(), name


@pytest.mark.parametrize("arm", ["tie", "near"])
def test_host_restatement_with_a_repeated_eigenvalue(arm):
    K = 6
    tips, peel, blens, rates, _ = point(9, K, 5)
    rates = np.ones_like(rates)
    if arm == "near":
        rates[1] += 1e-11
    freqs = np.full(K, 1.0 / K)
    ll, gb, gr, gf = geo.geo_gradients_host(tips, peel, blens, rates, freqs)
    tl, tg = go.truth_gradients(tips, peel, blens, rates, freqs)
    assert abs(ll - tl) <= 1e-10 * abs(tl)
    for name, got in (("blens", gb), ("rates", gr), ("freqs", gf)):
        assert np.abs(got - tg[name][1]).max() <= 1e-9 * np.abs(got).max(), name


def test_host_restatement_rescales_past_the_fp64_range():
    S, K = 600, 8
    rng = np.random.default_rng(600)
    peel, tips = go.random_peel(S, rng), go.random_tips(S, K, rng)
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    R = geo.rate_count(K)
    rates, freqs = params[0, :R], params[0, R:]
    with np.errstate(divide="ignore"):
        assert go.truth(tips, peel, blens[0], rates, freqs).real == -np.inf
        assert go.stan_loglik(tips, peel, blens[0], rates, freqs) == -np.inf
    ll, gb, gr, gf = geo.geo_gradients_host(tips, peel, blens[0], rates, freqs)
    tl, tg = go.truth_gradients(tips, peel, blens[0], rates, freqs, extended=True, max_entries=4)
    assert tl < np.log(np.finfo(np.float64).tiny) and abs(ll - tl) <= 1e-10 * abs(tl)
    for name, got in (("blens", gb), ("rates", gr), ("freqs", gf)):
        idx, want = tg[name]
        assert np.abs(got[idx] - want).max() <= 1e-9 * np.abs(got).max(), name


@pytest.mark.parametrize("K", [2, 3, 5, 17, 64])
def test_round_robin_jacobi_matches_eigh(K):
    """The device's rotation order, on the host: every pair once per sweep
    (odd K with a bye), and the same spectrum as LAPACK's."""
    rng = np.random.default_rng(K)
    _, params = go.random_draws(1, 1, K, rng)
    R = geo.rate_count(K)
    Q = geo.rate_matrix(params[0, R:], params[0, :R])[0]
    sq = np.sqrt(params[0, R:])
    A = sq[:, None] * Q / sq[None, :]
    A = 0.5 * (A + A.T)
    lam, V, sweeps = geo.jacobi_round_robin(A)
    assert 1 <= sweeps <= 12
    assert np.abs(np.sort(lam) - np.linalg.eigvalsh(A)).max() <= 1e-13 * np.abs(lam).max()
    assert np.abs(V @ np.diag(lam) @ V.T - A).max() <= 1e-13 * np.abs(A).max()
    assert np.abs(V.T @ V - np.eye(K)).max() <= 1e-13
    # the equal-rates model: a (K-1)-fold eigenvalue
    Q = geo.rate_matrix(np.full(K, 1.0 / K), np.ones(R))[0]
    lam, V, sweeps = geo.jacobi_round_robin(Q)
    assert sweeps >= 0 and np.abs(V @ np.diag(lam) @ V.T - Q).max() <= 1e-13 * np.abs(Q).max()


def test_rate_fill_order_is_the_emitters():
    assert geo.rate_pairs(4) == [(1, 0), (2, 0), (3, 0), (2, 1), (3, 1), (3, 2)]
    Q = geo.rate_matrix(np.full(3, 1 / 3), np.array([1.0, 2.0, 3.0]))[1]
    assert Q[1, 0] == 1.0 and Q[2, 0] == 2.0 and Q[2, 1] == 3.0 and np.all(Q == Q.T)


# ---------------------------------------------------------------- metadata
def test_read_metadata_state_order_and_errors(tmp_path):
    path = str(tmp_path / "meta.tsv")
    with open(path, "w") as fp:
        fp.write("strain\tHost\tCountry\n")
        fp.write("a\thuman\tPeru\nb\tswine\tChile\nc\thuman\tPeru\nd\thuman\tFiji\n")
    tips, states = geo.read_metadata(path, taxa=["c", "d", "b", "a"])
    assert states == ["Peru", "Fiji", "Chile"]  # first seen in taxon-namespace order, not file order
    assert tips.tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0]]
    tips, states = geo.read_metadata(path, key="Host", taxa=["b", "a"])
    assert states == ["swine", "human"] and tips.tolist() == [[1, 0], [0, 1]]
    assert geo.read_metadata(path)[1] == ["Peru", "Chile", "Fiji"]
    with pytest.raises(ValueError, match="without a row"):
        geo.read_metadata(path, taxa=["a", "zz"])
    with pytest.raises(ValueError, match="no column"):
        geo.read_metadata(path, key="Region", taxa=["a"])


# ---------------------------------------------------------------- posterior
def make_posterior(S=7, K=4, seed=3):
    tips, peel, blens, _, _ = point(S, K, seed)
    lik = go.HostGeoLikelihood(tips, peel)
    return geo.GeoPosterior(K, blens, lik)


def test_posterior_gradient_against_central_differences():
    post = make_posterior()
    assert post.dim == geo.rate_count(4) + 3
    rng = np.random.default_rng(0)
    u = rng.normal(0.0, 0.7, post.dim)
    lp, G = post.log_prob_grad(u[None])
    assert np.isfinite(lp[0])
    h = 1e-5
    for k in range(post.dim):
        e = np.zeros(post.dim)
        e[k] = h
        fd = (post.log_prob(u + e)[0] - post.log_prob(u - e)[0]) / (2 * h)
        # central differences: truncation h^2 f''' / 6 plus rounding eps |f| / h, both ~1e-9 here
        assert abs(fd - G[0, k]) <= 1e-6 * max(1.0, abs(G[0, k])), k


def test_posterior_batch_equals_single_and_rejects_bad_draws():
    post = make_posterior()
    rng = np.random.default_rng(1)
    U = rng.normal(0.0, 1.0, (5, post.dim))
    U[3, 0] = np.nan
    lp, G = post.log_prob_grad(U)
    assert lp[3] == -np.inf and np.all(G[3] == 0.0)
    for k in (0, 1, 2, 4):
        lp1, G1 = post.log_prob_grad(U[k][None])
        assert lp1[0] == lp[k] and np.array_equal(G1[0], G[k])
    assert np.allclose(post.log_prob(U[:3], propto=False) - post.log_prob(U[:3]), np.log(6.0))  # Gamma(4)
    rows = post.flat_rows(U[:3])
    assert rows.shape == (3, 6 + 4) and np.all(rows[:, :6] > 0.1) and np.allclose(rows[:, 6:].sum(1), 1.0)
    assert post.column_names()[:2] == ["rates_geo.1", "rates_geo.2"] and post.column_names()[-1] == "freqs_geo.4"
    q = post.initialize(np.random.default_rng(2))
    assert q.shape == (post.dim,)


# ---------------------------------------------------------------- planner
def test_geo_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "geo_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "geo_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "0 failures" in run.stdout


def test_boundary_is_declared_and_bound():
    from phylostan_amd import _lib
    top = open(os.path.join(ROOT, "include", "phylo_hip.h")).read()
    assert '#include "phylo_hip_geo.h"' in top  # the consumer boundary carries it
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_geo.h")).read(), flags=re.S)
    for name in ("phy_geo_create", "phy_geo_destroy", "phy_geo_num_branches", "phy_geo_output_len", "phy_geo_eval"):
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.GEO_SIGNATURES
    for name in ("phy_geo_info", "phy_geo_sweeps"):
        assert name in _lib.SIGNATURES
    src = open(os.path.join(ROOT, "phylostan_amd", "csrc", "phylo_hip.hip")).read()
    assert '#include "geo_engine.inc"' in src and '#include "geo_plan.h"' in src


# ---------------------------------------------------------------- the CLI
def test_build_geo_writes_the_model_description(tmp_path):
    script = str(tmp_path / "m.stan")
    assert cli.main(["build", "-s", script, "--geo", "--rescaling_geo"]) == 0
    doc = json.load(open(script))
    assert doc["options"] == {"geo": True, "rescaling_geo": True}
    help_text = cli.create_build_parser(argparse.ArgumentParser().add_subparsers(), "build", "x").format_help()
    assert "not supported" not in help_text and "changes nothing" in " ".join(help_text.split())


def test_run_geo_vb_end_to_end(tmp_path, capsys):
    tree, meta = write_geo_dataset(str(tmp_path), S=8, K=3, seed=4)
    out = str(tmp_path / "geo")
    post, lines = run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "-t", tree, "-o", out, "-S", "5",
                           "--iter", "200", "--elbo_samples", "10", "--samples", "30", "--tol_rel_obj", "0.01"])
    quoted = [s for s in lines if s.startswith('"')]
    assert len(quoted) == 1 and sorted(quoted[0].strip('"').split('","')) == ["P0", "P1", "P2"]
    header, data = stan_io.read_samples(out)
    assert header == ["lp__"] + ["rates_geo.%d" % k for k in (1, 2, 3)] + ["freqs_geo.%d" % k for k in (1, 2, 3)]
    assert data.shape == (31, 7) and np.all(data[:, 1:4] >= 0.1) and np.allclose(data[:, 4:].sum(1), 1.0, atol=1e-5)
    diag = [r for r in open(out + ".diag").read().splitlines() if not r.startswith("#")]
    assert diag[0] == "iter,time_in_seconds,ELBO" and diag[1].startswith("100,")
    assert all(np.isfinite(float(r.split(",")[2])) for r in diag[1:])
    assert not os.path.exists(out + ".trees")
    assert post.lik.calls > 0
    capsys.readouterr()


def test_run_geo_metadata_key_and_nuts(tmp_path, capsys):
    tree, meta = write_geo_dataset(str(tmp_path), S=6, K=3, seed=6)
    out = str(tmp_path / "geo")
    post, lines = run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "--metadata_key", "Region", "-t", tree,
                           "-o", out, "-a", "nuts", "--iter", "20", "-S", "2"])
    assert post.K == 2
    header, data = stan_io.read_samples(out)
    assert header[7:] == ["rates_geo.1", "freqs_geo.1", "freqs_geo.2"] and data.shape[0] == 10
    capsys.readouterr()


def test_run_geo_refusals(tmp_path):
    tree, meta = write_geo_dataset(str(tmp_path), S=6, K=3, seed=7)
    base = ["-s", str(tmp_path / "m.stan"), "-t", tree, "-o", str(tmp_path / "o")]
    with pytest.raises(SystemExit, match="needs a metadata file"):
        run_geo(base + ["--geo"])
    with pytest.raises(SystemExit, match="needs --geo"):
        run_geo(base + ["-M", meta])
    with pytest.raises(SystemExit, match="no column"):
        run_geo(base + ["--geo", "-M", meta, "--metadata_key", "Continent"])
    sub = str(tmp_path / "neg")
    os.mkdir(sub)
    tree2, meta2 = write_geo_dataset(sub, S=6, K=3, seed=7, negative=True)
    with pytest.raises(SystemExit) as e:
        run_geo(["-s", str(tmp_path / "m.stan"), "-t", tree2, "-o", str(tmp_path / "o"), "--geo", "-M", meta2])
    assert e.value.code == 3  # phylostan.py:242-243
    short = str(tmp_path / "short.tsv")
    with open(short, "w") as fp:
        fp.write("strain\tCountry\nt1\tP0\n")
    with pytest.raises(SystemExit, match="without a row"):
        run_geo(base + ["--geo", "-M", short])
    # a DNA model description is not a geo one
    cli.main(["build", "-s", str(tmp_path / "dna.stan"), "-m", "JC69"])
    with pytest.raises(SystemExit, match="differs from the built model"):
        run_geo(["-s", str(tmp_path / "dna.stan"), "-t", tree, "-o", str(tmp_path / "o"), "--geo", "-M", meta])
