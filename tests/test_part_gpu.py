"""GPU: the partitioned engine (include/phylo_hip_part.h).  The contracts of
DESIGN.md 5i on the smallest shapes where the block-range walk, the union of
the tip masks and the fold can go wrong:

1. truth: every partition row and its site log-likelihoods against the C
   oracle on the partition's own alignment at mu_k t; the draw's log L and
   d/dt against the sums; d/dmu_k against the complex step;
2. the fold, bit for bit (``partition_combine_host``);
3. one product: (t, mu) and (the numpy product mu_k t, 1) give the same bits;
4. a row's bits are its own (n, position, the other draws, a repeated call);
5. a rejected draw is -inf and zeros, the others keep their bits;
6. K = 1, mu = 1: the draw's row is its partition's row.

Every plan here is one chunk with the whole deep stack in LDS at C <= 4, so
these cases launch ``<512, 2, true>`` and ``<512, 1, true>`` only.  The other
four kernels, chunked staging, ``PHY_RECOMPUTE=0`` and ``PHY_QFUSE=0`` alone
are forced in tests/test_part_exact_gpu.py (forms and plan facts:
tests/test_part_exact_cpu.py), which holds the rows to the complex-step truth
on the edge draws of tests/part_exact_cases.py instead of the C oracle.
"""
import json
import os

import numpy as np
import pytest

from phylostan_amd import _lib, data as dataio, models, partition as pt
from tests import part_cases as pc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_DRAWS = 9


def clean_env(monkeypatch, **env):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def all_legs(c, eng, n_all):
    """Contracts 1 to 5 on the first n_all draws of ``c`` in the context ``eng``."""
    bl, mu, mv = c.blens[:n_all], c.mu[:n_all], c.model_vecs[:n_all]
    out, rows, site = eng.evaluate_rows(bl, mu, mv, part_rows=True, site_ll=True)
    assert out.shape == (n_all, c.outlen) and rows.shape == (n_all, c.K, c.rowlen)
    pc.check_truth(c, out, rows, site)                                   # 1
    pc.check_fold(c, out, rows)                                          # 2
    for k in range(c.K):                                                 # 3
        _, r1 = eng.evaluate_rows(mu[:, k:k + 1] * bl, np.ones_like(mu), mv, part_rows=True)
        np.testing.assert_array_equal(r1[:, k], rows[:, k])
    again = eng.evaluate_rows(bl, mu, mv)                                # 4
    np.testing.assert_array_equal(again, out)
    for pick in ([n_all // 2, 0, n_all - 1], [n_all - 2 if n_all > 1 else 0]):
        pick = [p for p in pick if p < n_all]
        o2, r2, s2 = eng.evaluate_rows(bl[pick], mu[pick], mv[pick], part_rows=True, site_ll=True)
        np.testing.assert_array_equal(o2, out[pick])
        np.testing.assert_array_equal(r2, rows[pick])
        np.testing.assert_array_equal(s2, site[pick])
    bad, mu_bad = mv.copy(), mu.copy()                                   # 5
    d_bad, k_bad = n_all // 2, c.K - 1
    if c.model == "JC69":  # no frequency parameters (the root's are fixed): a NaN rate instead
        mu_bad[d_bad, k_bad] = np.nan
    else:
        bad[d_bad, k_bad, 0] = -bad[d_bad, k_bad, 0]
    o3, r3 = eng.evaluate_rows(bl, mu_bad, bad, part_rows=True)
    assert o3[d_bad, 0] == -np.inf and not o3[d_bad, 1:].any()
    assert r3[d_bad, k_bad, 0] == -np.inf and not r3[d_bad, k_bad, 1:].any()
    keep = np.arange(n_all) != d_bad
    np.testing.assert_array_equal(o3[keep], out[keep])
    return out, rows, site


@pytest.mark.parametrize("i", range(len(pc.SHAPES)), ids=pc.SHAPE_IDS)
def test_contracts(i, monkeypatch):
    clean_env(monkeypatch)
    c = pc.shape_case(i)
    eng = c.engine(MAX_DRAWS)
    assert (eng.K, eng.B, eng.rowlen, eng.outlen) == (c.K, c.B, c.rowlen, c.outlen)
    out9, rows9, site9 = all_legs(c, eng, 9)
    for n in (3, 1):  # calls of 3 and 1 draws: the same bits as in the call of 9
        o, r, s = eng.evaluate_rows(c.blens[:n], c.mu[:n], c.model_vecs[:n], part_rows=True, site_ll=True)
        np.testing.assert_array_equal(o, out9[:n])
        np.testing.assert_array_equal(r, rows9[:n])
        np.testing.assert_array_equal(s, site9[:n])
    eng.close()


def test_union_of_tip_masks(monkeypatch):
    """One partition without ambiguity codes, one carrying all of 15, 3, 5, 10, 6: R and `extra` are the union's."""
    clean_env(monkeypatch)
    c = pc.ambiguity_case()
    plan = c.plan(MAX_DRAWS)
    masks = {(plan["extra_lo"] >> (4 * j)) & 15 for j in range(plan["R"] - 4)}
    assert plan["R"] == 4 + len(pc.AMBIGUITY) and masks == set(pc.AMBIGUITY) and plan["extra_hi"] == 0
    alone = pt.plan_partitions([c.parts[0][0]], c.peel0, c.rooted, c.C, MAX_DRAWS, model=c.model)
    assert alone["R"] == 5  # on its own the clean partition has the padding's mask 15 alone
    eng = c.engine(MAX_DRAWS)
    all_legs(c, eng, c.n)
    eng.close()


# max_draws 1 / 64 / 300: both column plans.  The finalize inside the sweep needs [C][B] + [C][8] doubles of LDS
# beside the tips, which every plan of these sizes has, so the placement after the sweep is reached through the
# PHY_FIN / PHY_QFUSE preferences at create (which fix the plan, as include/phylo_hip_part.h states).
PLANS = [(1, {}, 1, 1, 1, 0), (64, {"PHY_FIN": "0"}, 2, 0, 0, 1), (300, {}, 2, 1, 1, 0),
         (64, {"PHY_FIN": "0", "PHY_QFUSE": "0"}, 2, 0, 0, 0)]


@pytest.mark.parametrize("max_draws,env,cols,fin,qf,fin_qf", PLANS,
                         ids=["max1", "max64-nofin", "max300", "max64-nofin-noqfuse"])
def test_plans_of_max_draws(max_draws, env, cols, fin, qf, fin_qf, monkeypatch):
    clean_env(monkeypatch, **env)
    c = pc.shape_case(3)  # (127, 1, 200), S = 10, C = 2, GTR rooted
    plan = c.plan(max_draws)
    assert (plan["cols"], plan["fin"], plan["qf"], plan["fin_qf"]) == (cols, fin, qf, fin_qf), plan
    assert plan["latency"] == (1 if cols == 1 else 0)
    eng = c.engine(max_draws)
    n = min(max_draws, c.n)
    out, rows, site = all_legs(c, eng, n)
    if max_draws > c.n:  # a full call: every draw keeps the bits it had in the small one
        idx = np.arange(max_draws) % c.n
        o, r, s = eng.evaluate_rows(c.blens[idx], c.mu[idx], c.model_vecs[idx], part_rows=True, site_ll=True)
        np.testing.assert_array_equal(o, out[idx])
        np.testing.assert_array_equal(r, rows[idx])
        np.testing.assert_array_equal(s, site[idx])
    eng.close()


def test_one_partition_unit_rate(monkeypatch):
    """Contract 6: K = 1 and mu = 1 -- [log L, d/dt, tail] are the bits of the partition's row."""
    clean_env(monkeypatch)
    c = pc.PartCase((129,), 9, 3, "GTR", True, n=3, seed=31)
    eng = c.engine(4)
    mu = np.ones((c.n, 1))
    out, rows = eng.evaluate_rows(c.blens, mu, c.model_vecs, part_rows=True)
    B = c.B
    np.testing.assert_array_equal(out[:, :1 + B], rows[:, 0, :1 + B])
    np.testing.assert_array_equal(out[:, 2 + B:], rows[:, 0, 1 + B:])
    for d in range(c.n):
        np.testing.assert_array_equal(out[d], pt.partition_combine_host(rows[d], c.blens[d], mu[d]))
    eng.close()


def fluA_codon_split():
    from phylostan_amd.treeio import read_alignment
    base = os.path.join(ROOT, "tests", "golden", "examples", "fluA")
    d = dataio.load(os.path.join(base, "fluA.tree"), os.path.join(base, "fluA.fa"), rooted=True)
    chars = dataio.alignment_matrix(read_alignment(os.path.join(base, "fluA.fa")), d.tree.taxon_namespace)
    n = chars.shape[1]
    parts = [pt.Partition("pos%d" % (k + 1), np.arange(k, n, 3)) for k in range(3)]
    return d, chars, parts, pt.split_alignment(chars, parts)


def test_fluA_codon_positions_against_the_oracle(monkeypatch):
    clean_env(monkeypatch)
    from oracle import cpu
    d, chars, parts, split = fluA_codon_split()
    assert [s[0].shape[1] for s in split] == [65, 60, 137]
    C, n, K = 4, 4, 3
    rng = np.random.default_rng(8)
    bl = rng.uniform(0.001, 0.05, (n, d.B))
    mu = rng.uniform(0.4, 2.0, (n, K))
    mv = np.empty((n, K, 10 + 2 * C))
    for i in range(n):
        for k in range(K):
            rs, ps = models.weibull_site_rates(rng.uniform(0.3, 1.5), C)
            mv[i, k] = models.model_vector(rng.dirichlet(np.full(4, 8.0)),
                                           models.hky_exchangeabilities(rng.uniform(2.0, 8.0)), rs, ps)
    eng = pt.PartitionedLikelihood([(s[0], s[1]) for s in split], d.peel0, True, "HKY", C, max_draws=n)
    out, rows, site = eng.evaluate_rows(bl, mu, mv, part_rows=True, site_ll=True)
    eng.close()
    rowlen = 1 + d.B + 2 * C + 14
    for i in range(n):
        for k in range(K):
            ref, s = cpu.evaluate(split[k][0], split[k][1], d.peel0, True, models.MODEL_IDS["HKY"], mv[i, k],
                                  mu[i, k] * bl[i], C, site_ll=True)
            assert abs(rows[i, k, 0] - ref[0]) <= pc.RTOL_LL * abs(ref[0])
            np.testing.assert_allclose(site[i, eng.off[k]:eng.off[k + 1]], s, rtol=pc.RTOL_LL, atol=1e-12)
            pc._close(rows[i, k, 1:1 + d.B], ref[1:1 + d.B], pc.RTOL_G, "d/dblens")
            o = 1 + d.B
            pc._close(rows[i, k, o:o + C], ref[o:o + C], pc.RTOL_G, "drs")
            pc._close(rows[i, k, o + 2 * C + 4:o + 2 * C + 10], ref[o + 2 * C + 4:rowlen - 4], pc.RTOL_Q, "drates")
            pc._close(rows[i, k, o + 2 * C + 10:], ref[rowlen - 4:rowlen], pc.RTOL_Q, "dfreqs")
        np.testing.assert_array_equal(out[i], pt.partition_combine_host(rows[i], bl[i], mu[i]))


def test_live_contexts_reproduce_the_pinned_plans(monkeypatch):
    """tests/golden/part_plans.json (recorded without a device) against the plan live contexts report."""
    clean_env(monkeypatch)
    with open(os.path.join(ROOT, "tests", "golden", "part_plans.json")) as fp:
        pinned = json.load(fp)
    from tests.golden import record_part_plans as rec
    live = rec.cases()
    assert len(live) == len(pinned["rows"])
    for (name, c, max_draws), row in zip(live, pinned["rows"]):
        assert (name, max_draws, list(c.widths)) == (row["case"], row["max_draws"], row["widths"])
        eng = c.engine(max_draws)
        info = eng.info()
        eng.close()
        assert {k: info[k] for k in pt.PLAN_FACTS} == row["facts"], name
        assert info["blocks"] == row["block_ranges"], name


def test_refusals_touch_no_device():
    c = pc.shape_case(1)
    with pytest.raises(_lib.PhyloHipError, match=r"max_draws \* K = 65536"):
        pt.PartitionedLikelihood(c.parts, c.peel0, c.rooted, c.model, c.C, max_draws=32768, device=10 ** 6)
    empty = [c.parts[0], (np.zeros((c.S, 0), np.uint8), np.zeros(0))]
    with pytest.raises(_lib.PhyloHipError, match="partition 1"):
        pt.PartitionedLikelihood(empty, c.peel0, c.rooted, c.model, c.C, max_draws=4, device=10 ** 6)


def test_cli_fluA_three_codon_partitions(tmp_path):
    """``run --partitions`` on the device: fluA by codon position, mean-field ADVI.  100 iterations, not 50: the
    ELBO is evaluated every 100th iteration (advi.ADVI's eval_elbo), so a 50-iteration run writes no ELBO row to
    check; everything else is the 50-iteration run's."""
    from phylostan_amd import cli, stan_io
    base = os.path.join(ROOT, "tests", "golden", "examples", "fluA")
    parts = str(tmp_path / "codon.txt")
    with open(parts, "w") as fp:
        fp.write("".join("DNA, pos%d = %d-987\\3\n" % (k, k) for k in (1, 2, 3)))
    out = str(tmp_path / "fluA")
    import argparse
    parser = argparse.ArgumentParser()
    cli.create_run_parser(parser.add_subparsers()).set_defaults(func=cli.run)
    arg = parser.parse_args(["run", "-s", str(tmp_path / "m.json"), "-m", "HKY", "-C", "4", "-t",
                             os.path.join(base, "fluA.tree"), "-i", os.path.join(base, "fluA.fa"), "-o", out,
                             "--partitions", parts, "-a", "vb", "-S", "2", "--iter", "100", "--elbo_samples", "10",
                             "--samples", "10"])
    post = cli.run(arg, log=lambda *_: None)
    diag = [r for r in open(out + ".diag").read().splitlines() if r and not r.startswith("#")]
    assert diag[0] == "iter,time_in_seconds,ELBO" and len(diag) >= 2
    assert all(np.isfinite(float(r.split(",")[2])) for r in diag[1:])
    header, data = stan_io.read_samples(out)
    for k in (1, 2, 3):
        for nm in ("wshape_p%d" % k, "kappa_p%d" % k, "freqs_p%d.4" % k, "rs_p%d.4" % k, "mu.%d" % k):
            assert nm in header
    assert data.shape == (11, len(header))
    tsv = [ln.split("\t") for ln in open(out + ".partitions.tsv").read().splitlines()][1:]
    assert [(r[0], r[1], r[2]) for r in tsv] == [("pos1", "329", "65"), ("pos2", "329", "60"), ("pos3", "329", "137")]
    # sum_k (N_k / N) mu.k = 1 in every draw: to 1e-12 in the draws' own doubles, and to the six digits the CSV holds
    vals, _, _ = post.constrain(post.output_draws)
    mu = post.relative_rates(vals, 10)
    np.testing.assert_allclose(mu @ post.n_sites / post.n_sites.sum(), 1.0, rtol=1e-12)
    csv_mu = data[1:, [header.index("mu.%d" % k) for k in (1, 2, 3)]]
    np.testing.assert_allclose(csv_mu, mu, rtol=1e-5)
    np.testing.assert_allclose(csv_mu.mean(axis=1), 1.0, rtol=1e-5)


def test_partitioned_posterior_mu_identity_on_device():
    """sum_k (N_k / N) mu_k = 1 to 1e-12 in every draw, and the device-backed log density agrees with the host
    stand-in's, on the fluA codon split."""
    from phylostan_amd.posterior import ModelSpec, TreeData
    from tests.oracle_backend import OracleLikelihood
    d, chars, parts, split = fluA_codon_split()
    spec = ModelSpec(model="HKY", categories=4)
    du = dataio.load(os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.tree"),
                     os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.fa"), rooted=False)
    tree = TreeData(du.S, du.peel0, du.map, None, None)
    eng = pt.PartitionedLikelihood([(s[0], s[1]) for s in split], du.peel0, False, "HKY", 4, max_draws=4)
    post = pt.PartitionedPosterior(spec, tree, eng, [p.sites.size for p in parts])
    U = np.random.default_rng(4).uniform(-1.0, 1.0, (4, post.dim))
    U[:, post.param("blens").sl] -= 3.0
    vals, _, _ = post.constrain(U)
    mu = post.relative_rates(vals, 4)
    np.testing.assert_allclose(mu @ post.n_sites / post.n_sites.sum(), 1.0, rtol=1e-12)
    lp, G = post.log_prob_grad(U)
    assert np.all(np.isfinite(lp)) and np.all(np.isfinite(G))

    def ev(lik):
        def f(bl, mv, site_ll):
            r = lik.evaluate(bl, mv, site_ll)
            return np.concatenate([[r.loglik], r.grad_blens, r.grad_rs, r.grad_ps, r.grad_freq_root, r.grad_rates,
                                   r.grad_freqs]), None
        return f
    host = pt.partition_host([ev(OracleLikelihood(s[0], s[1], du.peel0, False, "HKY", 4)) for s in split], du.B, 4,
                             [s[0].shape[1] for s in split])
    ref = pt.PartitionedPosterior(spec, tree, host, [p.sites.size for p in parts])
    lr, Gr = ref.log_prob_grad(U[:2])
    np.testing.assert_allclose(lp[:2], lr, rtol=1e-10)
    np.testing.assert_allclose(G[:2], Gr, rtol=1e-7, atol=1e-7 * np.max(np.abs(Gr)))
    eng.close()
