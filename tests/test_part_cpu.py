"""CPU: the device-free parts of partitioned alignments -- the partition file
reader, the per-partition compression, the planner (csrc/part_plan.h) under
host sanitizers and pinned in tests/golden/part_plans.json, the host stand-in
against the truths of DESIGN.md 5i, the fold, ``PartitionedPosterior`` on the
stand-in, the ABI's declaration, and ``run --partitions`` end to end."""
import json
import math
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import _lib, cli, data as dataio, partition as pt, stan_io
from phylostan_amd.posterior import ModelSpec, Posterior, TreeData
from tests import cases, fixture_files, part_cases as pc
from tests.oracle_backend import OracleLikelihood
from tests.test_posterior import check_grad, preorder_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# -------------------------------------------------------- the partition file
def _write(tmp_path, text):
    path = str(tmp_path / "parts.txt")
    with open(path, "w") as fp:
        fp.write(text)
    return path


def test_read_partitions_ranges_and_strides(tmp_path):
    path = _write(tmp_path, "DNA, pos12 = 1-12\\3, 2-12\\3\n# a comment\nDNA,pos3=3-12\\3\n\ntail = 13-14, 15\n")
    parts = pt.read_partitions(path, 15)
    assert [p.name for p in parts] == ["pos12", "pos3", "tail"]
    assert parts[0].sites.tolist() == [0, 1, 3, 4, 6, 7, 9, 10]
    assert parts[1].sites.tolist() == [2, 5, 8, 11]
    assert parts[2].sites.tolist() == [12, 13, 14]


def test_read_partitions_refusals(tmp_path):
    with pytest.raises(ValueError, match=r"partition b: site 5 is already in partition a"):
        pt.read_partitions(_write(tmp_path, "a = 1-5\nb = 5-10\n"), 10)
    with pytest.raises(ValueError, match=r"site 6 is in no partition \(after partition a\)"):
        pt.read_partitions(_write(tmp_path, "a = 1-5\nb = 7-10\n"), 10)
    with pytest.raises(ValueError, match=r"partition b: site 11 is past the alignment's 10 sites"):
        pt.read_partitions(_write(tmp_path, "a = 1-5\nb = 6-12\n"), 10)
    with pytest.raises(ValueError, match=r"partition b: site 12 is past"):
        pt.read_partitions(_write(tmp_path, "a = 1-5, 7-10\\2, 8-10\\2\nb = 6-12\\3\n"), 10)
    with pytest.raises(ValueError, match=r"partition a: site 3 is listed twice"):
        pt.read_partitions(_write(tmp_path, "a = 1-5, 3\nb = 6-10\n"), 10)


def fluA_chars():
    base = os.path.join(ROOT, "tests", "golden", "examples", "fluA")
    d = dataio.load(os.path.join(base, "fluA.tree"), os.path.join(base, "fluA.fa"), rooted=True)
    return d, dataio.alignment_matrix(dataio.read_alignment(os.path.join(base, "fluA.fa")), d.tree.taxon_namespace)


def test_split_alignment_fluA_codon_positions(tmp_path):
    d, chars = fluA_chars()
    assert chars.shape[1] == 987
    path = _write(tmp_path, "".join("DNA, pos%d = %d-987\\3\n" % (k, k) for k in (1, 2, 3)))
    parts = pt.read_partitions(path, chars.shape[1])
    split = pt.split_alignment(chars, parts)
    assert [s[0].shape[1] for s in split] == [65, 60, 137] and [p.sites.size for p in parts] == [329] * 3
    for p, (tip, w, sp) in zip(parts, split):
        ref_tip, ref_w, _ = dataio.compress_patterns(chars[:, p.sites])
        np.testing.assert_array_equal(tip, ref_tip)
        np.testing.assert_array_equal(w, ref_w)
        assert w.sum() == 329 and sp.shape == (329,)
        np.testing.assert_array_equal(tip[:, sp], dataio.compress_patterns(chars)[0][:, dataio.site_patterns(chars)][:, p.sites])
        assert np.any(tip == 15)  # every partition has gaps
    both = pt.split_alignment(chars, pt.read_partitions(_write(tmp_path, "a = 1-987\\3, 2-987\\3\nb = 3-987\\3\n"), 987))
    assert [s[0].shape[1] for s in both] == [119, 137]


# ----------------------------------------------------------------- the planner
def test_part_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "part_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "part_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-2000:]
    assert re.search(r"part_plan_check: \d+ plans, 0 failures", ran.stdout)


def test_plans_are_pinned(monkeypatch):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    from tests.golden import record_part_plans as rec
    with open(rec.GOLDEN) as fp:
        pinned = json.load(fp)
    assert rec.record() == pinned
    by = {(r["case"], r["max_draws"]): r for r in pinned["rows"]}
    # both column plans occur over max_draws 1 / 64 / 300, and the padded layout is what the header states
    assert [by[(pc.SHAPE_IDS[3], m)]["facts"]["cols"] for m in (1, 64, 300)] == [1, 2, 2]
    assert by[(pc.SHAPE_IDS[3], 9)]["first_columns"] == [0, 128, 256]
    assert by[(pc.SHAPE_IDS[4], 9)]["first_columns"] == [0, 256, 384, 512]
    assert by[("ambiguity", 9)]["facts"]["R"] == 9


def test_plan_refusals_name_the_partition():
    c = pc.shape_case(1)
    tips = [p[0] for p in c.parts]
    with pytest.raises(_lib.PhyloHipError, match="partition 1"):
        pt.plan_partitions([tips[0], tips[1][:, :0]], c.peel0, c.rooted, c.C, 4)
    with pytest.raises(_lib.PhyloHipError, match="K >= 1"):
        pt.plan_partitions([], c.peel0, c.rooted, c.C, 4)
    with pytest.raises(_lib.PhyloHipError, match="65535"):
        pt.plan_partitions(tips, c.peel0, c.rooted, c.C, 32768)


# ------------------------------------------------------------------ the ABI
def test_part_boundary_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_part.h")).read(), flags=re.S)
    ctx = r"phy_part_ctx\s*\*\s*\w*"
    dbl, cdbl = r"\s*double\s*\*\s*\w+\s*", r"\s*const\s+double\s*\*\s*\w+\s*"
    assert re.search(r"typedef\s+struct\s+phy_part_ctx\s+phy_part_ctx\s*;", text)
    assert re.search(r"\bint\s+phy_part_create\s*\(\s*int\s+S\s*,\s*int\s+K\s*,\s*const\s+int32_t\s*\*\s*P_k\s*,\s*int\s+C\s*,"
                     r"\s*int\s+rooted\s*,\s*int\s+model\s*,\s*const\s+uint8_t\s*\*\s*tipcodes\s*,"
                     r"\s*const\s+double\s*\*\s*weights\s*,\s*const\s+int32_t\s*\*\s*peel\s*,\s*int\s+max_draws\s*,"
                     r"\s*int\s+device\s*,\s*phy_part_ctx\s*\*\*\s*out\s*\)", text)
    assert re.search(r"\bint\s+phy_part_destroy\s*\(\s*" + ctx + r"\)", text)
    for name in ("num_partitions", "num_branches", "row_len", "output_len"):
        assert re.search(r"\bint\s+phy_part_%s\s*\(\s*const\s+" % name + ctx + r"\)", text)
    assert re.search(r"\bint\s+phy_part_eval\s*\(\s*" + ctx + r",\s*int\s+n_draws\s*," + cdbl + "," + cdbl + "," + cdbl + "," +
                     dbl + "," + dbl + "," + dbl + r"\)", text)
    for name, nargs in (("phy_part_create", 12), ("phy_part_destroy", 1), ("phy_part_num_partitions", 1),
                        ("phy_part_num_branches", 1), ("phy_part_row_len", 1), ("phy_part_output_len", 1),
                        ("phy_part_eval", 8)):
        assert name in _lib.PART_SIGNATURES and len(_lib.PART_SIGNATURES[name][1]) == nargs
    assert len(_lib.SIGNATURES["phy_part_plan"][1]) == 15 and len(_lib.SIGNATURES["phy_part_info"][1]) == 3
    assert '#include "phylo_hip_part.h"' in open(os.path.join(ROOT, "include", "phylo_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "phylo_hip_diag.h")).read()
    assert re.search(r"\bint\s+phy_part_plan\s*\(", diag) and re.search(r"\bint\s+phy_part_info\s*\(", diag)


# ------------------------------------------------------------ the host form
@pytest.mark.parametrize("i", range(len(pc.SHAPES)), ids=pc.SHAPE_IDS)
def test_partition_host_against_the_truths(i):
    c = pc.shape_case(i)
    host = c.host()
    n = 3
    out, rows, site = host.evaluate_rows(c.blens[:n], c.mu[:n], c.model_vecs[:n], part_rows=True, site_ll=True)
    assert out.shape == (n, c.outlen) and rows.shape == (n, c.K, c.rowlen) and site.shape == (n, sum(c.widths))
    pc.check_truth(c, out, rows, site)
    pc.check_fold(c, out, rows)
    # a rejected partition (the device's rule: a negative frequency is -inf) rejects its draw alone
    evs = c.evaluators()
    first = evs[0]
    evs[0] = lambda bl, mv, sl: (np.full(c.rowlen, -np.inf), None) if mv[0] < 0 else first(bl, mv, sl)
    bad = c.model_vecs[:n].copy()
    bad[1, 0, 0] = -bad[1, 0, 0]
    o2, r2 = pt.partition_host(evs, c.B, c.C, c.widths).evaluate_rows(c.blens[:n], c.mu[:n], bad, part_rows=True)
    assert o2[1, 0] == -np.inf and not o2[1, 1:].any()
    assert r2[1, 0, 0] == -np.inf and not r2[1, 0, 1:].any()
    np.testing.assert_array_equal(o2[[0, 2]], out[[0, 2]])


def test_combine_against_a_plain_loop():
    rng = np.random.default_rng(12)
    for K, B, tail in ((1, 5, 16), (2, 11, 18), (4, 21, 22)):
        rows = rng.normal(size=(K, 1 + B + tail)) * 10.0 ** rng.integers(-3, 4, (K, 1))
        t, mu = rng.uniform(0.01, 0.4, B), rng.uniform(0.2, 3.0, K)
        out = pt.partition_combine_host(rows, t, mu)
        ref = []
        ll = float(rows[0][0])
        for k in range(1, K):
            ll = ll + float(rows[k][0])
        ref.append(ll)
        for b in range(B):
            v = float(mu[0]) * float(rows[0][1 + b])
            for k in range(1, K):
                v = v + float(mu[k]) * float(rows[k][1 + b])
            ref.append(v)
        for k in range(K):
            v = float(t[0]) * float(rows[k][1])
            for b in range(1, B):
                v = v + float(t[b]) * float(rows[k][1 + b])
            ref.append(v)
            ref += [float(x) for x in rows[k][1 + B:]]
        np.testing.assert_array_equal(out, np.array(ref))
        if K == 1:  # mu = 1: the partition's own bits
            one = pt.partition_combine_host(rows, t, np.ones(1))
            np.testing.assert_array_equal(one[:1 + B], rows[0, :1 + B])
            np.testing.assert_array_equal(one[2 + B:], rows[0, 1 + B:])
        rows[K - 1, 0] = np.nan
        rej = pt.partition_combine_host(rows, t, mu)
        assert rej[0] == -np.inf and not rej[1:].any()


# ------------------------------------------------------------- the posterior
def _row_evaluator(lik):
    def ev(bl, mv, site_ll):
        r = lik.evaluate(bl, mv, site_ll)
        return np.concatenate([[r.loglik], r.grad_blens, r.grad_rs, r.grad_ps, r.grad_freq_root, r.grad_rates,
                               r.grad_freqs]), r.site_ll
    return ev


def _partitioned_posterior(seed, widths, model, C, clock, coalescent=None, S=7):
    case = cases.random_case(seed, S=S, P=int(sum(widths)), C=1, model=model, rooted=clock is not None)
    tree = TreeData(S, case.peel0, preorder_map(case.peel0), None, None)
    spec = ModelSpec(model=model, categories=C, clock=clock, estimate_rate=clock is not None, coalescent=coalescent)
    off = np.concatenate([[0], np.cumsum(widths)])
    liks = [OracleLikelihood(case.tipcodes[:, off[k]:off[k + 1]], case.weights[off[k]:off[k + 1]], case.peel0,
                             clock is not None, model, spec.C) for k in range(len(widths))]
    host = pt.partition_host([_row_evaluator(lk) for lk in liks], liks[0].B, spec.C, widths)
    n_sites = [int(case.weights[off[k]:off[k + 1]].sum()) for k in range(len(widths))]
    return pt.PartitionedPosterior(spec, tree, host, n_sites), spec, tree, case


@pytest.mark.parametrize("model,C,clock,coalescent", [("JC69", 1, None, None), ("HKY", 4, "strict", "constant"),
                                                      ("GTR", 2, None, None)],
                         ids=["JC69-noclock", "HKY+W4-strict", "GTR"])
def test_partitioned_posterior_gradient_fd(model, C, clock, coalescent):
    post, _, _, _ = _partitioned_posterior(11, (14, 9, 17), model, C, clock, coalescent)
    assert post.K == 3 and post.param("relrates") is not None
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, post.dim)
    if post.param("rate") is not None:
        u[post.param("rate").sl] = math.log(0.3)
    check_grad(post, u)  # the tolerance tests/test_posterior.py holds the plain posterior to
    # mu: site-weighted mean 1
    vals, _, _ = post.constrain(u[None])
    mu = post.relative_rates(vals, 1)[0]
    assert abs(np.dot(mu, post.n_sites) / post.n_sites.sum() - 1.0) < 1e-14


@pytest.mark.parametrize("model,C,clock,coalescent", [("JC69", 1, None, None), ("HKY", 4, "strict", "constant"),
                                                      ("GTR", 3, None, None)],
                         ids=["JC69-noclock", "HKY+W4-strict", "GTR+W3"])
def test_one_partition_is_the_plain_posterior(model, C, clock, coalescent):
    part, spec, tree, case = _partitioned_posterior(13, (40,), model, C, clock, coalescent)
    plain = Posterior(spec, tree, OracleLikelihood(case.tipcodes, case.weights, case.peel0, clock is not None, model,
                                                   spec.C))
    assert part.param("relrates") is None and part.dim == plain.dim
    rng = np.random.default_rng(6)
    for _ in range(3):
        values = {p.name: p.tr.constrain(rng.uniform(-1.0, 1.0, (1, p.tr.size)))[0][0] for p in plain.params}
        up = plain.unconstrain(values)
        uq = part.unconstrain({(k + "_p1" if part.param(k + "_p1") is not None else k): v for k, v in values.items()})
        for propto in (True, False):
            lp, G = plain.log_prob_grad(up[None], propto=propto)
            lq, H = part.log_prob_grad(uq[None], propto=propto)
            # the same terms; the partitioned vector lists the tree's parameters first, so the transforms'
            # log-Jacobians add up in another order: a few ulps
            assert abs(lq[0] - lp[0]) <= 8 * np.spacing(abs(lp[0]))
            for p in plain.params:
                q = part.param(p.name + "_p1") or part.param(p.name)
                np.testing.assert_allclose(H[0, q.sl], G[0, p.sl], rtol=1e-13, atol=1e-13)


def test_columns_and_rows_agree():
    post, _, _, _ = _partitioned_posterior(11, (14, 9, 17), "HKY", 4, "strict", "constant")
    names = post.column_names()
    U = np.random.default_rng(2).uniform(-1, 1, (4, post.dim))
    rows = post.flat_rows(U)
    assert rows.shape == (4, len(names)) and len(set(names)) == len(names)
    # the tree's columns, then the partitions' blocks, then mu
    first_block = names.index("wshape_p1")
    assert all("_p" not in nm for nm in names[:first_block]) and "heights.6" in names[:first_block]
    assert names[-3:] == ["mu.1", "mu.2", "mu.3"]
    blocks = [nm for nm in names[first_block:-3]]
    per = len(blocks) // 3
    assert blocks[:per] == [nm.replace("_p2", "_p1") for nm in blocks[per:2 * per]]
    assert blocks[:per] == ["wshape_p1", "kappa_p1"] + ["freqs_p1.%d" % k for k in range(1, 5)] + \
        ["ps_p1.%d" % k for k in range(1, 5)] + ["rs_p1.%d" % k for k in range(1, 5)]
    vals, _, _ = post.constrain(U)
    np.testing.assert_array_equal(rows[:, names.index("kappa_p2")], vals["kappa_p2"])
    np.testing.assert_array_equal(rows[:, -3:], post.relative_rates(vals, 4))
    np.testing.assert_allclose(rows[:, -3:] @ post.n_sites / post.n_sites.sum(), 1.0, rtol=1e-14)


# -------------------------------------------------------------------- the CLI
def _run(argv, **kw):
    import argparse
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    arg = parser.parse_args(["run"] + argv)
    lines = []
    post = cli.run(arg, likelihood_factory=OracleLikelihood, log=lines.append, **kw)
    return post, lines


def _dataset(tmp_path):
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=6, sites=80, hetero=False)
    parts = _write(tmp_path, "DNA, first = 1-40\nDNA, second = 41-80\n")
    return t, a, parts


def test_run_partitions_vb(tmp_path, capsys):
    t, a, parts = _dataset(tmp_path)
    out = str(tmp_path / "vb")
    post, lines = _run(["-s", str(tmp_path / "x.stan"), "-m", "HKY", "-C", "2", "-t", t, "-i", a, "-o", out,
                        "--partitions", parts, "-S", "3", "--iter", "30", "--elbo_samples", "5", "--samples", "5"])
    assert any(s.startswith("Partition first: 40 sites, ") for s in lines)
    assert any(s.startswith("Partition second: 40 sites, ") for s in lines)
    header, data = stan_io.read_samples(out)
    assert header[1] == "blens.1" and data.shape == (6, len(header))
    for nm in ("wshape_p1", "kappa_p2", "freqs_p2.4", "rs_p1.2", "mu.1", "mu.2"):
        assert nm in header
    assert "kappa" not in header and header[-2:] == ["mu.1", "mu.2"]
    assert os.path.exists(out + ".diag") and open(out + ".trees").read().count("tree ") == 6
    tsv = [ln.split("\t") for ln in open(out + ".partitions.tsv").read().splitlines()]
    assert tsv[0] == ["partition", "sites", "patterns", "mu_mean", "mu_2.5%", "mu_97.5%"]
    assert [r[0] for r in tsv[1:]] == ["first", "second"] and [r[1] for r in tsv[1:]] == ["40", "40"]
    mu = data[1:, [header.index("mu.1"), header.index("mu.2")]]
    np.testing.assert_allclose(mu.mean(axis=1), 1.0, rtol=1e-5)  # the CSV holds six significant digits
    assert float(tsv[1][4]) <= float(tsv[1][3]) <= float(tsv[1][5])


def test_run_partitions_nuts(tmp_path, capsys):
    t, a, parts = _dataset(tmp_path)
    out = str(tmp_path / "nuts")
    _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "-t", t, "-i", a, "-o", out, "--partitions", parts,
          "-a", "nuts", "--iter", "20", "--chains", "2", "-S", "3"])
    for c in range(2):
        header, data = stan_io.read_samples(out + "_%d.csv" % c)
        assert header[7] == "blens.1" and header[-2:] == ["mu.1", "mu.2"] and data.shape[0] == 10
        assert os.path.exists(out + "_%d.trees" % c)
    assert len(open(out + ".partitions.tsv").read().splitlines()) == 3


@pytest.mark.parametrize("extra,what", [(["--geo"], "--geo"), (["--topologies", "tops.trees"], "--topologies"),
                                        (["--ancestral_seq"], "--ancestral_seq"), (["--rescaling"], "--rescaling")])
def test_run_partitions_refusals(tmp_path, extra, what):
    t, a, parts = _dataset(tmp_path)
    out = str(tmp_path / "no")
    with pytest.raises(SystemExit, match="--partitions is not supported with %s" % what):
        _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "-t", t, "-i", a, "-o", out, "--partitions", parts] + extra)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no")]


def test_run_partitions_bad_file(tmp_path):
    t, a, _ = _dataset(tmp_path)
    bad = _write(tmp_path, "DNA, first = 1-40\nDNA, second = 42-80\n")
    with pytest.raises(SystemExit, match="site 41 is in no partition"):
        _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "-t", t, "-i", a, "-o", str(tmp_path / "no"),
              "--partitions", bad])
