"""CPU: the forest's device-free parts -- the planner (csrc/forest_plan.h)
under host sanitizers, ``data.load_forest``, the lockstep mean-field ADVI and
``run --topologies`` on a host stand-in whose rows are the C oracle's."""
import argparse
import os
import subprocess

import numpy as np
import pytest

from phylostan_amd import cli, data as dataio, forest as fr, models, stan_io
from phylostan_amd.advi import ADVI
from phylostan_amd.posterior import ModelSpec, Posterior, TreeData
from tests import fixture_files, forest_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ planner
def test_forest_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "forest_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "forest_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    # all 42 DS1 peels in topology 0's tip order
    _, _, peels, _, _, _ = fc.ds1_forest()
    path = str(tmp_path / "ds1_peels.txt")
    with open(path, "w") as fp:
        fp.write("%d %d\n" % (peels.shape[1] + 1, peels.shape[0]))
        fp.write(" ".join(str(int(v)) for v in peels.reshape(-1)) + "\n")
    run = subprocess.run([exe, path], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert " 0 failures" in run.stdout and run.stdout.count("file forest: T 42") == 3


# -------------------------------------------------------------- load_forest
TAXA = ["t%d_%d" % (k, k) for k in range(6)]
NEWICKS = [
    "((t0_0,t1_1),((t2_2,t3_3),(t4_4,t5_5)));",
    "(t5_5,t3_3,((t1_1,t0_0),(t4_4,t2_2)));",           # a trifurcating root, another leaf order
    "(((((t0_0,t2_2),t4_4),t1_1),t3_3),t5_5);",
]


def _dataset(tmp_path, sites=40, seed=4):
    rng = np.random.default_rng(seed)
    tree = str(tmp_path / "first.tree")
    with open(tree, "w") as fp:
        fp.write(NEWICKS[0] + "\n")
    aln = str(tmp_path / "aln.fa")
    with open(aln, "w") as fp:
        for name in TAXA:
            fp.write(">%s\n%s\n" % (name, "".join(rng.choice(list("ACGT"), sites, p=[0.4, 0.2, 0.2, 0.2]))))
    tops = str(tmp_path / "tops.trees")
    with open(tops, "w") as fp:
        fp.write("\n".join(NEWICKS) + "\n")
    return tree, aln, tops


def test_load_forest(tmp_path):
    tree, aln, tops = _dataset(tmp_path)
    f = dataio.load_forest(tree, tops, aln)
    S = 6
    assert f.T == 3 and f.peels.shape == (3, S - 1, 3) and list(f.index) == [0, 1, 2]
    assert f.data.taxa == TAXA and f.tipcodes.shape[0] == S
    assert np.all(f.peels[:, -1, 1] == 2 * S - 3)  # the unrooted last-row rule, tree by tree
    for k, nwk in enumerate(NEWICKS):  # each tree on its own through data.load, tips remapped by label
        own = str(tmp_path / ("own%d.tree" % k))
        with open(own, "w") as fp:
            fp.write(nwk + "\n")
        d = dataio.load(own, aln, rooted=False)
        to_common = np.array([TAXA.index(lab) for lab in d.taxa] + list(range(S, 2 * S - 1)))
        np.testing.assert_array_equal(f.peels[k], to_common[d.peel0])
    # a selection keeps the file's indices
    sel = dataio.load_forest(tree, tops, aln, burnin=0.34)
    assert list(sel.index) == [1, 2]
    np.testing.assert_array_equal(sel.peels, f.peels[1:])
    # a foreign taxon names its tree
    bad = str(tmp_path / "bad.trees")
    with open(bad, "w") as fp:
        fp.write(NEWICKS[0] + "\n" + NEWICKS[2].replace("t4_4", "zz_9") + "\n")
    with pytest.raises(ValueError, match="tree 1"):
        dataio.load_forest(tree, bad, aln)


# ---------------------------------------------------------------- stand-ins
def oracle_evaluator(tip, w, peel, kind, C):
    from oracle import cpu

    def ev(bl, mv, site_ll):
        return cpu.evaluate(tip, w, peel, False, kind, mv, bl, C, site_ll=site_ll)
    return ev


def rejecting_evaluator(outlen):
    def ev(bl, mv, site_ll):
        row = np.zeros(outlen)
        row[0] = -np.inf
        return row, None
    return ev


def host_forest(tip, w, peels, rooted, model, C, reject=()):
    assert not rooted
    kind = models.MODEL_IDS[model]
    S, P = tip.shape
    B = 2 * S - 3
    evs = [rejecting_evaluator(1 + B + 2 * C + 14) if t in reject else oracle_evaluator(tip, w, peels[t], kind, C)
           for t in range(len(peels))]
    return fr.forest_host(evs, B, C, P)


class SingleTree:
    """Tree t of a forest as a single-tree likelihood (``evaluate_rows(blens, mv)``)."""

    def __init__(self, forest, t):
        self.forest, self.t = forest, t

    def evaluate_rows(self, blens, mv):
        blens = np.atleast_2d(blens)
        return self.forest.evaluate_rows(np.full(blens.shape[0], self.t), blens, mv)


def _problem(tmp_path, model, C):
    tree, aln, tops = _dataset(tmp_path)
    f = dataio.load_forest(tree, tops, aln)
    spec = ModelSpec(model=model, categories=C)
    td = TreeData(f.S, f.data.peel0, f.data.map, None, None)
    return f, spec, td


ADVI_KW = dict(grad_samples=1, elbo_samples=10, eval_elbo=50)
RUN_KW = dict(tol_rel_obj=0.001, max_iterations=300)


def _same(a, b):
    assert a.error is None and b.error is None
    assert a.iterations == b.iterations and a.eta == b.eta
    np.testing.assert_array_equal(a.q.mu, b.q.mu)
    np.testing.assert_array_equal(a.q.omega, b.q.omega)
    assert [(it, e) for it, _, e in a.trace] == [(it, e) for it, _, e in b.trace] and len(a.trace) >= 2
    np.testing.assert_array_equal(a.draws, b.draws)


@pytest.mark.parametrize("model,C", [("JC69", 1), ("HKY", 2)])
def test_lockstep_advi_equals_solo_runs(tmp_path, model, C):
    f, spec, td = _problem(tmp_path, model, C)
    forest = host_forest(f.tipcodes, f.weights, f.peels, False, model, C)
    post = Posterior(spec, td, fr.TaggedLikelihood(forest))
    full = fr.lockstep_advi(post, range(3), 11, samples=5, **ADVI_KW, **RUN_KW)
    for t in range(3):
        # the run on {t} alone: the other topologies change nothing
        alone = fr.lockstep_advi(post, [t], 11, samples=5, **ADVI_KW, **RUN_KW)
        _same(full[t], alone[t])
        # ADVI.run itself on a single-tree likelihood, with the same generator
        solo_post = Posterior(spec, td, SingleTree(forest, t))
        rng = np.random.default_rng((11, t))
        trace = []
        adv = ADVI(solo_post, rng, log=None, **ADVI_KW)
        q0 = solo_post.initialize(rng)
        q, eta, iters = adv.run(q0, diag=lambda it, sec, elbo: trace.append((it, elbo)), **RUN_KW)
        assert (iters, eta) == (full[t].iterations, full[t].eta)
        np.testing.assert_array_equal(q.mu, full[t].q.mu)
        np.testing.assert_array_equal(q.omega, full[t].q.omega)
        assert trace == [(it, e) for it, _, e in full[t].trace]
        np.testing.assert_array_equal(q.sample(rng, 5), full[t].draws)
    assert len({full[t].q.mu.tobytes() for t in range(3)}) == 3  # three different optimisations


def test_lockstep_a_failing_topology_ends_alone(tmp_path):
    f, spec, td = _problem(tmp_path, "JC69", 1)
    good = host_forest(f.tipcodes, f.weights, f.peels, False, "JC69", 1)
    bad = host_forest(f.tipcodes, f.weights, f.peels, False, "JC69", 1, reject=(1,))
    ref = fr.lockstep_advi(Posterior(spec, td, fr.TaggedLikelihood(good)), [0, 2], 3, **ADVI_KW, **RUN_KW)
    got = fr.lockstep_advi(Posterior(spec, td, fr.TaggedLikelihood(bad)), range(3), 3, **ADVI_KW, **RUN_KW)
    assert got[1].q is None and got[1].error
    for t in (0, 2):
        _same(got[t], ref[t])


def test_tags_reach_the_likelihood_and_change_nothing_else(tmp_path):
    f, spec, td = _problem(tmp_path, "HKY", 2)
    forest = host_forest(f.tipcodes, f.weights, f.peels, False, "HKY", 2)
    tagged = Posterior(spec, td, fr.TaggedLikelihood(forest))
    rng = np.random.default_rng(0)
    U = rng.uniform(-2, 2, (7, tagged.dim))
    U[3, 0] = np.inf  # out of support: dropped before the likelihood, its tag with it
    tags = np.array([0, 1, 2, 1, 2, 0, 1], np.int32)
    lp, G = tagged.log_prob_grad(U, tags=tags)
    assert lp[3] == -np.inf and not G[3].any()
    for t in range(3):
        single = Posterior(spec, td, SingleTree(forest, t))
        rows = tags == t
        lp1, G1 = single.log_prob_grad(U[rows])            # tags=None: the path as it was
        lp2, G2 = single.log_prob_grad(U[rows], tags=None)
        np.testing.assert_array_equal(lp1, lp2)
        np.testing.assert_array_equal(G1, G2)
        np.testing.assert_array_equal(lp[rows], lp1)
        np.testing.assert_array_equal(G[rows], G1)
    with pytest.raises(ValueError, match="tags"):
        tagged.log_prob_grad(U)


# ---------------------------------------------------------------------- CLI
def _args(argv):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    return parser.parse_args(["run"] + argv)


def test_cli_topologies_on_the_stand_in(tmp_path):
    tree, aln, tops = _dataset(tmp_path)
    out = str(tmp_path / "ds")
    base = ["-s", str(tmp_path / "m.stan"), "-m", "JC69", "-t", tree, "-i", aln, "-o", out, "-S", "5", "--iter", "200",
            "--elbo_samples", "10", "--samples", "20", "--topologies", tops]
    lines = []
    post, results = cli.run(_args(base), likelihood_factory=host_forest, log=lines.append)
    assert sorted(results) == [0, 1, 2]
    rows = [ln.split("\t") for ln in open(out + ".topologies.tsv").read().splitlines()]
    assert rows[0] == ["tree", "iterations", "converged", "eta", "elbo", "log_ml_is", "posterior"]
    assert [int(r[0]) for r in rows[1:]] == [0, 1, 2]
    probs = np.array([float(r[6]) for r in rows[1:]])
    elbos = np.array([float(r[4]) for r in rows[1:]])
    assert abs(probs.sum() - 1.0) < 1e-12 and np.all(np.isfinite(elbos)) and np.all(probs > 0)
    w = np.exp(elbos - elbos.max())
    np.testing.assert_allclose(probs, w / w.sum(), rtol=1e-12)
    f = dataio.load_forest(tree, tops, aln)
    forest = host_forest(f.tipcodes, f.weights, f.peels, False, "JC69", 1)
    for k in range(3):
        path = "%s_tree%d" % (out, k)
        header, data = stan_io.read_samples(path)
        assert header[0] == "lp__" and data.shape == (21, len(header))
        assert open(path + ".diag").read().count("\n") >= 3
        assert open(path + ".trees").read().count("tree ") == 21
        r = results[k]
        # the written draws are the result's; the ELBO is mean log p + entropy over them, on tree k alone
        np.testing.assert_allclose(data[1:, 1:], post.flat_rows(r.draws), rtol=1e-5)
        single = Posterior(post.spec, post.tree, SingleTree(forest, k))
        lp = single.log_prob(r.draws, propto=False)
        assert np.all(np.isfinite(lp))
        assert abs(float(lp.sum()) / 20 + r.q.entropy() - elbos[k]) <= 1e-12 * abs(elbos[k])
        lw = lp - cli.meanfield_log_q(r.q, r.draws)
        lml = lw.max() + np.log(np.exp(lw - lw.max()).sum() / 20)
        assert abs(lml - float(rows[1 + k][5])) <= 1e-12 * abs(lml)
        assert int(rows[1 + k][1]) == r.iterations and float(rows[1 + k][3]) == r.eta
    # --samples 0: the last ELBO of the run
    out0 = str(tmp_path / "ds0")
    argv0 = [a for a in base]
    argv0[argv0.index("-o") + 1] = out0
    argv0[argv0.index("--samples") + 1] = "0"
    _, res0 = cli.run(_args(argv0), likelihood_factory=host_forest, log=lines.append)
    rows0 = [ln.split("\t") for ln in open(out0 + ".topologies.tsv").read().splitlines()][1:]
    assert [float(r[4]) for r in rows0] == [res0[k].trace[-1][2] for k in range(3)]


@pytest.mark.parametrize("extra,what", [(["--clock", "strict"], "--clock"), (["-a", "nuts"], "-a nuts"),
                                        (["-a", "hmc"], "-a hmc"), (["-q", "fullrank"], "-q fullrank"),
                                        (["--geo"], "--geo"), (["--rescaling"], "--rescaling")])
def test_cli_topologies_refusals(tmp_path, extra, what):
    tree, aln, tops = _dataset(tmp_path)
    argv = ["-s", str(tmp_path / "m.stan"), "-m", "JC69", "-t", tree, "-i", aln, "-o", str(tmp_path / "x"),
            "--topologies", tops] + extra
    with pytest.raises(SystemExit, match="%s is not supported with --topologies" % what):
        cli.run(_args(argv), likelihood_factory=host_forest, log=lambda *_: None)
    bad = str(tmp_path / "bad.trees")
    with open(bad, "w") as fp:
        fp.write(NEWICKS[0] + "\n" + NEWICKS[1].replace("t3_3", "other_1") + "\n")
    argv[argv.index("--topologies") + 1] = bad
    with pytest.raises(SystemExit, match="tree 1"):
        cli.run(_args(argv[:len(argv) - len(extra)]), likelihood_factory=host_forest, log=lambda *_: None)
