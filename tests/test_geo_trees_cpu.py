"""CPU: phylogeography over a tree sample (the mixture likelihood) above the
kernel: ``geo.geo_trees_host`` / ``geo_trees_summaries_host`` against the truth
of tests/geo_trees_truth.py (complex log-sum-exp of per-tree expm likelihoods,
complex-step derivatives, p_t-weighted Minin-Suchard counts and root
marginals), ``treeio.read_trees`` and ``geo.tree_sample``, ``run --geo --trees``
end to end on a host likelihood, the declared boundary, and the device-free
planner under host sanitizers (tests/geo_trees_check.cpp).  The device:
tests/test_geo_trees_gpu.py.

Bars (the project's): log L_mix and every finite tree log L at relative 1e-10,
each gradient array, ``jumps`` and ``root`` within 1e-9 of the array's largest
entry; at K = 2 the rate gradient is exactly zero and compared absolutely.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import cli, geo, stan_io, treeio
from tests import geo_oracle as go
from tests import geo_summary_truth as gst
from tests import geo_trees_truth as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LL_BAR, GRAD_BAR, K2_RATE_BAR = 1e-10, 1e-9, 1e-12


def check_host(tips, peels, blens, params, logw, entries=None):
    K = tips.shape[1]
    rates, freqs = gt.split_params(params, K)
    ll, gr, gf, tll = geo.geo_trees_host(tips, peels, blens, rates, freqs, logw)
    tl, tlls, tg = gt.mix_truth_gradients(tips, peels, blens, rates, freqs,
                                          gt.uniform_logw(len(peels)) if logw is None else logw, max_entries=entries)
    assert abs(ll - tl) <= LL_BAR * abs(tl)
    assert np.all(np.abs(tll - tlls) <= LL_BAR * np.abs(tlls))
    for name, got in (("rates", gr), ("freqs", gf)):
        idx, want = tg[name]
        if name == "rates" and K == 2:
            assert np.abs(got).max() <= K2_RATE_BAR and np.abs(want).max() <= K2_RATE_BAR
            continue
        assert np.abs(got[idx] - want).max() <= GRAD_BAR * np.abs(got).max(), name
    return ll, gr, gf, tll


@pytest.mark.parametrize("T", [1, 2, 3, 7])
@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("S", [4, 7])
def test_host_mixture_against_the_truth(S, K, T):
    """S = 4: its three topologies in turn; S = 7: a caterpillar, a balanced
    tree, then random ones.  Odd T gets unequal weights."""
    tips, peels, blens, params = gt.make_sample(S, K, T, 1000 * S + 10 * K + T)
    logw = gt.uniform_logw(T) if T % 2 == 0 else np.log(np.random.default_rng(T).dirichlet(np.ones(T)))
    check_host(tips, peels, blens, params, None if T % 2 == 0 else logw)
    if T % 2 == 0:  # the default weights are 1 / T
        a = geo.geo_trees_host(tips, peels, blens, *gt.split_params(params, K))
        b = geo.geo_trees_host(tips, peels, blens, *gt.split_params(params, K), log_weights=logw)
        assert a[0] == b[0]


@pytest.mark.parametrize("S,K", [(4, 2), (7, 5)])
def test_one_tree_is_the_single_tree_row(S, K):
    tips, peels, blens, params = gt.make_sample(S, K, 1, 50 + S)
    rates, freqs = gt.split_params(params, K)
    ll, gr, gf, tll = geo.geo_trees_host(tips, peels, blens, rates, freqs)
    l1, _, r1, f1 = geo.geo_gradients_host(tips, peels[0], blens[0], rates, freqs)
    assert abs(ll - l1) <= LL_BAR * abs(l1) and abs(tll[0] - l1) <= LL_BAR * abs(l1)
    if K > 2:
        assert np.abs(gr - r1).max() <= GRAD_BAR * np.abs(r1).max()
    else:
        assert np.abs(gr).max() <= K2_RATE_BAR
    assert np.abs(gf - f1).max() <= GRAD_BAR * np.abs(f1).max()
    jumps, root = geo.geo_trees_summaries_host(tips, peels, blens, rates, freqs)
    marg, j1, _ = geo.geo_summaries_host(tips, peels[0], blens[0], rates, freqs)
    assert np.abs(jumps - j1).max() <= GRAD_BAR * np.abs(j1).max()
    assert np.abs(root - marg[-1]).max() <= GRAD_BAR


@pytest.mark.parametrize("S,K,T", [(4, 3, 3), (7, 5, 3), (7, 2, 2)])
def test_host_summaries_against_the_truth(S, K, T):
    tips, peels, blens, params = gt.make_sample(S, K, T, 7000 + S + K)
    rates, freqs = gt.split_params(params, K)
    logw = np.log(np.random.default_rng(S).dirichlet(np.ones(T)))
    jumps, root = geo.geo_trees_summaries_host(tips, peels, blens, rates, freqs, logw)
    tj, tr, p = gt.summaries_truth(tips, peels, blens, rates, freqs, logw)
    assert np.abs(jumps - tj).max() <= GRAD_BAR * np.abs(tj).max()
    assert np.abs(root - tr).max() <= GRAD_BAR * tr.max()
    assert abs(root.sum() - 1.0) <= 1e-12
    assert abs(np.trace(jumps) - p @ blens.sum(1)) <= 1e-9 * blens.sum(1).max()


def test_root_truth_is_the_enumerated_marginal():
    tips, peels, blens, params = gt.make_sample(4, 3, 3, 11)
    rates, freqs = gt.split_params(params, 3)
    for t in range(3):
        brute = gst.brute_marginals(tips, peels[t], blens[t], rates, freqs)
        assert np.abs(gt.root_truth(tips, peels[t], blens[t], rates, freqs) - brute[-1]).max() <= 1e-12


def test_a_tree_without_likelihood_has_no_weight():
    """A branch of -1e6 on tree 0: e^{lam t} overflows and that tree's
    likelihood is not finite; it gets -inf and weight 0, the mixture is the
    other trees'.  A tip whose partial is all zeros: L = 0 on every tree."""
    S, K = 4, 3
    tips = np.eye(K)[[0, 1, 2, 0]]
    peels = gt.S4_PEELS
    rng = np.random.default_rng(3)
    blens = rng.exponential(0.3, (3, 5))
    blens[0, 2] = -1e6
    _, params = go.random_draws(1, 5, K, rng)
    rates, freqs = gt.split_params(params[0], K)
    with np.errstate(all="ignore"):
        ll, gr, gf, tll = geo.geo_trees_host(tips, peels, blens, rates, freqs)
    assert tll[0] == -np.inf and np.all(np.isfinite(tll[1:]))
    l2, r2, f2, _ = geo.geo_trees_host(tips, peels[1:], blens[1:], rates, freqs, np.full(2, -np.log(3.0)))
    assert ll == l2 and np.array_equal(gr, r2) and np.array_equal(gf, f2)
    dead = tips.copy()
    dead[3] = 0.0
    with np.errstate(all="ignore"):
        none = geo.geo_trees_host(dead, peels[1:], blens[1:], rates, freqs)
    assert none[0] == -np.inf and not none[1].any() and not none[2].any() and np.all(none[3] == -np.inf)
    bad = geo.geo_trees_host(tips, peels, blens, rates, np.array([0.5, 0.5, 0.0]))
    assert bad[0] == -np.inf and np.all(bad[3] == -np.inf)


# ---------------------------------------------------------------- files
def newick(peel, edge, labels, rng):
    """Newick text of a peel with per-node edge lengths, children in random order."""
    S = len(labels)
    text = {n: labels[n] for n in range(S)}
    for a, b, p in peel:
        if p != 2 * S - 2 and rng.random() < 0.5:  # the root keeps its order: its second child is where the root sits
            a, b = b, a
        text[p] = "(%s:%.8f,%s:%.8f)" % (text[a], edge[a], text[b], edge[b])
    return text[2 * S - 2] + ";"


def random_sample_text(S, T, seed, labels=None):
    """T random trees: (peels, merged blens [T, 2S-3], newick strings)."""
    rng = np.random.default_rng(seed)
    labels = ["t%d" % (n + 1) for n in range(S)] if labels is None else labels
    peels, blens, texts = [], [], []
    for _ in range(T):
        peel = go.random_peel(S, rng)
        edge = rng.exponential(0.3, 2 * S - 1)
        bl = edge.copy()
        bl[peel[-1][0]] += bl[peel[-1][1]]
        peels.append(peel)
        blens.append(bl[:2 * S - 3])
        texts.append(newick(peel, edge, labels, rng))
    return np.stack(peels), np.stack(blens), texts


def same_trees(tips, params, peels_a, blens_a, peels_b, blens_b):
    """Two descriptions of the same trees: the same likelihood at a parameter point."""
    K = tips.shape[1]
    rates, freqs = gt.split_params(params, K)
    for t in range(len(peels_a)):
        la = go.truth(tips, peels_a[t], blens_a[t], rates, freqs).real
        lb = go.truth(tips, peels_b[t], blens_b[t], rates, freqs).real
        assert abs(la - lb) <= 1e-7 * abs(la), t  # the file holds 8 decimals of every length


def test_read_trees_newick_in_any_leaf_order(tmp_path):
    S, K, T = 6, 3, 4
    peels, blens, texts = random_sample_text(S, T, 21)
    path = tmp_path / "sample.nwk"
    path.write_text("\n".join(t.replace(",", ",\n", 1) for t in texts) + "\n")  # trees broken over lines
    trees = treeio.read_trees(str(path))
    assert len(trees) == T
    orders = {tuple(leaf.taxon.label for leaf in tr.leaf_node_iter()) for tr in trees}
    assert len(orders) > 1  # the trees list their leaves in different orders
    taxa = ["t%d" % (n + 1) for n in range(S)]
    got_peels, got_blens = geo.tree_sample(trees, taxa)
    assert got_peels.shape == (T, S - 1, 3) and got_blens.shape == (T, 2 * S - 3)
    assert np.all(got_peels[:, -1, 1] == 2 * S - 3) and np.all(got_peels[:, -1, 2] == 2 * S - 2)
    rng = np.random.default_rng(1)
    tips = go.random_tips(S, K, rng, missing=())
    _, params = go.random_draws(1, 2 * S - 3, K, rng)
    same_trees(tips, params[0], peels, blens, got_peels, got_blens)
    assert len(treeio.read_trees(str(path))) == T and treeio.read_tree(str(path)) is not None


def test_read_trees_nexus_with_a_translate_block(tmp_path):
    S, K, T = 5, 3, 3
    taxa = ["A_1", "B_2", "C_3", "D_4", "E_5"]
    peels, blens, texts = random_sample_text(S, T, 22, labels=[str(n + 1) for n in range(S)])
    body = "#NEXUS\nBegin taxa;\n Dimensions ntax=%d;\n Taxlabels %s;\nEnd;\nBegin trees;\n Translate\n" % (S, " ".join(taxa))
    body += ",\n".join("  %d %s" % (n + 1, taxa[n]) for n in range(S)) + ";\n"
    body += "".join("tree STATE_%d = [&R] %s\n" % (t, texts[t]) for t in range(T)) + "End;\n"
    path = tmp_path / "sample.trees"
    path.write_text(body)
    trees = treeio.read_trees(str(path))
    assert len(trees) == T and [t.label for t in trees[0].taxon_namespace] == taxa
    got_peels, got_blens = geo.tree_sample(trees, taxa)
    rng = np.random.default_rng(2)
    tips = go.random_tips(S, K, rng, missing=())
    _, params = go.random_draws(1, 2 * S - 3, K, rng)
    same_trees(tips, params[0], peels, blens, got_peels, got_blens)
    # tips are numbered by `taxa`, not by the file: reversing taxa reverses the tip ids
    rev_peels, rev_blens = geo.tree_sample(treeio.read_trees(str(path)), taxa[::-1])
    rates, freqs = gt.split_params(params[0], K)
    for t in range(T):
        la = go.truth(tips, peels[t], blens[t], rates, freqs).real
        lb = go.truth(tips[::-1], rev_peels[t], rev_blens[t], rates, freqs).real
        assert abs(la - lb) <= 1e-7 * abs(la), t


def test_tree_sample_refusals(tmp_path):
    taxa = ["a", "b", "c", "d"]
    ok = "((a:0.1,b:0.2):0.1,(c:0.3,d:0.1):0.2);"
    path = tmp_path / "s.nwk"
    path.write_text(ok + "\n((a:0.1,b:0.2):0.1,(c:0.3,x:0.1):0.2);\n")
    with pytest.raises(ValueError, match=r"tree 1: .*not the 4 taxa"):
        geo.tree_sample(treeio.read_trees(str(path)), taxa)
    path.write_text(ok + "\n" + ok + "\n((a:0.1,b):0.1,(c:0.3,d:0.1):0.2);\n")
    with pytest.raises(ValueError, match=r"tree 2: negative or missing branch length"):
        geo.tree_sample(treeio.read_trees(str(path)), taxa)
    path.write_text("((a:0.1,b:-0.2):0.1,(c:0.3,d:0.1):0.2);\n")
    with pytest.raises(ValueError, match=r"tree 0: negative or missing"):
        geo.tree_sample(treeio.read_trees(str(path)), taxa)
    path.write_text("((a:0.1,b:0.2):0.1,c:0.3);\n")
    with pytest.raises(ValueError, match=r"tree 0: its 3 leaves"):
        geo.tree_sample(treeio.read_trees(str(path)), taxa)


def test_select_trees():
    assert list(geo.select_trees(8)) == list(range(8))
    assert list(geo.select_trees(8, 0.25)) == [2, 3, 4, 5, 6, 7]
    assert list(geo.select_trees(8, 0.25, 3)) == [2, 4, 6]
    assert list(geo.select_trees(10, 0.5, 2)) == [5, 7]
    assert list(geo.select_trees(5, 0.0, 9)) == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError):
        geo.select_trees(5, 1.0)


# ---------------------------------------------------------------- the CLI
def write_dataset(tmp_path, S, K, T, seed):
    """The dataset of tests/geo_oracle.py and a sample of T trees on its taxa:
    two random topologies, the rest the dataset's own tree with every length
    rescaled at random."""
    tree, meta = go.write_geo_dataset(str(tmp_path), S=S, K=K, seed=seed)
    _, _, texts = random_sample_text(S, min(T, 2), seed + 1)
    rng = np.random.default_rng(seed + 2)
    own = open(tree).read().strip()
    for _ in range(T - len(texts)):
        texts.append(re.sub(r":([0-9.]+)", lambda m: ":%.6f" % (float(m.group(1)) * rng.uniform(0.5, 1.5)), own))
    sample = str(tmp_path / "sample.nwk")
    with open(sample, "w") as fp:
        fp.write("\n".join(texts) + "\n")
    return tree, meta, sample


class Recording(gt.HostGeoTreesLikelihood):
    made = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        Recording.made.append(self)


def test_run_geo_trees_vb_writes_the_sample(tmp_path, capsys):
    S, K, T = 8, 3, 4
    tree, meta, sample = write_dataset(tmp_path, S, K, T, 4)
    out = str(tmp_path / "geo")
    Recording.made = []
    post, lines = go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "-t", tree, "--trees", sample, "-o", out,
                              "-S", "5", "--iter", "200", "--elbo_samples", "10", "--samples", "20",
                              "--tol_rel_obj", "0.01"], factory=Recording)
    assert isinstance(post, geo.GeoTreesPosterior) and post.dim == 3 + 2
    assert len(Recording.made) == 1 and Recording.made[0].T == T
    header, data = stan_io.read_samples(out)
    assert header[0] == "lp__" and "rates_geo.1" in header and header[-1] == "freqs_geo.3"
    assert data.shape[0] >= 20 and np.all(np.isfinite(data[:, header.index("rates_geo.1"):]))
    assert [s for s in lines if s.startswith("Tree sample: 4 of the 4 trees")]
    for ext in (".trees", ".jumps.tsv", ".root.tsv", ".treeprob.tsv"):
        assert not os.path.exists(out + ext)
    capsys.readouterr()


def test_run_geo_trees_ancestral_selects_and_writes(tmp_path, capsys):
    S, K, T = 8, 3, 8
    tree, meta, sample = write_dataset(tmp_path, S, K, T, 4)
    out = str(tmp_path / "geo")
    Recording.made = []
    post, lines = go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree,
                              "--trees", sample, "--trees_burnin", "0.25", "--trees_max", "3", "-o", out, "-S", "5",
                              "--iter", "200", "--elbo_samples", "10", "--samples", "12", "--tol_rel_obj", "0.01"],
                             factory=Recording)
    lik = Recording.made[0]
    assert lik.T == 3
    # the documented selection: trees 2, 4, 6 of the file, with the taxa of -t
    taxa = [t.label for t in treeio.read_tree(tree).taxon_namespace]
    all_trees = treeio.read_trees(sample)
    want_peels, want_blens = geo.tree_sample([all_trees[i] for i in (2, 4, 6)], taxa)
    assert np.array_equal(lik.peels, want_peels) and np.array_equal(lik.blens, want_blens)
    assert not os.path.exists(out + ".trees")
    rows = [ln.rstrip("\n").split("\t") for ln in open(out + ".treeprob.tsv")]
    assert rows[0] == ["tree", "probability"] and [r[0] for r in rows[1:]] == ["2", "4", "6"]
    probs = np.array([float(r[1]) for r in rows[1:]])
    assert np.all(probs >= 0.0) and abs(probs.sum() - 1.0) <= 1e-12
    rows = [ln.rstrip("\n").split("\t") for ln in open(out + ".root.tsv")]
    assert rows[0] == ["location", "probability"] and [r[0] for r in rows[1:]] == ["P0", "P1", "P2"]
    assert abs(sum(float(r[1]) for r in rows[1:]) - 1.0) <= 1e-12
    jt = [ln.rstrip("\n").split("\t") for ln in open(out + ".jumps.tsv")]
    assert jt[0] == ["from\\to", "P0", "P1", "P2", "time"] and len(jt) == 1 + K
    times = sum(float(r[-1]) for r in jt[1:])
    assert want_blens.sum(1).min() - 1e-9 <= times <= want_blens.sum(1).max() + 1e-9
    summary = [s for s in lines if s.startswith("Expected migrations")]
    assert len(summary) == 1 and re.search(r"over \d+ draws and 3 trees; root location: P\d", summary[0])
    capsys.readouterr()


def test_trees_refusals(tmp_path):
    tree, meta, sample = write_dataset(tmp_path, 6, 3, 2, 7)
    out = str(tmp_path / "o")
    with pytest.raises(SystemExit, match="needs --geo"):
        go.run_geo(["-s", str(tmp_path / "m.stan"), "-t", tree, "--trees", sample, "-o", out], factory=Recording)
    other = tmp_path / "other.nwk"
    other.write_text("((a:1,b:1):1,(c:1,d:1):1);\n")
    with pytest.raises(SystemExit, match="--trees: tree 0"):
        go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "-t", tree, "--trees", str(other), "-o", out],
                   factory=Recording)


# ---------------------------------------------------------------- the boundary and the planner
def test_boundary_is_declared_and_bound():
    from phylostan_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_geo.h")).read(), flags=re.S)
    new = ("phy_geo_trees_create", "phy_geo_trees_destroy", "phy_geo_trees_num_trees", "phy_geo_trees_output_len",
           "phy_geo_trees_summary_len", "phy_geo_trees_eval", "phy_geo_trees_eval_summaries")
    old = ("phy_geo_create", "phy_geo_destroy", "phy_geo_num_branches", "phy_geo_output_len", "phy_geo_eval",
           "phy_geo_summary_len", "phy_geo_eval_summaries")
    for name in new + old:
        assert re.search(r"\bint\s+%s\s*\(" % name, text), name
        assert name in _lib.GEO_SIGNATURES
    assert "typedef struct phy_geo_trees_ctx phy_geo_trees_ctx;" in text
    assert len(_lib.GEO_SIGNATURES["phy_geo_trees_create"][1]) == 10
    diag = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_diag.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+phy_geo_trees_info\s*\(", diag) and "phy_geo_trees_info" in _lib.SIGNATURES
    top = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip.h")).read(), flags=re.S)
    assert "phy_geo_trees" not in top  # phylo_hip.h itself declares what it did
    src = open(os.path.join(ROOT, "phylostan_amd", "csrc", "phylo_hip.hip")).read()
    assert src.index('#include "geo_engine.inc"') < src.index('#include "geo_trees.inc"')
    plan = open(os.path.join(ROOT, "phylostan_amd", "csrc", "geo_plan.h")).read()
    assert "hip/" not in plan


def test_trees_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "geo_trees_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "geo_trees_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "0 failures" in run.stdout
