"""CPU: the codon model (``phylostan_amd.codon``) -- the genetic code, the
codon alignment and its refusals, ``codon_rates`` and the frequency models with
their exact transposes, ``CodonPosterior`` against central differences, and
``run --codon`` end to end on the host likelihood."""
import argparse
import math
import os

import numpy as np
import pytest

from phylostan_amd import cli, codon, data as dataio, stan_io
from phylostan_amd.kseq import HostKStateLikelihood
from phylostan_amd.posterior import ModelSpec, TreeData
from tests import cases, fixture_files, kseq_truth as kt
from tests.test_posterior import check_grad, preorder_map

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STEP = 1e-30


def _chars(rows):
    return np.stack([np.frombuffer(r.encode("ascii"), np.uint8) for r in rows])


# ------------------------------------------------------------ code and data
def test_genetic_code():
    assert codon.K == 61 and len(codon.CODONS) == 61 and codon.CODONS[0] == "TTT" and codon.CODONS[-1] == "GGG"
    assert sorted(codon.CODONS64[i] for i in codon.STOPS) == ["TAA", "TAG", "TGA"]
    assert "".join(codon.AMINO).count("L") == 6 and codon.AMINO[codon.CODONS.index("ATG")] == "M"
    assert codon.AMINO[codon.CODONS.index("TGG")] == "W"


def test_fluA_reads_as_codons():
    base = os.path.join(ROOT, "tests", "golden", "examples", "fluA")
    d = dataio.load(os.path.join(base, "fluA.tree"), os.path.join(base, "fluA.fa"), rooted=True)
    chars = dataio.alignment_matrix(dataio.read_alignment(os.path.join(base, "fluA.fa")), d.tree.taxon_namespace)
    assert chars.shape == (69, 987)
    masks, weights, pattern = codon.codon_alignment(chars, d.taxa)
    assert masks.shape == (69, 242) and weights.sum() == 329 and pattern.shape == (329,)
    assert pattern[0] == 0 and pattern.max() == 241 and np.all(np.bincount(pattern) == weights)
    assert np.all(masks != 0) and np.all(masks < np.uint64(1 << 61))
    # frames 1 and 2 are full of stop codons
    for shift in (1, 2):
        with pytest.raises(ValueError, match="stop codon"):
            codon.codon_alignment(chars[:, shift:shift + 984], d.taxa)


def test_alignment_refusals_name_taxon_and_site():
    rows = ["ATGGCCAAA", "ATGGCTAAA", "ATGGCCAAG"]
    masks, w, _ = codon.codon_alignment(_chars(rows))
    assert masks.shape == (3, 3) and list(w) == [1.0, 1.0, 1.0]
    with pytest.raises(ValueError, match="986 is not a multiple of 3"):
        codon.codon_alignment(np.full((3, 986), ord("A"), np.uint8))
    planted = [rows[0], "ATGTAAAAA", rows[2]]
    with pytest.raises(ValueError, match="second site 4: TAA is an in-frame stop codon"):
        codon.codon_alignment(_chars(planted), ["first", "second", "third"])
    with pytest.raises(ValueError, match="taxon 3 site 7: TAR is compatible only with stop codons"):
        codon.codon_alignment(_chars([rows[0], rows[1], "ATGGCCTAR"]))
    with pytest.raises(ValueError, match="is not a nucleotide symbol"):
        codon.codon_alignment(_chars([rows[0], rows[1], "ATGGCCAAZ"]))


def test_masks_of_ambiguous_triplets():
    acn = codon.triplet_mask("ACN")
    assert bin(acn).count("1") == 4
    assert [codon.CODONS[j] for j in range(61) if (acn >> j) & 1] == ["ACT", "ACC", "ACA", "ACG"]
    assert codon.triplet_mask("TAR") == 0  # TAA, TAG: stop only
    assert bin(codon.triplet_mask("TAN")).count("1") == 2  # TAT, TAC: the stops drop out
    assert codon.triplet_mask("---") == (1 << 61) - 1 and codon.triplet_mask("NNN") == (1 << 61) - 1
    assert codon.triplet_mask("ATG") == 1 << codon.CODONS.index("ATG")
    masks, w, pat = codon.codon_alignment(_chars(["ACNACN---", "ACGACG---", "ACAACAATG"]))
    assert masks.shape == (3, 2) and list(w) == [2.0, 1.0] and list(pat) == [0, 0, 1]  # first-seen order, counts
    assert masks[0, 0] == np.uint64(acn) and masks[0, 1] == np.uint64((1 << 61) - 1)


def test_codon_counts_take_unambiguous_codons():
    masks, w, _ = codon.codon_alignment(_chars(["ATGATGACN", "ATGATGACG"]))
    counts = codon.codon_counts(masks, w)
    assert counts[codon.CODONS.index("ATG")] == 4 and counts[codon.CODONS.index("ACG")] == 1 and counts.sum() == 5


# ------------------------------------------------------- rates and frequencies
def test_codon_rates_structure():
    x6 = np.asarray([1.1, 5.0, 0.9, 1.2, 4.0, 1.0])
    r = codon.codon_rates(x6, 0.3)
    assert r.shape == (61 * 60 // 2,) and np.count_nonzero(r) == 263
    from phylostan_amd.geo import rate_pairs
    pairs = rate_pairs(61)
    at = {(codon.CODONS[a], codon.CODONS[b]): r[k] for k, (a, b) in enumerate(pairs)}
    get = lambda a, b: at.get((a, b), at.get((b, a)))  # noqa: E731
    assert get("TTT", "TTC") == x6[4]            # C <-> T, synonymous (F)
    assert get("TTT", "TTA") == x6[2] * 0.3      # A <-> T, F -> L
    assert get("CTA", "CTG") == x6[1]            # A <-> G, synonymous (L)
    assert get("ATG", "ACG") == x6[4] * 0.3      # C <-> T, M -> T
    assert get("TTT", "CCT") == 0.0              # two positions differ
    # GY94: -m HKY
    k = codon.codon_rates(np.asarray([1.0, 2.0, 1.0, 1.0, 2.0, 1.0]), 1.0)
    assert set(np.unique(k)) == {0.0, 1.0, 2.0}
    # batched
    rb = codon.codon_rates(np.stack([x6, x6 * 2]), np.asarray([0.3, 0.6]))
    np.testing.assert_array_equal(rb[0], r)
    np.testing.assert_allclose(rb[1], codon.codon_rates(x6 * 2, 0.6))


def test_codon_rates_jacobian_transpose():
    rng = np.random.default_rng(3)
    x6 = rng.uniform(0.5, 3.0, 6)
    om = 0.37
    g = rng.standard_normal(61 * 60 // 2)
    g_x6, g_om = codon.codon_rates_backward(x6, om, g)
    for k in range(6):
        z = x6.astype(complex)
        z[k] += 1j * STEP
        assert abs(np.dot(g, codon.codon_rates(z, om).imag) / STEP - g_x6[k]) <= 1e-13 * np.abs(g_x6).max()
    assert abs(np.dot(g, codon.codon_rates(x6, om + 1j * STEP).imag) / STEP - g_om) <= 1e-13 * abs(g_om)


def test_position_frequencies_and_transpose():
    rng = np.random.default_rng(4)
    f = rng.dirichlet(np.ones(4) * 3, 3)
    pi = codon.position_frequencies(f[0], f[1], f[2])
    assert pi.shape == (61,) and abs(pi.sum() - 1.0) < 1e-15
    j = codon.CODONS.index("ACG")
    stop = f[0][3] * f[1][0] * (f[2][0] + f[2][2]) + f[0][3] * f[1][2] * f[2][0]  # TAA TAG TGA in (A, C, G, T)
    assert abs(pi[j] - f[0][0] * f[1][1] * f[2][2] / (1.0 - stop)) < 1e-16
    g = rng.standard_normal(61)
    gs = codon.position_frequencies_backward(f[0], f[1], f[2], g)
    for p in range(3):
        for k in range(4):
            z = [v.astype(complex) for v in f]
            z[p][k] += 1j * STEP
            dd = np.dot(g, codon.position_frequencies(*z).imag) / STEP
            assert abs(dd - gs[p][k]) <= 1e-13 * np.abs(gs[p]).max()
    # batched rows agree with single ones
    gb = codon.position_frequencies_backward(f[None, 0], f[None, 1], f[None, 2], g[None])
    np.testing.assert_allclose(gb[1][0], gs[1], rtol=1e-14)


# ----------------------------------------------------------------- posterior
def _neighbours(j):
    """The sense codons one nucleotide away from codon j."""
    return [k for k in range(61) if sum(a != b for a, b in zip(codon.CODONS[j], codon.CODONS[k])) == 1]


def _codon_data(seed, S, P):
    """Columns as real codon data has them: a main codon and two of its one-nucleotide neighbours.  (Codons three
    changes apart across short branches make L_i a sum of P entries of size t^3, which the eigen route -- any
    engine's -- holds to 1e-16 absolutely, not relatively: central differences of such a log density are noise.)"""
    rng = np.random.default_rng(seed)
    main = rng.integers(0, 61, P)
    alt = np.asarray([rng.choice(_neighbours(int(j)), 2, replace=False) for j in main]).T
    pick = rng.random((S, P))
    states = np.where(pick < 0.6, main[None, :], np.where(pick < 0.8, alt[0][None, :], alt[1][None, :]))
    masks = (np.uint64(1) << states.astype(np.uint64)).astype(np.uint64)
    masks[0, 0] = np.uint64(codon.triplet_mask(codon.CODONS[int(main[0])][:2] + "N"))
    return masks, rng.integers(1, 4, P).astype(float)


def _posterior(seed, model, freqs, C, clock, coalescent=None, S=6, P=12, invariant=False):
    rooted = clock is not None
    peel0 = cases.random_peel(S, np.random.default_rng(seed))
    if not rooted:
        peel0 = cases.make_unrooted(peel0)
    masks, w = _codon_data(seed + 1, S, P)
    tree = TreeData(S, peel0, preorder_map(peel0), None, None)
    spec = ModelSpec(model=model, categories=C, invariant=invariant, clock=clock, estimate_rate=clock is not None,
                     coalescent=coalescent)
    lik = HostKStateLikelihood(masks, w, peel0, rooted, 61, spec.C)
    return codon.CodonPosterior(spec, tree, lik, freqs, counts=codon.codon_counts(masks, w))


@pytest.mark.parametrize("model,freqs,C,clock,coalescent", [("HKY", "F3x4", 1, "strict", "constant"),
                                                            ("GTR", "F1x4", 1, None, None),
                                                            ("JC69", "F61", 4, None, None)],
                         ids=["HKY+F3x4-strict-constant", "GTR+F1x4-unrooted", "JC69+F61+W4"])
def test_codon_posterior_gradient_fd(model, freqs, C, clock, coalescent):
    post = _posterior(21, model, freqs, C, clock, coalescent)
    names = [p.name for p in post.params]
    assert "omega" in names and ("kappa" in names) == (model == "HKY") and ("rates" in names) == (model == "GTR")
    assert [n for n in names if n.startswith("freqs")] == {"F3x4": ["freqs_pos1", "freqs_pos2", "freqs_pos3"],
                                                          "F1x4": ["freqs"], "F61": []}[freqs]
    rng = np.random.default_rng(5)
    u = rng.uniform(-1.0, 1.0, post.dim)
    if post.param("rate") is not None:
        u[post.param("rate").sl] = math.log(0.3)
    check_grad(post, u, tol=1e-6)
    # propto=False adds a constant
    a = post.log_prob(u[None], propto=False)[0] - post.log_prob(u[None])[0]
    assert abs(a - post.const) < 1e-9


def test_codon_posterior_columns_and_frequencies():
    post = _posterior(22, "HKY", "F3x4", 4, "strict", "constant")
    names = post.column_names()
    for nm in ("omega", "kappa", "wshape", "freqs_pos1.1", "freqs_pos3.4", "rs.4", "heights.5"):
        assert nm in names
    U = np.random.default_rng(1).uniform(-1, 1, (3, post.dim))
    assert post.flat_rows(U).shape == (3, len(names))
    s = post.codon_summary(U)
    np.testing.assert_allclose(s["pi"].sum(axis=1), 1.0, rtol=1e-14)
    mv = post.model_vectors(U)
    assert mv.shape == (3, 61 * 60 // 2 + 61 + 8) and np.count_nonzero(mv[0, :1830]) == 263
    with pytest.raises(ValueError, match="F61 needs"):
        codon.CodonPosterior(post.spec, post.tree, post.lik, "F61")


# ----------------------------------------------------------------------- CLI
def _run(argv, factory=HostKStateLikelihood, **kw):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    arg = parser.parse_args(["run"] + argv)
    lines = []
    post = cli.run(arg, likelihood_factory=factory, log=lines.append, **kw)
    return post, lines


def _dataset(tmp_path, stop=False):
    """6 taxa, 30 codons, seeded: the tree of the random fixture, sense codons drawn column by column."""
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=6, sites=90, hetero=False)
    rng = np.random.default_rng(9)
    taxa = [ln[1:].strip() for ln in open(a) if ln.startswith(">")]
    pool = rng.integers(0, 61, (2, 30))
    seqs = []
    for s in range(6):
        pick = np.where(rng.random(30) < 0.75, pool[0], pool[1])
        seqs.append("".join(codon.CODONS[j] for j in pick))
    if stop:
        seqs[2] = seqs[2][:12] + "TGA" + seqs[2][15:]
    seqs[1] = seqs[1][:3] + "ACN" + seqs[1][6:]
    with open(a, "w") as fp:
        for name, seq in zip(taxa, seqs):
            fp.write(">%s\n%s\n" % (name, seq))
    return t, a


def test_run_codon_vb(tmp_path):
    t, a = _dataset(tmp_path)
    out = str(tmp_path / "vb")
    post, lines = _run(["-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon", "-t", t, "-i", a, "-o", out, "-S", "3",
                        "--iter", "30", "--elbo_samples", "5", "--samples", "8"])
    assert any(s.startswith("Codons: 30 in ") and s.endswith("frequencies F3x4") for s in lines)
    header, data = stan_io.read_samples(out)
    for nm in ("omega", "kappa", "freqs_pos1.1", "freqs_pos2.4", "freqs_pos3.2", "blens.1"):
        assert nm in header
    assert data.shape == (9, len(header)) and np.all(data[:, header.index("omega")] > 0)
    assert os.path.exists(out + ".diag") and open(out + ".trees").read().count("tree ") == 9
    tsv = [ln.split("\t") for ln in open(out + ".codon.tsv").read().splitlines()]
    assert tsv[0] == ["parameter", "mean", "2.5%", "97.5%"]
    assert [r[0] for r in tsv[1:3]] == ["omega", "kappa"] and len(tsv) == 1 + 2 + 61 and tsv[3][0] == "pi.TTT"
    assert abs(sum(float(r[1]) for r in tsv[3:]) - 1.0) < 1e-4
    assert float(tsv[1][2]) <= float(tsv[1][1]) <= float(tsv[1][3])
    assert post.lik.calls > 0 and post.lik.K == 61


def test_run_codon_nuts_f61_gtr(tmp_path):
    t, a = _dataset(tmp_path)
    out = str(tmp_path / "nuts")
    _run(["-s", str(tmp_path / "x.stan"), "-m", "GTR", "--codon", "--codon_freqs", "F61", "-t", t, "-i", a, "-o", out,
          "-a", "nuts", "--iter", "8", "-S", "3"])
    header, data = stan_io.read_samples(out)
    assert "omega" in header and "rates.6" in header and not [h for h in header if h.startswith("freqs")]
    tsv = open(out + ".codon.tsv").read().splitlines()
    assert len(tsv) == 1 + 1 + 6 + 61 and tsv[2].startswith("rates.AC\t")


@pytest.mark.parametrize("extra,what", [(["--geo"], "--geo"), (["--topologies", "tops.trees"], "--topologies"),
                                        (["--partitions", "parts.txt"], "--partitions"),
                                        (["--ancestral_seq"], "--ancestral_seq"), (["--rescaling"], "--rescaling")])
def test_run_codon_refusals(tmp_path, extra, what):
    t, a = _dataset(tmp_path)
    out = str(tmp_path / "no")
    with pytest.raises(SystemExit, match="--codon is not supported with %s" % what):
        _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "--codon", "-t", t, "-i", a, "-o", out] + extra)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no") or f.startswith("x.stan")]


def test_run_codon_refuses_a_stop_codon_and_a_missing_engine(tmp_path):
    t, a = _dataset(tmp_path, stop=True)
    out = str(tmp_path / "no")
    with pytest.raises(SystemExit, match="--codon: codon alignment: .* site 13: TGA is an in-frame stop codon"):
        _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "--codon", "-t", t, "-i", a, "-o", out])
    # without a likelihood there is no device engine to run on: an error, never the host in its place
    with pytest.raises(SystemExit, match="--codon: this build has no device engine"):
        _run(["-s", str(tmp_path / "x.stan"), "-m", "JC69", "--codon", "-t", t, "-i", a, "-o", out], factory=None)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no") or f.startswith("x.stan")]


def test_build_records_the_codon_options(tmp_path):
    import json
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_build_parser(sub, "build", "build").set_defaults(func=cli.build)
    script = str(tmp_path / "m.stan")
    cli.build(parser.parse_args(["build", "-s", script, "-m", "HKY", "--codon", "--codon_freqs", "F1x4"]))
    opts = json.load(open(script))["options"]
    assert opts["codon"] is True and opts["codon_freqs"] == "F1x4"
    plain = str(tmp_path / "p.stan")
    cli.build(parser.parse_args(["build", "-s", plain, "-m", "HKY"]))
    assert "codon" not in json.load(open(plain))["options"]  # without --codon the description is what it was
    with pytest.raises(SystemExit, match="--codon is not supported with --geo"):
        cli.build(parser.parse_args(["build", "-s", script, "--codon", "--geo"]))
    # a run against a script built without --codon says so
    t, a = _dataset(tmp_path)
    with pytest.raises(SystemExit, match="run option codon=True differs from the built model"):
        _run(["-s", plain, "-m", "HKY", "--codon", "-t", t, "-i", a, "-o", str(tmp_path / "no")])


def test_existing_runs_against_a_built_script(tmp_path):
    """Scripts written by ``build`` carry their options into ``run``: the plain, partitioned and topologies paths
    read them as before (the option check of each path runs only when the script exists)."""
    from tests import test_forest_cpu as tf
    from tests.oracle_backend import OracleLikelihood
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_build_parser(sub, "build", "build").set_defaults(func=cli.build)
    script = str(tmp_path / "m.stan")
    cli.build(parser.parse_args(["build", "-s", script, "-m", "JC69"]))
    tree, aln, tops = tf._dataset(tmp_path)
    out = str(tmp_path / "tp")
    _, results = cli.run(tf._args(["-s", script, "-m", "JC69", "-t", tree, "-i", aln, "-o", out, "-S", "5", "--iter",
                                   "40", "--elbo_samples", "5", "--samples", "4", "--topologies", tops]),
                         likelihood_factory=tf.host_forest, log=lambda s: None)
    assert sorted(results) == [0, 1, 2] and os.path.exists(out + ".topologies.tsv")
    with pytest.raises(SystemExit, match="run option model='HKY' differs from the built model"):
        cli.run(tf._args(["-s", script, "-m", "HKY", "-t", tree, "-i", aln, "-o", out, "--topologies", tops]),
                likelihood_factory=tf.host_forest, log=lambda s: None)
    plain = str(tmp_path / "pl")
    _run(["-s", script, "-m", "JC69", "-t", tree, "-i", aln, "-o", plain, "-S", "5", "--iter", "20", "--elbo_samples", "5",
          "--samples", "4"], factory=OracleLikelihood)
    assert os.path.exists(plain) and not os.path.exists(plain + ".codon.tsv")
    # a script built with --codon is another model than a plain run's
    cscript = str(tmp_path / "c.stan")
    cli.build(parser.parse_args(["build", "-s", cscript, "-m", "JC69", "--codon"]))
    with pytest.raises(SystemExit, match="run option codon=None differs from the built model"):
        _run(["-s", cscript, "-m", "JC69", "-t", tree, "-i", aln, "-o", str(tmp_path / "no")], factory=OracleLikelihood)
