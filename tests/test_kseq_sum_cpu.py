"""CPU: the K-state engine's posterior summaries on the host.

* ``kseq.kseq_sum_host`` (node posteriors and labelled substitution counts per
  branch) against the exact reference of ``tests/kseq_sum_truth.py`` over its
  shape list, the tied codon case and the deep caterpillar, at the project's
  bars: log L 1e-10 relative, node_post 1e-9 absolute, bcounts 1e-9 of the
  array's largest entry;
* its invariants: every (node, pattern) sums to one to 1e-12, counts linear in
  the labels and exactly zero on a zero-length branch, the unrooted root and the
  merged child equal, a zero-weight column keeps its posterior and counts
  nothing, refused draws, the running sum;
* ``codon.codon_labels`` and ``codon.neutral_rates``;
* ``run --codon --codon_ancestral`` end to end on the host stand-ins, and its
  refusals;
* tests/kseq_sum_plan_check.cpp under the host sanitizers, the signatures
  against the header, the create refusals before the device, the wrapper's own
  checks and the committed resource table.
"""
import argparse
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import _lib, cli, codon, kseq
from tests import kseq_sum_truth as st
from tests import test_codon_cpu as tcc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHY_EINVAL = 1
CASES = st.small_cases()


def _host(case, blens=None, params=None, labels=None, weights=None):
    bl = case.blens[None] if blens is None else blens
    pr = case.params[None] if params is None else params
    return kseq.kseq_sum_host(case.masks, case.weights if weights is None else weights, case.peel, case.rooted, bl, pr,
                              case.K, case.M, case.C, case.labels if labels is None else labels)


# ----------------------------------------------------------------- the truth
@pytest.mark.parametrize("case", CASES + [st.tied_codon(), st.deep_caterpillar()],
                         ids=[c.name for c in CASES] + ["tied_codon", "deep_caterpillar"])
def test_host_against_the_truth(case):
    ref = st.shared_truth(case)
    ll, bc, npost = _host(case)
    err = st.compare(case, ll[0], bc[0], npost[0], ref)
    assert not st.bars(err), err


# ----------------------------------------------------------------- invariants
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_invariants(case):
    ll, bc, npost = _host(case)
    assert np.isfinite(ll[0]) and np.all(npost >= -1e-15)
    np.testing.assert_allclose(npost[0].sum(axis=1), 1.0, rtol=0, atol=st.SUM_BAR)  # zero-weight columns included
    zero = np.flatnonzero(case.blens == 0.0)
    assert not bc[0][:, zero].any()
    if not case.rooted:  # the root 2S-2 and the merged child 2S-3: the same point of the tree
        np.testing.assert_allclose(npost[0, case.S - 2], npost[0, case.S - 3], rtol=0, atol=1e-13)
    # linear in the labels
    rng = np.random.default_rng(1)
    mix = rng.uniform(0.5, 2.0, (1, case.NL))
    _, bc2, _ = _host(case, labels=mix @ case.labels)
    np.testing.assert_allclose(bc2[0, 0], (mix @ bc[0])[0], rtol=1e-12, atol=1e-13 * np.max(np.abs(bc)))


def test_zero_weight_column_keeps_its_posterior_and_counts_nothing():
    case = CASES[3]  # K = 17, M = 2, C = 4; weights[0] = 0
    assert case.weights[0] == 0.0
    _, bc, npost = _host(case)
    w1 = case.weights.copy()
    w1[0] = 1.0
    _, bc1, npost1 = _host(case, weights=w1)
    np.testing.assert_allclose(npost[0, :, :, 0], npost1[0, :, :, 0], rtol=0, atol=1e-15)
    # without the column altogether: the same counts
    keep = np.arange(1, case.P)
    _, bc_cut, _ = kseq.kseq_sum_host(case.masks[:, keep], case.weights[keep], case.peel, case.rooted, case.blens[None],
                                      case.params[None], case.K, case.M, case.C, case.labels)
    np.testing.assert_allclose(bc[0], bc_cut[0], rtol=1e-13)
    assert np.max(np.abs(bc1 - bc)) > 1e-3  # and with its weight it counts


def test_category_of_rate_zero_counts_nothing():
    case = CASES[7]  # K = 64, C = 4 with rs_0 = 0
    pr = case.params.copy()
    G = case.M * case.C
    pr[-G:] = 0.0
    pr[-G] = 1.0  # all the weight on the category of rate 0: only constant patterns have a likelihood
    masks = np.repeat(np.left_shift(np.uint64(1), np.arange(case.P, dtype=np.uint64))[None], case.S, 0)
    ll, bc, npost = kseq.kseq_sum_host(masks, case.weights, case.peel, case.rooted, case.blens[None], pr[None],
                                       case.K, case.M, case.C, case.labels)
    assert np.isfinite(ll[0]) and not bc.any()
    np.testing.assert_allclose(npost[0].sum(axis=1), 1.0, rtol=0, atol=st.SUM_BAR)


def test_refused_draws_and_the_running_sum():
    case = CASES[1]
    bl = np.repeat(case.blens[None], 4, 0)
    pr = np.repeat(case.params[None], 4, 0)
    pr[1, case.R + 1] = -1.0
    bl[2] *= 0.5
    host = kseq.HostKStateSummaries(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C,
                                    case.labels)
    ll, bc, npost = host.evaluate(bl, pr)
    assert ll[1] == -np.inf and not bc[1].any() and not npost[1].any() and np.isfinite(ll[[0, 2, 3]]).all()
    np.testing.assert_array_equal(npost[0], npost[3])
    host.reset()
    host.add(bl[:1], pr[:1])
    l2, b2 = host.add(bl[1:], pr[1:])
    total, nf = host.read()
    assert nf == 3 and l2[0] == -np.inf
    np.testing.assert_array_equal(total, ((0.0 + npost[0]) + npost[2]) + npost[3])
    np.testing.assert_array_equal(b2, bc[1:])
    with pytest.raises(ValueError, match="labels must be"):
        kseq.check_labels(np.ones((5, case.R)), case.K)
    with pytest.raises(ValueError, match="finite and non-negative"):
        kseq.check_labels(-np.ones((1, case.R)), case.K)


# -------------------------------------------------------------- codon helpers
def test_codon_labels_partition_the_live_pairs():
    lab = codon.codon_labels()
    assert lab.shape == (2, 61 * 60 // 2) and set(np.unique(lab)) == {0.0, 1.0}
    assert not (lab[0] * lab[1]).any() and int(lab.sum()) == 263
    rates = codon.codon_rates(np.asarray([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), 0.5)
    np.testing.assert_array_equal(lab.sum(axis=0) > 0, rates > 0)
    pairs = kseq.rate_pairs(61)
    for k, (row, col) in enumerate(pairs):
        a, b = codon.CODONS[row], codon.CODONS[col]
        one = sum(x != y for x, y in zip(a, b)) == 1
        same = codon.AMINO[row] == codon.AMINO[col]
        assert lab[0, k] == float(one and same) and lab[1, k] == float(one and not same)


def test_neutral_rates_against_a_double_loop():
    rng = np.random.default_rng(2)
    x6 = rng.uniform(0.5, 3.0, (2, 6))
    pi = rng.dirichlet(np.ones(61) * 3.0, 2)
    rho_s, rho_n = codon.neutral_rates(x6, pi)
    pair = {frozenset("AC"): 0, frozenset("AG"): 1, frozenset("AT"): 2, frozenset("CG"): 3, frozenset("CT"): 4,
            frozenset("GT"): 5}
    for n in range(2):
        s = v = 0.0
        for i in range(61):
            for j in range(61):
                a, b = codon.CODONS[i], codon.CODONS[j]
                diff = [p for p in range(3) if a[p] != b[p]]
                if len(diff) != 1:
                    continue
                q = x6[n, pair[frozenset((a[diff[0]], b[diff[0]]))]] * pi[n, j]
                if codon.AMINO[i] == codon.AMINO[j]:
                    s += pi[n, i] * q
                else:
                    v += pi[n, i] * q
        assert abs(rho_s[n] - s) <= 1e-14 * s and abs(rho_n[n] - v) <= 1e-14 * v
    one_s, one_n = codon.neutral_rates(x6[0], pi[0])
    assert one_s == rho_s[0] and one_n == rho_n[0]


# ----------------------------------------------------------------------- CLI
def run_codon_ancestral(tmp_path, extra, device=False, sites=None, model="HKY"):
    """``run --codon --codon_ancestral`` on the 6-taxon, 30-codon fixture of tests/test_codon_cpu.py; the
    likelihood and the summaries on the host stand-ins, or the device classes as ``cli.main`` binds them."""
    t, a = tcc._dataset(tmp_path)
    out = str(tmp_path / "anc")
    argv = ["-s", str(tmp_path / "x.stan"), "-m", model, "--codon", "--codon_ancestral", "-t", t, "-i", a, "-o", out,
            "--iter", "30", "--elbo_samples", "5", "--samples", "6"] + (["--codon_sites", sites] if sites else []) + extra
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    arg = parser.parse_args(["run"] + argv)
    if device:
        lik = kseq.DeviceKStateMixLikelihood if sites else kseq.DeviceKStateLikelihood
        summ = kseq.DeviceKStateSummaries
    else:
        lik = kseq.HostKStateMixLikelihood if sites else kseq.HostKStateLikelihood
        summ = kseq.HostKStateSummaries
    lines = []
    post = cli.run(arg, likelihood_factory=lik, log=lines.append, codon_summary_factory=summ)
    return {"stem": out, "post": post, "lines": lines, "S": 6, "codons": 30}


def check_outputs(out):
    stem, S, ncod = out["stem"], out["S"], out["codons"]
    fasta = open(stem + ".ancestral.fasta").read().split()
    assert fasta[0::2] == [">node%d" % v for v in range(S + 1, 2 * S)]
    for seq in fasta[1::2]:
        assert len(seq) == 3 * ncod and set(seq) <= set("ACGT")
        assert all(seq[k:k + 3] in codon.CODONS for k in range(0, len(seq), 3))
    tsv = [ln.split("\t") for ln in open(stem + ".ancestral.tsv").read().splitlines()]
    assert tsv[0] == ["node", "codon_site", "codon", "amino_acid", "probability"] and len(tsv) == 1 + (S - 1) * ncod
    for r in tsv[1:]:
        assert r[2] in codon.CODONS and r[3] == codon.AMINO[codon.CODONS.index(r[2])] and 0.0 < float(r[4]) <= 1.0 + 1e-6
    assert "".join(r[2] for r in tsv[1:1 + ncod]) == fasta[1]
    br = [ln.split("\t") for ln in open(stem + ".codon_branches.tsv").read().splitlines()]
    assert br[0] == ["branch", "S_mean", "S_2.5%", "S_97.5%", "N_mean", "N_2.5%", "N_97.5%", "dNdS"]
    B = out["post"].B
    assert len(br) == 1 + B and [r[0] for r in br[1:]] == [str(b + 1) for b in range(B)]
    vals = np.asarray([[float(x) for x in r[1:]] for r in br[1:]])
    assert np.all(vals[:, :6] >= 0) and np.all(vals[:, 1] <= vals[:, 0] + 1e-6) and np.all(vals[:, 0] <= vals[:, 2] + 1e-6)
    assert np.all(vals[:, 4] <= vals[:, 3] + 1e-6) and np.all(vals[:, 3] <= vals[:, 5] + 1e-6)
    assert np.all(np.isnan(vals[:, 6]) == (vals[:, 0] == 0)) and np.all(vals[~np.isnan(vals[:, 6]), 6] >= 0)
    trees = open(stem + ".ancestral.trees").read()
    assert trees.count("[&S=") == 2 * S - 2 and trees.count(",N=") == 2 * S - 2 and trees.count("tree 1 = ") == 1
    line = [s for s in out["lines"] if s.startswith("Codon substitutions: S ")]
    assert len(line) == 1 and "over 6 draws" in line[0] and "tree dN/dS" in line[0]
    got = re.match(r"Codon substitutions: S ([0-9.]+), N ([0-9.]+)", line[0])
    assert abs(float(got.group(1)) - vals[:, 0].sum()) < 2e-3 and abs(float(got.group(2)) - vals[:, 3].sum()) < 2e-3
    assert os.path.exists(stem + ".codon.tsv")


@pytest.mark.parametrize("extra,sites", [(["-a", "vb", "-S", "3"], None), (["-a", "vb", "-S", "3"], "M2a"),
                                         (["-a", "nuts", "-S", "3", "--iter", "12"], None),
                                         (["-a", "nuts", "-S", "3", "--iter", "12"], "M2a")],
                         ids=["vb", "vb_M2a", "nuts", "nuts_M2a"])
def test_run_codon_ancestral(tmp_path, extra, sites):
    out = run_codon_ancestral(tmp_path, extra, sites=sites)  # vb: 6 output draws; nuts: 6 kept of 12 iterations
    check_outputs(out)
    assert os.path.exists(out["stem"] + ".codon_sites.tsv") == bool(sites)


def _refused(tmp_path, argv, match, **kw):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    t, a = tcc._dataset(tmp_path)
    arg = parser.parse_args(["run", "-s", str(tmp_path / "x.stan"), "-m", "JC69", "-t", t, "-i", a, "-o",
                             str(tmp_path / "no")] + argv)
    with pytest.raises(SystemExit, match=match):
        cli.run(arg, log=lambda s: None, **kw)
    assert not [f for f in os.listdir(str(tmp_path)) if f.startswith("no") or f.startswith("x.stan")]


def test_run_codon_ancestral_refusals(tmp_path):
    both = dict(likelihood_factory=kseq.HostKStateLikelihood, codon_summary_factory=kseq.HostKStateSummaries)
    _refused(tmp_path, ["--codon_ancestral"], "--codon_ancestral needs --codon", **both)
    _refused(tmp_path, ["--codon", "--codon_ancestral", "--ancestral_seq"],
             "--codon_ancestral is not supported with --ancestral_seq", **both)
    _refused(tmp_path, ["--codon", "--codon_ancestral", "--samples", "0"],
             "--codon_ancestral needs at least one posterior draw", **both)
    _refused(tmp_path, ["--codon", "--ancestral_seq"], "--codon is not supported with --ancestral_seq", **both)
    # without the summaries class there is no device engine to run on: an error, never the host in its place
    _refused(tmp_path, ["--codon", "--codon_ancestral"], "--codon_ancestral: this build has no device summaries",
             likelihood_factory=kseq.HostKStateLikelihood)


def test_without_the_flag_no_summary_is_made(tmp_path):
    def never(*a, **k):
        raise AssertionError("the summaries were made without --codon_ancestral")

    t, a = tcc._dataset(tmp_path)
    out = str(tmp_path / "plain")
    tcc._run(["-s", str(tmp_path / "x.stan"), "-m", "HKY", "--codon", "-t", t, "-i", a, "-o", out, "-S", "3", "--iter",
              "20", "--elbo_samples", "5", "--samples", "4"], codon_summary_factory=never)
    made = sorted(f for f in os.listdir(str(tmp_path)) if f.startswith("plain"))
    assert made == ["plain", "plain.codon.tsv", "plain.diag", "plain.trees"]


# ------------------------------------------------------- planner and boundary
def test_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "kseq_sum_plan_check")
    # the sanitizer runtimes linked in: the program needs nothing preloaded
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "kseq_sum_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "0 failures" in run.stdout and "FAIL" not in run.stdout


def test_signatures_match_the_header():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "phylo_hip_kseq_sum.h")).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(phy_kseq_sum_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = ["ptr" if "*" in a else "int" for a in args.split(",")]
    assert sorted(protos) == ["phy_kseq_sum_add", "phy_kseq_sum_create", "phy_kseq_sum_destroy", "phy_kseq_sum_eval",
                              "phy_kseq_sum_num_branches", "phy_kseq_sum_read", "phy_kseq_sum_reset"]
    assert sorted(protos) == sorted(_lib.KSEQ_SUM_SIGNATURES)
    for name, kinds in protos.items():
        res, args = _lib.KSEQ_SUM_SIGNATURES[name]
        assert res is ctypes.c_int
        assert ["int" if a is ctypes.c_int else "ptr" for a in args] == kinds, name
    main = open(os.path.join(ROOT, "include", "phylo_hip_kseq.h")).read()
    assert '#include "phylo_hip_kseq_sum.h"' in main and "phy_kseq_sum_create(" not in main


needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason="HIP library not built (run __graft_entry__.build())")


@needs_lib
def test_create_refusals_come_before_the_device():
    case = CASES[3]
    S, P, K, M, C = case.S, case.P, case.K, case.M, case.C
    m, w, peel = case.masks, case.weights, np.ascontiguousarray(case.peel, np.int32)
    lib = _lib.load()

    def create(K_, M_, NL, labels):
        ctx = ctypes.c_void_p()
        rc = lib.phy_kseq_sum_create(S, P, K_, M_, C, 0, m.ctypes.data, w.ctypes.data, peel.ctypes.data, NL,
                                     None if labels is None else labels.ctypes.data, 1, 0, ctypes.byref(ctx))
        msg = lib.phy_last_error().decode()
        if rc == 0:
            lib.phy_kseq_sum_destroy(ctx)
        return rc, msg

    neg = case.labels.copy()
    neg[1, 7] = -0.5
    nan = case.labels.copy()
    nan[0, 2] = np.nan
    for args, needle in [((K, M, 0, case.labels), "phy_kseq_sum_create: n_labels = 0, supported 1..4"),
                         ((K, M, 5, case.labels), "n_labels = 5"),
                         ((K, M, 2, None), "labels is NULL"),
                         ((K, M, 2, neg), "labels[1][7] is negative or not finite"),
                         ((K, M, 2, nan), "labels[0][2] is negative or not finite"),
                         ((K, 9, 2, case.labels), "phy_kseq_sum_create: M = 9 components"),
                         ((65, M, 2, case.labels), "K = 65 states")]:
        rc, msg = create(*args)
        assert rc == PHY_EINVAL and needle in msg and "device" not in msg, (needle, rc, msg)
    x = np.zeros(8)
    p = x.ctypes.data
    assert lib.phy_kseq_sum_eval(None, 1, p, p, p, p, None) == PHY_EINVAL
    assert "phy_kseq_sum_eval: NULL ctx" in lib.phy_last_error().decode()
    assert lib.phy_kseq_sum_add(None, 1, p, p, p, p) == PHY_EINVAL and lib.phy_kseq_sum_reset(None) == PHY_EINVAL
    assert lib.phy_kseq_sum_read(None, p, None) == PHY_EINVAL and lib.phy_kseq_sum_num_branches(None) == -1


def test_wrapper_validates_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    case = CASES[1]
    ok = (case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C, case.labels)
    with pytest.raises(ValueError, match="tipmasks must be \\[S, P\\]"):
        kseq.DeviceKStateSummaries(case.masks[0], *ok[1:])
    with pytest.raises(ValueError, match="labels must be"):
        kseq.DeviceKStateSummaries(*ok[:7], case.labels[:, :-1])
    with pytest.raises(ValueError, match="finite and non-negative"):
        kseq.DeviceKStateSummaries(*ok[:7], -case.labels)
    with pytest.raises(ValueError, match="M 1..8"):
        kseq.DeviceKStateSummaries(case.masks, case.weights, case.peel, case.rooted, case.K, 0, 1, case.labels)
    with pytest.raises(ValueError, match="max_draws"):
        kseq.DeviceKStateSummaries(*ok, max_draws=0)
    with pytest.raises(AssertionError, match="the library was touched"):  # valid data reaches the library
        kseq.DeviceKStateSummaries(*ok)


def test_resource_table():
    """profiles/kseq_sum_resources.json: the gfx950 cross-compile's figures of the four new kernels; no scratch;
    the five kernels of kseq_engine.inc at the parent commit's figures."""
    table = json.load(open(os.path.join(ROOT, "profiles", "kseq_sum_resources.json")))
    assert sorted(table["kernels"]) == ["kseq_sum_blab_kernel", "kseq_sum_counts_kernel", "kseq_sum_down_kernel",
                                        "kseq_sum_fold_kernel"]
    for name, k in table["kernels"].items():
        assert k["scratch_bytes_per_lane"] == 0 and k["vgprs_spilled"] == 0, name
        assert k["vgprs"] <= 256 and k["agprs"] <= 256, name
    old = {n: k for n, k in table["existing_kernels"].items() if n != "statement"}
    assert sorted(old) == ["kseq_combine_kernel", "kseq_down_kernel", "kseq_eig_kernel", "kseq_site_kernel",
                           "kseq_up_kernel"]
    for name, k in old.items():
        for key in ("vgprs", "agprs", "sgprs", "scratch_bytes_per_lane", "waves_per_simd"):
            assert k[key] == k["parent"][key], (name, key)
        assert k["scratch_bytes_per_lane"] == 0, name
