"""CPU: the sequence summaries (ancestral states, site rates, expected
substitutions) -- the host restatement and the host formula against the
independent truth of tests/seqsum_truth.py, the planner under host sanitizers,
the declared boundary, and ``run --ancestral_seq`` end to end on host
stand-ins (the device runs of the same checks: tests/test_seqsum_gpu.py)."""
import argparse
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import _lib, cli, models, seqsum
from tests import cases, fixture_files, seqsum_cases as sc, seqsum_truth
from tests.oracle_backend import OracleLikelihood

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(case):
    return seqsum.seqsum_host(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C)


# ------------------------------------------------------- the host restatement
@pytest.mark.parametrize("key", list(range(len(sc.SHAPES))) + sc.TREES)
def test_host_rows_against_the_clamping_truth(key):
    case = sc.tree_case(key) if key in sc.TREES else sc.shape_case(key)
    row = _host(case).evaluate_rows(case.blens, case.model_vec())[0]
    want = sc.truth(key)
    assert abs(row[0] - want[0]) <= 1e-10 * abs(want[0])
    sc.check_row(row, case, want, "host %s" % (key,))


def test_host_all_missing_pattern_is_the_prior():
    case = sc.missing_case()
    row = _host(case).evaluate_rows(case.blens, case.model_vec())[0]
    sc.check_row(row, case, sc.truth("missing"), "host missing")
    _, anc, cat, rate = seqsum.split_row(row, case.S, case.P, case.C)
    assert np.abs(anc[:, :, 64] - case.freqs[None, :]).max() < 1e-10
    assert np.abs(cat[:, 64] - case.ps).max() < 1e-10
    assert abs(rate[64] - float(np.dot(case.rs, case.ps))) < 1e-10


def test_host_rejected_draws_and_the_running_sum():
    case = sc.draws_case()
    bl, mv = sc.draws(case, 5)
    h = _host(case)
    good = h.evaluate_rows(bl, mv)
    bl[2, 3] = np.nan
    mv[0, 1] = -0.1
    rows = h.evaluate_rows(bl, mv)
    for k in (0, 2):
        assert rows[k, 0] == -np.inf and not rows[k, 1:].any()
    for k in (1, 3, 4):
        np.testing.assert_array_equal(rows[k], good[k])
    h.reset()
    ll = h.add(bl[:2], mv[:2])
    ll = np.concatenate([ll, h.add(bl[2:], mv[2:])])
    total, n = h.read()
    assert n == 3 and list(np.isfinite(ll)) == [False, True, False, True, True]
    want = np.zeros(h.row_len)
    for k in (1, 3, 4):
        want += rows[k]
    np.testing.assert_array_equal(total, want)


# -------------------------------------------------- expected substitutions
def _subs_case(name):
    if name == "JC69":  # a triple tie
        return cases.random_case(1, S=7, P=40, C=3, model="JC69")
    if name in ("HKY_kappa1", "HKY_near1"):  # ties / a near tie
        c = cases.random_case(2, S=7, P=40, C=3, model="HKY")
        c.freqs = np.full(4, 0.25)
        c.rates = models.hky_exchangeabilities(1.0 if name == "HKY_kappa1" else 1.0 + 1e-7)
        return c
    if name == "GTR":
        return cases.random_case(3, S=7, P=40, C=3, model="GTR")
    if name == "short_branch":
        c = cases.random_case(4, S=7, P=40, C=3, model="GTR")
        c.blens = c.blens.copy()
        c.blens[2] = 1e-8
        return c
    assert name == "unrooted"
    return cases.random_case(5, S=7, P=40, C=3, model="GTR", rooted=False)


@pytest.mark.parametrize("name", ["JC69", "HKY_kappa1", "HKY_near1", "GTR", "short_branch", "unrooted"])
def test_expected_substitutions_against_the_block_exponential(name):
    case = _subs_case(name)
    G = case.oracle()["dLdP"]
    want = seqsum_truth.expected_substitutions(case, G)
    got = models.expected_substitutions(G, case.blens, case.rs, case.freqs,
                                        None if case.model == "JC69" else case.rates)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("%s: expected substitutions, max error / largest entry %.2e (total %.3f)" % (name, err, want.sum()))
    assert got.shape == (case.blens.size,) and np.all(want > 0)
    assert err < 1e-9
    both = models.expected_substitutions(np.stack([G, G]), np.stack([case.blens] * 2), np.stack([case.rs] * 2),
                                         np.stack([case.freqs] * 2), np.stack([case.rates] * 2))
    np.testing.assert_array_equal(both[0], both[1])
    assert np.abs(both[0] - want).max() < 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("rooted", [True, False])
def test_expected_substitutions_of_an_all_missing_alignment(rooted):
    """No data: E[N_b] = (sum w) t_b sum_c ps_c rs_c."""
    case = cases.random_case(6, S=6, P=9, C=4, model="GTR", rooted=rooted)
    case.tipcodes = np.full_like(case.tipcodes, 15)
    got = models.expected_substitutions(case.oracle()["dLdP"], case.blens, case.rs, case.freqs, case.rates)
    want = case.weights.sum() * case.blens * float(np.dot(case.ps, case.rs))
    assert np.abs(got - want).max() < 1e-9 * np.abs(want).max()


# ------------------------------------------------------------------ planner
def test_seqsum_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "seqsum_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "seqsum_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    ran = subprocess.run([exe], capture_output=True, text=True)
    assert ran.returncode == 0, (ran.stdout + ran.stderr)[-2000:]
    assert re.search(r"seqsum_plan_check: \d+ plans, 0 failures", ran.stdout)


# ------------------------------------------------------------------ the ABI
def test_seqsum_boundary_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_seqsum.h")).read(), flags=re.S)
    ctx = r"phy_seqsum_ctx\s*\*\s*\w*"
    dbl, cdbl = r"\s*double\s*\*\s*\w+\s*", r"\s*const\s+double\s*\*\s*\w+\s*"
    assert re.search(r"typedef\s+struct\s+phy_seqsum_ctx\s+phy_seqsum_ctx\s*;", text)
    assert re.search(r"\bint\s+phy_seqsum_create\s*\(\s*int\s+S\s*,\s*int\s+P\s*,\s*int\s+C\s*,\s*int\s+rooted\s*,"
                     r"\s*int\s+model\s*,\s*const\s+uint8_t\s*\*\s*tipcodes\s*,\s*const\s+double\s*\*\s*weights\s*,"
                     r"\s*const\s+int32_t\s*\*\s*peel\s*,\s*int\s+max_draws\s*,\s*int\s+device\s*,"
                     r"\s*phy_seqsum_ctx\s*\*\*\s*out\s*\)", text)
    assert re.search(r"\bint\s+phy_seqsum_destroy\s*\(\s*" + ctx + r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_num_branches\s*\(\s*const\s+" + ctx + r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_row_len\s*\(\s*const\s+" + ctx + r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_eval\s*\(\s*" + ctx + r",\s*int\s+n_draws\s*," + cdbl + "," + cdbl + "," + dbl +
                     r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_reset\s*\(\s*" + ctx + r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_add\s*\(\s*" + ctx + r",\s*int\s+n_draws\s*," + cdbl + "," + cdbl + "," + dbl +
                     r"\)", text)
    assert re.search(r"\bint\s+phy_seqsum_read\s*\(\s*" + ctx + "," + dbl + r",\s*int\s*\*\s*n_finite\s*\)", text)
    for name, nargs in (("phy_seqsum_create", 11), ("phy_seqsum_destroy", 1), ("phy_seqsum_num_branches", 1),
                        ("phy_seqsum_row_len", 1), ("phy_seqsum_eval", 5), ("phy_seqsum_reset", 1),
                        ("phy_seqsum_add", 5), ("phy_seqsum_read", 3)):
        assert name in _lib.SEQSUM_SIGNATURES and len(_lib.SEQSUM_SIGNATURES[name][1]) == nargs
    assert '#include "phylo_hip_seqsum.h"' in open(os.path.join(ROOT, "include", "phylo_hip.h")).read()
    diag = open(os.path.join(ROOT, "include", "phylo_hip_diag.h")).read()
    assert re.search(r"\bint\s+phy_seqsum_plan\s*\(", diag) and len(_lib.SIGNATURES["phy_seqsum_plan"][1]) == 11
    # a context of its own: the sweep's argument structs are not grown for it
    src = open(os.path.join(ROOT, "phylostan_amd", "csrc", "seqsum_engine.inc")).read()
    assert "struct phy_seqsum_ctx" in src and "SweepArgs" not in src and "pmat_kernel<false, false>" in src


# ------------------------------------------------------------------ the CLI
def _args(argv):
    parser = argparse.ArgumentParser()
    sub = parser.add_subparsers()
    cli.create_run_parser(sub).set_defaults(func=cli.run)
    return parser.parse_args(["run"] + argv)


class CountingFactory:
    def __init__(self):
        self.made = []

    def __call__(self, *a, **kw):
        self.made.append(seqsum.seqsum_host(*a, **kw))
        return self.made[-1]


MODEL = ["-m", "HKY", "-C", "4", "--clock", "strict", "--estimate_rate", "--coalescent", "constant", "--heterochronous"]


def check_outputs(out, S, sites, C, lines, draws):
    """The four files of ``run --ancestral_seq`` and the log line (also the
    device run's checks, tests/test_seqsum_gpu.py).  Returns the pattern count."""
    fasta = open(out + ".ancestral.fasta").read().split()
    assert [h for h in fasta[0::2]] == [">node%d" % v for v in range(S + 1, 2 * S)]
    assert all(len(s) == sites and set(s) <= set("ACGT") for s in fasta[1::2])
    tsv = [ln.split("\t") for ln in open(out + ".ancestral.tsv").read().splitlines()]
    assert tsv[0] == ["node", "pattern", "A", "C", "G", "T"]
    body = np.array(tsv[1:], dtype=np.float64)
    P = int(body[:, 1].max())
    assert body.shape == ((S - 1) * P, 6) and set(body[:, 0]) == set(range(S + 1, 2 * S))
    assert np.all(body[:, 2:] >= 0) and np.abs(body[:, 2:].sum(axis=1) - 1.0).max() < 1e-10
    rates = [ln.split("\t") for ln in open(out + ".siterates.tsv").read().splitlines()]
    assert rates[0] == ["site", "pattern", "rate"] + ["p_cat%d" % (c + 1) for c in range(C)]
    rb = np.array(rates[1:], dtype=np.float64)
    assert rb.shape == (sites, 3 + C) and list(rb[:, 0]) == list(range(1, sites + 1))
    assert rb[:, 1].min() >= 1 and rb[:, 1].max() == P and np.all(rb[:, 2] > 0)
    assert np.abs(rb[:, 3:].sum(axis=1) - 1.0).max() < 1e-10
    # the fasta is the modal state of the site's pattern
    modal = {(int(r[0]), int(r[1])): "ACGT"[int(np.argmax(r[2:]))] for r in body}
    for k, v in enumerate(range(S + 1, 2 * S)):
        assert fasta[1 + 2 * k] == "".join(modal[(v, int(p))] for p in rb[:, 1])
    trees = open(out + ".ancestral.trees").read()
    assert trees.startswith("#NEXUS\nBegin trees;\nTranslate\n1 t") and trees.count("tree ") == 1 and trees.endswith("END;")
    subs = [float(x) for x in re.findall(r"\[&subs=([^\]]+)\]", trees)]
    lens = [float(x) for x in re.findall(r"\]:([0-9.eE+-]+)", trees)]
    assert len(subs) == 2 * S - 2 and len(lens) == 2 * S - 2 and all(x >= 0 for x in subs) and all(x >= 0 for x in lens)
    assert re.search(r"\)%d;" % (2 * S - 1), trees)  # internal nodes carry their id, the root last
    line = [s for s in lines if s.startswith("Expected substitutions:")]
    assert len(line) == 1
    m = re.match(r"Expected substitutions: ([0-9.]+) over (\d+) draws; mean site rate ([0-9.]+)", line[0])
    assert m and int(m.group(2)) == draws and abs(float(m.group(1)) - sum(subs)) < 1e-3 * max(1.0, sum(subs))
    assert abs(float(m.group(3)) - rb[:, 2].mean()) < 1e-3
    return P


@pytest.mark.parametrize("algo", ["vb", "nuts"])
def test_cli_ancestral_seq_on_host_stand_ins(tmp_path, capsys, algo):
    S, sites = 6, 30
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=S, sites=sites)
    out = str(tmp_path / "anc")
    how = ["--iter", "200", "--elbo_samples", "10", "--samples", "12", "--tol_rel_obj", "0.01"] if algo == "vb" else \
        ["-a", "nuts", "--iter", "24"]
    factory, lines = CountingFactory(), []
    cli.run(_args(["-s", str(tmp_path / "m.stan")] + MODEL + ["-t", t, "-i", a, "-o", out, "-S", "3", "--ancestral_seq"] +
                  how), likelihood_factory=OracleLikelihood, log=lines.append, summary_factory=factory)
    capsys.readouterr()
    assert len(factory.made) == 1
    check_outputs(out, S, sites, 4, lines, 12)
    assert factory.made[0].read()[1] == 12
    assert os.path.exists(out + ".trees")  # the run's own files are written as before


def test_cli_without_the_flag_nothing_new(tmp_path, capsys):
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=6, sites=30)
    out = str(tmp_path / "plain")
    factory, lines = CountingFactory(), []
    cli.run(_args(["-s", str(tmp_path / "m.stan")] + MODEL + ["-t", t, "-i", a, "-o", out, "-S", "3", "--iter", "200",
                                                             "--elbo_samples", "10", "--samples", "12", "--tol_rel_obj",
                                                             "0.01"]),
            likelihood_factory=OracleLikelihood, log=lines.append, summary_factory=factory)
    capsys.readouterr()
    assert factory.made == []
    assert sorted(os.listdir(str(tmp_path))) == sorted(["plain", "plain.diag", "plain.trees", "rand.fa", "rand.tree"])
    assert not any("Expected substitutions" in s for s in lines)


@pytest.mark.parametrize("extra,what", [(["--geo"], "--geo"), (["--topologies", "tops.trees"], "--topologies"),
                                        (["--rescaling"], "--rescaling"), (["--samples", "0"], "--samples")])
def test_cli_ancestral_seq_refusals(tmp_path, extra, what):
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=6, sites=30)
    out = str(tmp_path / "no")
    factory = CountingFactory()
    with pytest.raises(SystemExit, match="--ancestral_seq .*%s" % what):
        cli.run(_args(["-s", str(tmp_path / "m.stan"), "-m", "JC69", "-t", t, "-i", a, "-o", out, "--ancestral_seq"] + extra),
                likelihood_factory=OracleLikelihood, log=lambda s: None, summary_factory=factory)
    assert factory.made == [] and not any(f.startswith("no") for f in os.listdir(str(tmp_path)))


def test_ancestral_without_geo_still_refuses(tmp_path):
    t, a = fixture_files.write_random_dataset(str(tmp_path), seed=4, S=6, sites=30)
    with pytest.raises(SystemExit, match="--ancestral .* needs --geo"):
        cli.run(_args(["-s", str(tmp_path / "m.stan"), "-m", "JC69", "-t", t, "-i", a, "-o", str(tmp_path / "x"),
                       "--ancestral"]), likelihood_factory=OracleLikelihood, log=lambda s: None)


def test_site_pattern_map_expands_patterns_to_sites():
    from phylostan_amd import data as dataio
    chars = np.frombuffer(b"ACCAGA" b"ATTAGA" b"GCCGGG", dtype=np.uint8).reshape(3, 6)
    tip, w, first = dataio.compress_patterns(chars)
    sp = dataio.site_patterns(chars)
    assert list(sp) == [0, 1, 1, 0, 2, 0] and list(w) == [3, 2, 1] and list(first) == [0, 1, 4]
    np.testing.assert_array_equal(tip[:, sp], dataio._DNA_CODE[chars])
