"""CPU: the phylogeography summaries (ancestral locations, expected migration
counts and dwell times, migrations per branch) above the kernel:
``geo.geo_summaries_host`` against truths that share no algebra with it
(tests/geo_summary_truth.py: enumeration for the marginals, complex-step
derivatives with respect to Q's own entries for the counts), the invariants,
the accumulator, ``run --geo --ancestral`` end to end on a host likelihood, and
the declared boundary.  The device: tests/test_geo_summaries_gpu.py.

Bars (the project's): marginals absolute 1e-10, each count array within 1e-9
of its largest entry, the invariants at 1e-12 (row sums) and relative 1e-9.
A known tip's marginal is ``tip partial x up``: the off states are exact zeros
(a zero partial) and the on state is the row sum, 1 within the 1e-12 of the row
sums -- that is what "one-hot" is held to.
"""
import functools
import os
import re

import numpy as np
import pytest

from phylostan_amd import _lib, geo, treeio
from tests import geo_oracle as go
from tests import geo_summary_truth as gt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARG_BAR, JUMP_BAR, SUM_BAR, REL_BAR = 1e-10, 1e-9, 1e-12, 1e-9


def point(S, K, seed, missing=(0,)):
    rng = np.random.default_rng(seed)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=missing)
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    R = geo.rate_count(K)
    return tips, peel, blens[0], params[0, :R], params[0, R:]


def check_invariants(tips, peel, blens, rates, freqs, marg, jumps, bjumps, grad_blens=None):
    """The identities of the issue, for any source of the three arrays."""
    S, K = tips.shape
    assert np.abs(marg.sum(1) - 1.0).max() <= SUM_BAR
    for n in range(S):
        if tips[n].sum() == 1.0:
            on = int(np.argmax(tips[n]))
            assert np.all(np.delete(marg[n], on) == 0.0) and abs(marg[n, on] - 1.0) <= SUM_BAR, n
    assert np.array_equal(marg[2 * S - 3], marg[2 * S - 2])
    T = np.diag(jumps)
    off = jumps.sum() - T.sum()
    tree_len = blens.sum()
    assert abs(T.sum() - tree_len) <= REL_BAR * tree_len
    assert abs(bjumps.sum() - off) <= REL_BAR * off
    if grad_blens is None:
        grad_blens = geo.geo_gradients_host(tips, peel, blens, rates, freqs)[1]
    Q = go.build_q(freqs, rates).real
    assert abs((blens * grad_blens).sum() - (np.diag(Q) * T).sum() - off) <= REL_BAR * off
    assert np.all(jumps >= -JUMP_BAR * np.abs(jumps).max()) and np.all(bjumps >= -JUMP_BAR * bjumps.max())


@functools.lru_cache(maxsize=None)
def host_and_truth(S, K):
    tips, peel, blens, rates, freqs = point(S, K, 1000 * S + K)
    host = geo.geo_summaries_host(tips, peel, blens, rates, freqs)
    jumps = gt.jump_matrix(tips, peel, blens, rates, freqs)
    bj = gt.branch_jump_truth(tips, peel, blens, rates, freqs)
    return (tips, peel, blens, rates, freqs), host, jumps, bj


@pytest.mark.parametrize("K", [2, 3])
@pytest.mark.parametrize("S", [4, 5])
def test_marginals_against_enumeration(S, K):
    """Every joint assignment of the nodes, one tip missing."""
    tips, peel, blens, rates, freqs = point(S, K, 40 * S + K)
    want = gt.brute_marginals(tips, peel, blens, rates, freqs)
    marg = geo.geo_summaries_host(tips, peel, blens, rates, freqs)[0]
    print("S %d K %d: marginals vs enumeration %.2e" % (S, K, np.abs(marg - want).max()))
    assert np.abs(want.sum(1) - 1.0).max() <= SUM_BAR
    assert np.abs(marg - want).max() <= MARG_BAR
    assert 0.0 < marg[0].max() < 1.0  # the missing tip is imputed, not one-hot


def test_the_complex_step_counts_against_quadrature():
    """The truth of the counts itself, once, where both can be had: on a single
    branch from a known state to a known state, E[N_ij] and E[T_i] by numerical
    quadrature of Minin and Suchard's integral P(s) E_ij P(t - s)."""
    K, t = 3, 0.7
    rng = np.random.default_rng(3)
    _, params = go.random_draws(1, 3, K, rng)
    rates, freqs = params[0, :3], params[0, 3:]
    Q = go.build_q(freqs, rates).real
    # S = 3 with two zero-length branches: tips 1 and 2 sit on the root, tip 0 is t away
    tips = np.eye(K)[[0, 1, 1]]
    peel = np.asarray([(1, 2, 3), (0, 3, 4)], np.int32)
    blens = np.asarray([t, 0.0, 0.0])
    got = gt.jump_matrix(tips, peel, blens, rates, freqs)
    x, w = np.polynomial.legendre.leggauss(40)
    s = 0.5 * t * (x + 1.0)
    Ps = go.expm(Q[None] * s[:, None, None]).real
    Pr = go.expm(Q[None] * (t - s)[:, None, None]).real
    Pt = go.expm(Q * t).real
    # the branch's parent end is the root (state 1), its child end tip 0 (state 0)
    want = np.einsum("s,si,sj->ij", 0.5 * t * w, Ps[:, 1, :], Pr[:, :, 0]) / Pt[1, 0]
    want = np.where(np.eye(K, dtype=bool), want, want * Q)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    host = geo.geo_summaries_host(tips, peel, blens, rates, freqs)
    assert np.abs(host[1] - want).max() <= JUMP_BAR * np.abs(want).max()
    off = want.sum() - np.trace(want)
    assert abs(host[2][0] - off) <= JUMP_BAR * off and np.all(host[2][1:] == 0.0)  # the one branch with a length


@pytest.mark.parametrize("K", [2, 3, 5])
@pytest.mark.parametrize("S", [3, 5, 7])
def test_host_summaries_against_the_truths(S, K):
    (tips, peel, blens, rates, freqs), (marg, jumps, bjumps), tj, tb = host_and_truth(S, K)
    ej, eb = np.abs(jumps - tj).max() / np.abs(tj).max(), np.abs(bjumps - tb).max() / np.abs(tb).max()
    print("S %d K %d: jumps %.2e, bjumps %.2e of the largest entry" % (S, K, ej, eb))
    assert ej <= JUMP_BAR and eb <= JUMP_BAR
    assert abs(bjumps.sum() - tb.sum()) <= JUMP_BAR * tb.sum()
    if K ** (2 * S - 2) <= 70000:
        want = gt.brute_marginals(tips, peel, blens, rates, freqs)
        assert np.abs(marg - want).max() <= MARG_BAR
    check_invariants(tips, peel, blens, rates, freqs, marg, jumps, bjumps)
    # the truths obey the same identities
    off = tj.sum() - np.trace(tj)
    assert abs(np.trace(tj) - blens.sum()) <= REL_BAR * blens.sum() and abs(tb.sum() - off) <= REL_BAR * off


@pytest.mark.parametrize("arm", ["tie", "near"])
def test_host_summaries_with_a_repeated_eigenvalue(arm):
    K = 4
    tips, peel, blens, rates, _ = point(6, K, 9)
    rates = np.ones_like(rates)
    if arm == "near":
        rates[1] += 1e-11
    freqs = np.full(K, 1.0 / K)
    marg, jumps, bjumps = geo.geo_summaries_host(tips, peel, blens, rates, freqs)
    tj = gt.jump_matrix(tips, peel, blens, rates, freqs)
    tb = gt.branch_jump_truth(tips, peel, blens, rates, freqs)
    assert np.abs(jumps - tj).max() <= JUMP_BAR * np.abs(tj).max()
    assert np.abs(bjumps - tb).max() <= JUMP_BAR * np.abs(tb).max()
    check_invariants(tips, peel, blens, rates, freqs, marg, jumps, bjumps)


def test_host_summaries_of_a_bad_draw_are_zero():
    tips, peel, blens, rates, freqs = point(5, 3, 2)
    bad = freqs.copy()
    bad[1] = np.nan
    for arr in geo.geo_summaries_host(tips, peel, blens, rates, bad):
        assert np.all(arr == 0.0)
    assert geo.summary_len(5, 3) == 9 * 3 + 9 + 7


def test_summary_accumulator_and_layout():
    S, K = 5, 3
    tips, peel, blens, rates, freqs = point(S, K, 8)
    rng = np.random.default_rng(1)
    _, params = go.random_draws(4, 2 * S - 3, K, rng)
    each = [geo.geo_summaries_host(tips, peel, blens, p[:3], p[3:]) for p in params]
    flat = np.stack([np.concatenate([m.ravel(), j.ravel(), b]) for m, j, b in each])
    assert flat.shape[1] == geo.summary_len(S, K)
    marg, jumps, bjumps = geo.split_summaries(flat, S, K)
    assert np.array_equal(marg[2], each[2][0]) and np.array_equal(jumps[1], each[1][1])
    assert np.array_equal(bjumps[3], each[3][2])
    acc = geo.GeoSummary(S, K)
    with pytest.raises(ValueError):
        acc.marg
    rows = np.zeros((4, 1))
    rows[3, 0] = -np.inf  # a refused draw: its zero summary is not averaged in
    acc.add(rows[:2], marg[:2], jumps[:2], bjumps[:2])
    acc.add(rows[2:], marg[2:], jumps[2:], bjumps[2:])
    assert acc.count == 3 and acc.skipped == 1
    assert np.allclose(acc.marg, marg[:3].mean(0), rtol=0, atol=1e-15)
    assert np.allclose(acc.jumps, jumps[:3].mean(0), rtol=1e-14)
    assert np.allclose(acc.bjumps, bjumps[:3].mean(0), rtol=1e-14)
    over = geo.GeoSummary(S, K)  # a known tip the device rounds to 1 + 2^-52 is written as 1
    m1 = marg[:1].copy()
    m1[0, 1] = [0.0, 1.0 + 2.0 ** -52, 0.0]
    over.add(rows[:1], m1, jumps[:1], bjumps[:1])
    assert over.marg.max() == 1.0 and np.array_equal(over.marg[1], [0.0, 1.0, 0.0])
    assert np.all(np.diag(acc.migrations) == 0.0) and np.array_equal(acc.times, np.diag(acc.jumps))


class HostSummaryLikelihood(go.HostGeoLikelihood):
    """The CPU suite's likelihood with ``evaluate_summaries`` on ``geo_summaries_host``."""

    def __init__(self, tips, peel0, max_draws=128, device=0):
        super().__init__(tips, peel0, max_draws=max_draws, device=device)
        self.max_draws = max_draws
        self.summary_calls = []
        self.finite = 0  # draws whose row had a finite log L

    def evaluate_summaries(self, blens, params):
        blens, params = np.atleast_2d(blens), np.atleast_2d(params)
        assert blens.shape[0] <= self.max_draws
        self.summary_calls.append(blens.shape[0])
        # the device's rule for a draw without a likelihood (the improper rate scale sends some vb draws to
        # inf): a -inf row and a zero summary
        ok = np.isfinite(params).all(axis=1)
        rows = np.zeros((blens.shape[0], 1 + self.B + self.R + self.K))
        rows[~ok, 0] = -np.inf
        if ok.any():
            rows[ok] = self.evaluate_rows(blens[ok], params[ok])
        each = [geo.geo_summaries_host(self.tips, self.peel, blens[n], params[n, :self.R], params[n, self.R:])
                for n in range(blens.shape[0])]
        self.finite += int(np.isfinite(rows[:, 0]).sum())
        return (rows,) + tuple(np.stack([e[k] for e in each]) for k in range(3))


def check_ancestral_files(out, S, K, tree_path):
    states = ["P%d" % k for k in range(K)]
    text = open(out + ".trees").read()
    assert text.startswith("#NEXUS") and len(re.findall(r"\btree \d+ = ", text)) == 1
    parsed = treeio.read_tree(out + ".trees")
    src = treeio.read_tree(tree_path)
    assert sorted(t.label for t in parsed.taxon_namespace) == sorted(t.label for t in src.taxon_namespace)
    assert len(list(parsed.postorder_node_iter())) == 2 * S - 1
    assert abs(sum(n.edge_length for n in parsed.postorder_node_iter() if n.parent_node is not None)
               - sum(n.edge_length for n in src.postorder_node_iter() if n.parent_node is not None)) < 1e-9
    locs = re.findall(r'location="([^"]*)"', text)
    assert len(locs) == 2 * S - 1 and set(locs) <= set(states)
    probs = [float(v) for v in re.findall(r"location\.prob=([^,\]]+)", text)]
    assert len(probs) == 2 * S - 1 and all(0.0 < p <= 1.0 for p in probs)
    sets = re.findall(r"location\.set=\{([^}]*)\}", text)
    setp = re.findall(r"location\.set\.prob=\{([^}]*)\}", text)
    assert len(sets) == len(setp) == 2 * S - 1
    for names, ps, loc, p in zip(sets, setp, locs, probs):
        names, ps = names.split(","), [float(v) for v in ps.split(",")]
        assert names[0] == '"%s"' % loc and ps[0] == p and len(names) == len(ps)
        assert all(0.0 < v <= 1.0 for v in ps) and sum(ps) <= 1.0 + 1e-9 and ps == sorted(ps, reverse=True)
    jumps = [float(v) for v in re.findall(r"jumps=([^,\]]+)", text)]
    assert len(jumps) == 2 * S - 2 and all(v >= 0.0 for v in jumps)
    table = [r.split("\t") for r in open(out + ".jumps.tsv").read().splitlines()]
    assert table[0][1:] == states + ["time"] and [r[0] for r in table[1:]] == states
    body = [r[1:] for r in table[1:]]
    assert all(body[i][i] == "" for i in range(K))
    tree_len = sum(n.edge_length for n in src.postorder_node_iter() if n.parent_node is not None)
    assert abs(sum(float(r[K]) for r in body) - tree_len) <= 1e-6
    moves = sum(float(body[i][j]) for i in range(K) for j in range(K) if i != j)
    assert abs(moves - sum(jumps)) <= 1e-6 * moves
    return moves, locs, probs


@pytest.mark.parametrize("algorithm", ["vb", "nuts"])
def test_run_geo_ancestral_end_to_end(tmp_path, capsys, algorithm):
    S, K = 8, 3
    tree, meta = go.write_geo_dataset(str(tmp_path), S=S, K=K, seed=4)
    out = str(tmp_path / "geo")
    argv = ["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree, "-o", out, "-S", "5"]
    if algorithm == "vb":
        argv += ["--iter", "200", "--elbo_samples", "10", "--samples", "25", "--tol_rel_obj", "0.01"]
        n_draws = 25
    else:
        argv += ["-a", "nuts", "--iter", "20", "--chains", "2"]
        n_draws = 20
    post, lines = go.run_geo(argv, factory=HostSummaryLikelihood)
    calls = post.lik.summary_calls
    assert sum(calls) == n_draws and max(calls) <= post.lik.max_draws  # every draw once, in chunks of max_draws
    if algorithm == "vb":
        assert calls == [10, 10, 5]
    moves, locs, probs = check_ancestral_files(out, S, K, tree)
    summary = [s for s in lines if s.startswith("Expected migrations")]
    assert len(summary) == 1
    m = re.match(r"Expected migrations: ([0-9.]+) over (\d+) draws; root location: (\S+) \(probability ([0-9.]+)\)",
                 summary[0])
    assert m and abs(float(m.group(1)) - moves) <= 1e-3
    assert int(m.group(2)) == post.lik.finite and int(m.group(2)) > n_draws // 2
    assert m.group(3) in ("P0", "P1", "P2") and 0.0 < float(m.group(4)) <= 1.0
    capsys.readouterr()


def test_without_the_switch_nothing_changes(tmp_path, capsys):
    tree, meta = go.write_geo_dataset(str(tmp_path), S=8, K=3, seed=4)
    out = str(tmp_path / "geo")
    post, lines = go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "-M", meta, "-t", tree, "-o", out, "-S", "5",
                              "--iter", "200", "--elbo_samples", "10", "--samples", "25", "--tol_rel_obj", "0.01"],
                             factory=HostSummaryLikelihood)
    assert post.lik.summary_calls == []
    import argparse
    from phylostan_amd import cli
    parser = argparse.ArgumentParser()
    run_parser = cli.create_run_parser(parser.add_subparsers())
    assert run_parser.parse_args(["-s", "m", "-t", "t", "-o", "o"]).ancestral is False  # opt-in
    assert not os.path.exists(out + ".trees") and not os.path.exists(out + ".jumps.tsv")
    assert not [s for s in lines if s.startswith("Expected migrations")]
    capsys.readouterr()


def test_ancestral_refusals(tmp_path):
    tree, meta = go.write_geo_dataset(str(tmp_path), S=6, K=3, seed=7)
    base = ["-s", str(tmp_path / "m.stan"), "-t", tree, "-o", str(tmp_path / "o")]
    with pytest.raises(SystemExit, match="--ancestral .* needs --geo"):
        go.run_geo(base + ["--ancestral"])
    with pytest.raises(SystemExit, match="evaluate_summaries"):  # a likelihood that cannot give the summaries
        go.run_geo(base + ["--geo", "--ancestral", "-M", meta])
    assert not os.path.exists(str(tmp_path / "o"))  # refused before anything is sampled or written


def test_summary_boundary_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_geo.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+phy_geo_summary_len\s*\(\s*const\s+phy_geo_ctx\s*\*", text)
    assert re.search(r"\bint\s+phy_geo_eval_summaries\s*\(\s*phy_geo_ctx\s*\*\s*ctx\s*,\s*int\s+n_draws\s*,"
                     r"\s*const\s+double\s*\*\s*blens\s*,\s*const\s+double\s*\*\s*params\s*,\s*double\s*\*\s*out\s*,"
                     r"\s*double\s*\*\s*summaries\s*\)", text)
    for name, nargs in (("phy_geo_summary_len", 1), ("phy_geo_eval_summaries", 6)):
        assert name in _lib.GEO_SIGNATURES and len(_lib.GEO_SIGNATURES[name][1]) == nargs
    assert re.search(r"\bint\s+phy_geo_eval\s*\(", text)  # the plain call stays
    src = open(os.path.join(ROOT, "phylostan_amd", "csrc", "geo_engine.inc")).read()
    assert "geo_kernel<false>" in src and "geo_kernel<true>" in src
