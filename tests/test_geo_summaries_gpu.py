"""GPU: ``phy_geo_eval_summaries`` -- node marginals, expected transitions and
dwell times, transitions per branch -- against the truths of
tests/geo_summary_truth.py (enumeration; complex-step derivatives with respect
to Q's own entries), the identities that tie the three arrays to each other and
to the gradient row, and the bitwise promises of the header.

Bars (the project's, as tests/test_geo_summaries_cpu.py): marginals absolute
1e-10, each count array within 1e-9 of its largest entry, row sums 1e-12, the
identities relative 1e-9.  A complex-step entry costs one evaluation of the
whole tree with K x K complex matrix exponentials, so up to K = 5 every entry
is compared with the truth and from K = 33 about 40 seeded (i, j) entries and
four seeded branches are, the rest being held to ``geo_summaries_host`` -- which
the CPU suite pins to the truth entry by entry -- at the same bar.  On the
69-tip tree at K = 64 one evaluation takes a quarter of a second: six entries
and two branches there.
"""
import functools
import os

import numpy as np
import pytest

from phylostan_amd import _lib, geo
from tests import geo_oracle as go
from tests import geo_summary_truth as gt
from tests.test_geo_summaries_cpu import JUMP_BAR, MARG_BAR, check_invariants

pytestmark = pytest.mark.gpu

PHY_EINVAL, PHY_ERANGE = 1, 4  # include/phylo_hip.h

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def make_case(S, K, seed, peel=None, missing=(0,)):
    """One all-ones tip (0) and one zero-length branch (1) in every case."""
    rng = np.random.default_rng(seed)
    peel = go.random_peel(S, rng) if peel is None else peel
    tips = go.random_tips(S, K, rng, missing=missing)
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens[0, 1] = 0.0
    return tips, peel, blens[0], params[0]


def evaluate(tips, peel, blens, params, max_draws=1):
    eng = geo.GeoLikelihood(tips, peel, max_draws=max_draws)
    try:
        return eng.evaluate_summaries(blens, params)
    finally:
        eng.close()


def check_draw(row, marg, jumps, bjumps, tips, peel, blens, params, entries=None, branches=None, seed=0,
               truth=True):
    """One draw's summaries against the truth (all entries, or a seeded subset)
    and the host restatement (every entry), then the identities."""
    S, K = tips.shape
    B, R = 2 * S - 3, geo.rate_count(K)
    rates, freqs = params[:R], params[R:]
    hm, hj, hb = geo.geo_summaries_host(tips, peel, blens, rates, freqs)
    rng = np.random.default_rng(seed)
    e_marg = np.abs(marg - hm).max()
    print("S %d K %d: marginals vs host %.2e" % (S, K, e_marg))
    assert e_marg <= MARG_BAR
    if K ** (2 * S - 2) <= 70000:
        e_enum = np.abs(marg - gt.brute_marginals(tips, peel, blens, rates, freqs)).max()
        print("  marginals vs enumeration %.2e" % e_enum)
        assert e_enum <= MARG_BAR
    sj, sb = np.abs(hj).max(), np.abs(hb).max()
    e_hj, e_hb = np.abs(jumps - hj).max() / sj, np.abs(bjumps - hb).max() / sb
    print("  jumps vs host %.2e, bjumps vs host %.2e of the largest entry" % (e_hj, e_hb))
    assert e_hj <= JUMP_BAR and e_hb <= JUMP_BAR
    if truth:
        pairs = [(i, j) for i in range(K) for j in range(K)]
        if entries is not None and len(pairs) > entries:
            pairs = [pairs[k] for k in np.sort(rng.choice(len(pairs), entries, replace=False))]
        tj = gt.jump_truth(tips, peel, blens, rates, freqs, entries=pairs)
        e_tj = max(abs(jumps[i, j] - v) for (i, j), v in tj.items()) / sj
        which = np.arange(B) if branches is None or B <= branches else np.sort(rng.choice(B, branches, replace=False))
        tb = gt.branch_jump_truth(tips, peel, blens, rates, freqs, branches=which)
        e_tb = np.abs(bjumps[which] - tb).max() / sb
        print("  jumps vs truth (%d entries) %.2e, bjumps vs truth (%d branches) %.2e" % (len(pairs), e_tj,
                                                                                           len(which), e_tb))
        assert e_tj <= JUMP_BAR and e_tb <= JUMP_BAR
    check_invariants(tips, peel, blens, rates, freqs, marg, jumps, bjumps, grad_blens=row[1:1 + B])


@functools.lru_cache(maxsize=None)
def flu_peel():
    from phylostan_amd import data as dataio
    tree = dataio.read_tree(os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.tree"))
    tree.resolve_polytomies(update_bipartitions=True)
    dataio.setup_indexes(tree)
    peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
    return peel0, geo.tree_branch_lengths(tree, peel0)


@pytest.mark.parametrize("K", [2, 3, 5, 33, 64])
@pytest.mark.parametrize("S", [3, 7])
def test_small_trees_every_k(S, K):
    """K = 2: one rotation pair; 3: the bye; 64: LDS full.  S = 3: a single
    peel level and the merged row.  Tip 0 is missing."""
    tips, peel, blens, params = make_case(S, K, 100 * S + K)
    rows, marg, jumps, bjumps = evaluate(tips, peel, blens, params)
    few = K >= 33
    check_draw(rows[0], marg[0], jumps[0], bjumps[0], tips, peel, blens, params, entries=40 if few else None,
               branches=4 if few else None)
    assert 0.0 < marg[0, 0].max() < 1.0  # the missing tip is imputed


@pytest.mark.parametrize("K,entries,branches", [(5, None, None), (64, 6, 2)])
def test_fluA_tree_synthetic_locations(K, entries, branches):
    peel, tree_blens = flu_peel()
    S = peel.shape[0] + 1
    assert S == 69
    tips, _, _, params = make_case(S, K, 69000 + K, peel=peel, missing=(0, 7, 40))
    blens = tree_blens * (0.3 / tree_blens.mean())
    blens[1] = 0.0
    rows, marg, jumps, bjumps = evaluate(tips, peel, blens, params)
    check_draw(rows[0], marg[0], jumps[0], bjumps[0], tips, peel, blens, params, entries=entries, branches=branches)


@pytest.mark.parametrize("K", [4, 17])
@pytest.mark.parametrize("arm", ["tie", "near"])
def test_repeated_eigenvalues(K, arm):
    """Equal rates and frequencies: a (K-1)-fold eigenvalue (Phi's tie arm,
    and an eigenbasis the solver is free to choose); one rate moved by 1e-11:
    its near arm."""
    tips, peel, blens, _ = make_case(9, K, 900 + K)
    rates = np.ones(geo.rate_count(K))
    if arm == "near":
        rates[1] += 1e-11
    params = np.concatenate([rates, np.full(K, 1.0 / K)])
    rows, marg, jumps, bjumps = evaluate(tips, peel, blens, params)
    check_draw(rows[0], marg[0], jumps[0], bjumps[0], tips, peel, blens, params, entries=40, branches=6)


BATCH_S, BATCH_K, BATCH_N = 7, 5, 300


@functools.lru_cache(maxsize=None)
def batch_case():
    tips, peel, _, _ = make_case(BATCH_S, BATCH_K, 77)
    blens, params = go.random_draws(BATCH_N, 2 * BATCH_S - 3, BATCH_K, np.random.default_rng(78))
    return tips, peel, blens, params


def test_rows_are_phy_geo_evals_and_summaries_do_not_depend_on_the_batch():
    """The rows of the summaries call are ``phy_geo_eval``'s bit for bit; a
    draw's summary is bitwise the same alone, in a batch of 300 (the workgroup
    loop when the device has fewer workgroups) and on a repeat; ``out`` may be
    NULL."""
    tips, peel, blens, params = batch_case()
    S, K, n = BATCH_S, BATCH_K, BATCH_N
    eng = geo.GeoLikelihood(tips, peel, max_draws=n)
    one = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        plain = eng.evaluate_rows(blens, params)
        rows, marg, jumps, bjumps = eng.evaluate_summaries(blens, params)
        assert rows.tobytes() == plain.tobytes()
        again = eng.evaluate_summaries(blens, params)
        for first, second in zip((rows, marg, jumps, bjumps), again):
            assert first.tobytes() == second.tobytes()
        assert eng.evaluate_rows(blens, params).tobytes() == plain.tobytes()  # and the plain call after it
        for k in (0, n // 2, n - 1):
            alone = one.evaluate_summaries(blens[k], params[k])
            for batch, single in zip((rows, marg, jumps, bjumps), alone):
                assert batch[k].tobytes() == single[0].tobytes(), k
        slen = eng.lib.phy_geo_summary_len(eng.ctx)
        assert slen == geo.summary_len(S, K) == (2 * S - 1) * K + K * K + 2 * S - 3
        flat = np.empty((4, slen))
        b4, p4 = np.ascontiguousarray(blens[:4]), np.ascontiguousarray(params[:4])
        _lib.check(eng.lib.phy_geo_eval_summaries(eng.ctx, 4, b4.ctypes.data, p4.ctypes.data, None, flat.ctypes.data),
                   "phy_geo_eval_summaries")
        for got, want in zip(geo.split_summaries(flat, S, K), (marg, jumps, bjumps)):
            assert got.tobytes() == want[:4].tobytes()
    finally:
        eng.close()
        one.close()
    R = geo.rate_count(K)
    for k in (1, 150, 299):  # and they are right, not only repeatable
        check_draw(rows[k], marg[k], jumps[k], bjumps[k], tips, peel, blens[k], params[k], seed=k)
        check_invariants(tips, peel, blens[k], params[k, :R], params[k, R:], marg[k], jumps[k], bjumps[k])


def test_more_draws_than_workgroups():
    """At K = 64 the LDS admits one workgroup per CU, so a 300-draw call loops
    on a device of fewer than 300 CUs: a draw of the second pass is bitwise the
    draw alone, and right."""
    S, K, n = 5, 64, 300
    tips, peel, _, _ = make_case(S, K, 64300)
    blens, params = go.random_draws(n, 2 * S - 3, K, np.random.default_rng(64301))
    eng = geo.GeoLikelihood(tips, peel, max_draws=n)
    one = geo.GeoLikelihood(tips, peel, max_draws=1)
    try:
        assert eng.info()["workgroups"] < n
        batch = eng.evaluate_summaries(blens, params)
        for k in (0, n - 1):
            alone = one.evaluate_summaries(blens[k], params[k])
            for b, a in zip(batch, alone):
                assert b[k].tobytes() == a[0].tobytes(), k
    finally:
        eng.close()
        one.close()
    k = n - 1
    check_draw(batch[0][k], batch[1][k], batch[2][k], batch[3][k], tips, peel, blens[k], params[k], truth=False)


def test_a_bad_draw_in_a_batch():
    """A NaN parameter: a -inf row and a zero summary; the neighbours are
    bitwise what they are without it."""
    tips, peel, blens, params = batch_case()
    n = 5
    bad = params[:n].copy()
    bad[2, 1] = np.nan
    eng = geo.GeoLikelihood(tips, peel, max_draws=n)
    try:
        good = eng.evaluate_summaries(blens[:n], params[:n])
        got = eng.evaluate_summaries(blens[:n], bad)
    finally:
        eng.close()
    rows, marg, jumps, bjumps = got
    assert rows[2, 0] == -np.inf and np.all(rows[2, 1:] == 0.0)
    assert np.all(marg[2] == 0.0) and np.all(jumps[2] == 0.0) and np.all(bjumps[2] == 0.0)
    keep = [0, 1, 3, 4]
    for a, b in zip(good, got):
        assert a[keep].tobytes() == b[keep].tobytes()
        assert np.all(np.isfinite(b[keep]))
    assert np.all(good[1][2].sum(1) > 0.5)  # the draw itself has a summary when its parameters are sound


def test_past_the_fp64_range():
    """600 tips: the likelihood itself underflows; the marginals and counts are
    ratios in which every power-of-two scale cancels."""
    S, K = 600, 5
    rng = np.random.default_rng(600)
    peel = go.random_peel(S, rng)
    tips = go.random_tips(S, K, rng, missing=(3, 200))
    blens, params = go.random_draws(1, 2 * S - 3, K, rng)
    blens, params = blens[0], params[0]
    rows, marg, jumps, bjumps = evaluate(tips, peel, blens, params)
    assert np.isfinite(rows[0, 0]) and rows[0, 0] < np.log(np.finfo(np.float64).tiny)
    check_draw(rows[0], marg[0], jumps[0], bjumps[0], tips, peel, blens, params, truth=False)


def test_refusals():
    tips, peel, blens, params = make_case(7, 4, 1)
    lib = _lib.load()
    assert lib.phy_geo_summary_len(None) == -1
    S, K = tips.shape
    flat = np.empty((3, geo.summary_len(S, K)))
    out = np.empty((3, 1 + (2 * S - 3) + geo.rate_count(K) + K))
    b3, p3 = np.tile(blens, (3, 1)), np.tile(params, (3, 1))
    args = (b3.ctypes.data, p3.ctypes.data, out.ctypes.data, flat.ctypes.data)
    assert lib.phy_geo_eval_summaries(None, 1, *args) == PHY_EINVAL
    eng = geo.GeoLikelihood(tips, peel, max_draws=2)
    try:
        for n in (0, -1, 3):
            with pytest.raises(_lib.PhyloHipError, match="n_draws out of range"):
                _lib.check(lib.phy_geo_eval_summaries(eng.ctx, n, *args), "phy_geo_eval_summaries")
        assert lib.phy_geo_eval_summaries(eng.ctx, 3, *args) == PHY_ERANGE
        with pytest.raises(_lib.PhyloHipError, match="NULL host buffer"):
            _lib.check(lib.phy_geo_eval_summaries(eng.ctx, 2, b3.ctypes.data, p3.ctypes.data, out.ctypes.data, None),
                       "phy_geo_eval_summaries")
        with pytest.raises(_lib.PhyloHipError, match="NULL host buffer"):
            _lib.check(lib.phy_geo_eval_summaries(eng.ctx, 2, None, p3.ctypes.data, out.ctypes.data,
                                                  flat.ctypes.data), "phy_geo_eval_summaries")
        with pytest.raises(_lib.PhyloHipError, match="n_draws out of range"):
            eng.evaluate_summaries(b3, p3)
        rows, marg, _, _ = eng.evaluate_summaries(b3[:2], p3[:2])  # the context still works
        assert np.all(np.isfinite(rows)) and np.abs(marg.sum(2) - 1.0).max() <= 1e-12
    finally:
        eng.close()


def test_cli_run_geo_ancestral_on_the_engine(tmp_path):
    """run --geo --ancestral -a nuts, 2 chains x (15 + 15), on the device engine
    and the CPU suite's data set (S = 8, K = 3): the files of its check, written
    from the device's summaries of the 30 kept draws."""
    from tests.test_geo_summaries_cpu import check_ancestral_files
    tree, meta = go.write_geo_dataset(str(tmp_path), S=8, K=3, seed=4)
    out = str(tmp_path / "geo")
    post, lines = go.run_geo(["-s", str(tmp_path / "m.stan"), "--geo", "--ancestral", "-M", meta, "-t", tree, "-o", out,
                              "-S", "5", "-a", "nuts", "--iter", "30", "--chains", "2"], host=False)
    check_ancestral_files(out, 8, 3, tree)
    summary = [s for s in lines if s.startswith("Expected migrations")]
    assert len(summary) == 1 and " over 30 draws" in summary[0]
