"""GPU: the forest engine (include/phylo_hip_forest.h) -- every row of a call
on its own tree against the C oracle at the parity bar of
tests/test_gpu_parity.py, and bit for bit independent of the rest of the call
and of the context's other trees."""
import os

import numpy as np
import pytest

from tests import cases, forest_cases as fc
from tests.test_gpu_parity import RTOL_G, RTOL_LL, _close

pytestmark = pytest.mark.gpu


def rows_vs_truth(rows, site, truth_rows, truth_site, what=""):
    for k, (r, ref) in enumerate(zip(rows, truth_rows)):
        assert abs(r[0] - ref[0]) <= RTOL_LL * abs(ref[0]), "%s row %d: log-likelihood %r vs %r" % (what, k, r[0], ref[0])
        _close(r[1:], ref[1:], RTOL_G, "%s row %d" % (what, k))
    if site is not None:
        np.testing.assert_allclose(site, truth_site, rtol=RTOL_LL, atol=1e-12)


def bitwise_legs(f, eng, rows, site, max_rows):
    """The independence contract: permuted, alone, padded to max_rows with
    other trees' rows, and from a context holding only the trees used."""
    n = len(f.tree_of_row)
    perm = np.random.default_rng(5).permutation(n)
    r2, s2 = eng.evaluate_rows(f.tree_of_row[perm], f.blens[perm], f.model_vecs[perm], site_ll=True)
    np.testing.assert_array_equal(r2, rows[perm])
    np.testing.assert_array_equal(s2, site[perm])
    for k in range(n):
        r1, s1 = eng.evaluate_rows(f.tree_of_row[k:k + 1], f.blens[k:k + 1], f.model_vecs[k:k + 1], site_ll=True)
        np.testing.assert_array_equal(r1[0], rows[k])
        np.testing.assert_array_equal(s1[0], site[k])
    pad = max_rows - n
    assert pad > 0
    rng = np.random.default_rng(6)
    pt = rng.integers(0, f.peels.shape[0], pad).astype(np.int32)
    pb, pm = fc.random_rows(rng, pad, f.B, f.C, f.model)
    where = np.sort(rng.choice(max_rows, n, replace=False))
    tree, bl, mv = np.empty(max_rows, np.int32), np.empty((max_rows, f.B)), np.empty((max_rows, f.model_vecs.shape[1]))
    rest = np.setdiff1d(np.arange(max_rows), where)
    tree[where], bl[where], mv[where] = f.tree_of_row, f.blens, f.model_vecs
    tree[rest], bl[rest], mv[rest] = pt, pb, pm
    r3, s3 = eng.evaluate_rows(tree, bl, mv, site_ll=True)
    np.testing.assert_array_equal(r3[where], rows)
    np.testing.assert_array_equal(s3[where], site)
    used = np.unique(f.tree_of_row)
    if len(used) < f.peels.shape[0]:
        sub = f.engine(max_rows, peels=f.peels[used])
        same_plan = sub.info() == eng.info()
        if same_plan:
            r4 = sub.evaluate_rows(np.searchsorted(used, f.tree_of_row), f.blens, f.model_vecs)
            np.testing.assert_array_equal(r4, rows)
        sub.close()
        return same_plan
    return None


@pytest.mark.parametrize("max_rows,cols", [(16, 1), (600, 2)])
@pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])
@pytest.mark.parametrize("model", ["JC69", "HKY", "GTR"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("P", [70, 130])
def test_rows_against_the_oracle(P, C, model, rooted, max_rows, cols):
    f = fc.random_forest(3, 8, P, C, model, rooted)
    eng = f.engine(max_rows)
    info = eng.info()
    assert info["cols"] == cols and info["min_depth"] == 0 and info["max_depth"] >= 1
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    rows_vs_truth(rows, site, *f.truth())
    eng.close()


@pytest.mark.parametrize("max_rows", [16, 600])
@pytest.mark.parametrize("P,C,model,rooted", [(70, 1, "JC69", False), (130, 3, "GTR", True), (130, 3, "HKY", False)])
def test_bitwise_independence(P, C, model, rooted, max_rows):
    # tree 3 is not used: the plan stands without it
    f = fc.random_forest(3, 8, P, C, model, rooted, tree_of_row=(1, 0, 0, 2, 1, 2, 0))
    eng = f.engine(max_rows)
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    rows_vs_truth(rows, site, *f.truth())
    again = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs)
    np.testing.assert_array_equal(again, rows)
    same_plan = bitwise_legs(f, eng, rows, site, max_rows)
    eng.close()
    if same_plan is False:
        pytest.skip("the sub-forest's plan differs: that leg does not apply (every other leg passed)")


FORCED = [
    ("lds16k", {"PHY_LDS_BUDGET": "16384"}, 24, 4, True),
    ("cols1", {"PHY_COLS": "1"}, 12, 3, True),
    ("cols2", {"PHY_COLS": "2"}, 12, 3, False),
    ("deep1", {"PHY_DEEP": "1"}, 12, 3, True),
    ("deep2", {"PHY_DEEP": "2"}, 12, 3, False),
    ("deep2cols2", {"PHY_DEEP": "2", "PHY_COLS": "2"}, 12, 2, True),
    ("norecompute", {"PHY_RECOMPUTE": "0"}, 12, 3, True),
    ("nofin", {"PHY_FIN": "0"}, 12, 3, True),
    ("noqfuse", {"PHY_QFUSE": "0", "PHY_FIN": "0"}, 12, 3, False),
    ("C10", {}, 12, 10, True),  # C > 8: the one-column 1,024-thread form
]


@pytest.mark.parametrize("name,env,S,C,rooted", FORCED, ids=[r[0] for r in FORCED])
def test_forced_plans(name, env, S, C, rooted, monkeypatch):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    f = fc.random_forest(11, S, 130, C, "GTR" if C != 10 else "HKY", rooted, tree_of_row=(2, 0, 0, 1, 2, 1, 0),
                         seeds=(1,))
    eng = f.engine(12)
    info = eng.info()
    if name == "lds16k":
        # the trees' chunk boundaries over their programs differ (first step of every chunk, ST_CHUNK = column 11)
        from phylostan_amd.engine import plan_records
        bounds = {tuple(np.flatnonzero(np.diff(plan_records(p, rooted, C, 5, info["cols"], info["cap_m"])[0][:, 11])))
                  for p in f.peels}
        assert info["lds_bytes"] <= 16384 and info["max_chunks"] >= 2, info
        assert info["min_chunks"] != info["max_chunks"] or len(bounds) > 1, (info, bounds)
    if name.startswith("cols"):
        assert info["cols"] == int(name[4])
    if name == "deep1":
        assert info["deep_in_lds"] == info["max_depth"] >= 1
    if name.startswith("deep2"):
        assert info["deep_in_lds"] == 0 and info["max_depth"] >= 1
    if name == "C10":
        assert info["cols"] == 1
    rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
    rows_vs_truth(rows, site, *f.truth(), what=name)
    bitwise_legs(f, eng, rows, site, 12)
    eng.close()


def test_ds1_all_topologies_in_one_call():
    from oracle import cpu
    tip0, w, peels, blens, site_ref, ll_ref = fc.ds1_forest()
    T, S = peels.shape[0], tip0.shape[0]
    assert T == 42 and np.all(peels[:, -1, 1] == 2 * S - 3)
    mv = cases.ds1_case().model_vec()
    from phylostan_amd.forest import ForestLikelihood
    eng = ForestLikelihood(tip0, w, peels, False, "JC69", 1, max_rows=3 * T)
    assert eng.info()["cols"] == 2
    rows, site = eng.evaluate_rows(np.arange(T), blens, np.repeat(mv[None], T, axis=0), site_ll=True)
    np.testing.assert_allclose(site, site_ref, rtol=RTOL_LL, atol=1e-12)
    assert np.all(np.abs(rows[:, 0] - ll_ref) <= RTOL_LL * np.abs(ll_ref))
    # three rows per tree, interleaved: the fixture's point and two scaled ones
    tree3 = np.tile(np.arange(T), 3)
    bl3 = np.concatenate([blens, 0.7 * blens, 1.4 * blens])
    rows3, site3 = eng.evaluate_rows(tree3, bl3, np.repeat(mv[None], 3 * T, axis=0), site_ll=True)
    np.testing.assert_array_equal(rows3[:T], rows)
    np.testing.assert_array_equal(site3[:T], site)
    truth = [cpu.evaluate(tip0, w, peels[t], False, 0, mv, bl, 1, site_ll=True) for t, bl in zip(tree3, bl3)]
    rows_vs_truth(rows3, site3, [o[:eng.outlen] for o, _ in truth], [s for _, s in truth], what="DS1")
    eng.close()


def test_flua_sized_forest():
    base = cases.fluA_case()
    S = base.S
    peels = np.array([base.peel0] + [cases.random_peel(S, np.random.default_rng(s)) for s in (1, 2, 3)], dtype=np.int32)
    tree = np.array([0, 1, 2, 3, 3, 0, 2, 1], dtype=np.int32)
    rng = np.random.default_rng(9)
    bl = base.blens[None] * rng.uniform(0.5, 1.5, (8, base.blens.size))
    _, mvs = fc.random_rows(rng, 8, base.blens.size, 4, "HKY")
    f = fc.Forest(base.tipcodes, base.weights, peels, True, "HKY", 4, tree, bl, mvs)
    eng = f.engine(8)
    rows, site = eng.evaluate_rows(tree, bl, mvs, site_ll=True)
    rows_vs_truth(rows, site, *f.truth(), what="fluA-sized")
    eng.close()


def test_one_tree_forest_matches_tree_likelihood():
    from phylostan_amd.engine import TreeLikelihood
    case = cases.random_case(21, S=12, P=200, C=3, model="GTR")
    f = fc.Forest(case.tipcodes, case.weights, case.peel0[None], True, "GTR", 3, [0, 0, 0],
                  *fc.random_rows(np.random.default_rng(2), 3, case.blens.size, 3, "GTR"))
    eng = f.engine(4)
    rows = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs)
    single = TreeLikelihood(case.tipcodes, case.weights, case.peel0, True, "GTR", 3, max_draws=4)
    single.set_output(compact=True)
    ref = single.evaluate_rows(f.blens, f.model_vecs)
    rows_vs_truth(rows, None, ref, None, what="T = 1")
    single.close()
    eng.close()


def test_bad_rows_and_refusals():
    from phylostan_amd import _lib
    f = fc.random_forest(3, 8, 70, 3, "HKY", True)
    eng = f.engine(16)
    rows = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs)
    bl, mv = f.blens.copy(), f.model_vecs.copy()
    mv[2, 1] = -0.2      # a negative frequency
    bl[5, 3] = np.nan    # a NaN branch length
    bad = eng.evaluate_rows(f.tree_of_row, bl, mv)
    for k in (2, 5):
        assert bad[k, 0] == -np.inf and not bad[k, 1:].any()
    keep = [k for k in range(len(rows)) if k not in (2, 5)]
    np.testing.assert_array_equal(bad[keep], rows[keep])
    lib, ctx = eng.lib, eng.ctx
    tree = np.ascontiguousarray(f.tree_of_row)
    out = np.empty((len(tree), eng.outlen))
    p = lambda a: a.ctypes.data  # noqa: E731
    good = (p(tree), p(f.blens), p(f.model_vecs), p(out), None)
    PHY_EINVAL, PHY_ERANGE = 1, 4
    assert lib.phy_forest_eval(ctx, 0, *good) == PHY_ERANGE
    assert lib.phy_forest_eval(ctx, 17, *good) == PHY_ERANGE
    for t in (-1, 4):
        tb = tree.copy()
        tb[6] = t
        assert lib.phy_forest_eval(ctx, len(tree), p(tb), *good[1:]) == PHY_ERANGE
        assert b"row 6" in lib.phy_last_error()
    assert lib.phy_forest_eval(None, len(tree), *good) == PHY_EINVAL
    for hole in range(4):
        args = list(good)
        args[hole] = None
        assert lib.phy_forest_eval(ctx, len(tree), *args) == PHY_EINVAL
    assert lib.phy_forest_num_trees(None) == -1 and lib.phy_forest_num_trees(ctx) == 4
    # still good after the refusals
    np.testing.assert_array_equal(eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs), rows)
    eng.close()
    peels = f.peels.copy()
    peels[2, 0, 0] = 99
    with pytest.raises(_lib.PhyloHipError, match="tree 2"):
        f.engine(4, peels=peels)
    with pytest.raises(_lib.PhyloHipError, match="T >= 1"):
        f.engine(4, peels=f.peels[:0])


def test_cli_topologies_on_the_device(tmp_path):
    from phylostan_amd import cli, stan_io
    from tests.test_forest_cpu import _args, _dataset
    tree, aln, tops = _dataset(tmp_path)
    out = str(tmp_path / "dev")
    post, results = cli.run(_args(["-s", str(tmp_path / "m.stan"), "-m", "JC69", "-t", tree, "-i", aln, "-o", out,
                                   "-S", "5", "--iter", "200", "--elbo_samples", "10", "--samples", "20",
                                   "--topologies", tops]), log=lambda *_: None)
    rows = [ln.split("\t") for ln in open(out + ".topologies.tsv").read().splitlines()]
    assert rows[0] == ["tree", "iterations", "converged", "eta", "elbo", "log_ml_is", "posterior"] and len(rows) == 4
    elbo = np.array([float(r[4]) for r in rows[1:]])
    prob = np.array([float(r[6]) for r in rows[1:]])
    assert np.all(np.isfinite(elbo)) and abs(prob.sum() - 1.0) < 1e-12
    for k in range(3):
        assert results[k].error is None and results[k].iterations > 0
        header, data = stan_io.read_samples("%s_tree%d" % (out, k))
        assert data.shape == (21, len(header))
        assert os.path.exists("%s_tree%d.diag" % (out, k)) and os.path.exists("%s_tree%d.trees" % (out, k))
