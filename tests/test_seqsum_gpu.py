"""GPU: the sequence-summary engine (include/phylo_hip_seqsum.h) -- rows
against the clamping truth of tests/seqsum_truth.py, bitwise independence of a
draw from the rest of its call, the ordered running sum, rejected draws,
misuse, expected substitutions from device rows and ``run --ancestral_seq``
on the device."""
import ctypes
import os

import numpy as np
import pytest

from phylostan_amd import _lib, cli, models, seqsum
from tests import cases, fixture_files, seqsum_cases as sc, seqsum_truth
from tests.test_gpu_parity import RTOL_LL

pytestmark = pytest.mark.gpu


def _engine(case, max_draws=8):
    return seqsum.SequenceSummaries(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                                    max_draws=max_draws)


def _parity(case, key):
    eng = _engine(case, 2)
    row = eng.evaluate_rows(case.blens, case.model_vec())[0]
    eng.close()
    assert row.shape == (1 + (4 * (case.S - 1) + case.C + 1) * case.P,)
    want = sc.truth(key)
    ref = case.oracle()["loglik"]
    print("%s loglik %.12f oracle %.12f" % (key, row[0], ref))
    assert abs(row[0] - ref) <= RTOL_LL * abs(ref)
    sc.check_row(row, case, want, "device %s" % (key,))
    return row


@pytest.mark.parametrize("k", range(len(sc.SHAPES)))
def test_rows_against_the_clamping_truth(k):
    _parity(sc.shape_case(k), k)


@pytest.mark.parametrize("kind", sc.TREES)
def test_rows_on_a_caterpillar_and_a_balanced_tree(kind):
    _parity(sc.tree_case(kind), kind)


def test_an_all_missing_pattern_is_the_prior():
    case = sc.missing_case()
    row = _parity(case, "missing")
    _, anc, cat, _ = seqsum.split_row(row, case.S, case.P, case.C)
    assert np.abs(anc[:, :, 64] - case.freqs[None, :]).max() < 1e-10
    assert np.abs(cat[:, 64] - case.ps).max() < 1e-10


def test_a_draw_is_bitwise_its_own():
    case = sc.draws_case()
    bl, mv = sc.draws(case, 5)
    eng = _engine(case, 8)
    rows = eng.evaluate_rows(bl, mv)
    np.testing.assert_array_equal(eng.evaluate_rows(bl, mv), rows)  # two calls, the same bits
    assert len({rows[k].tobytes() for k in range(5)}) == 5
    alone = eng.evaluate_rows(bl[3:4], mv[3:4])[0]
    np.testing.assert_array_equal(alone, rows[3])
    for pos in (0, 2, 4):  # first, middle and last of 5
        order = [k for k in range(5) if k != 3]
        order.insert(pos, 3)
        got = eng.evaluate_rows(bl[order], mv[order])
        np.testing.assert_array_equal(got[pos], alone)
    eng.close()
    other = _engine(case, 3)  # another max_draws: calls of 5 are chunked 3 + 2
    np.testing.assert_array_equal(other.evaluate_rows(bl, mv), rows)
    other.close()


def test_the_running_sum_is_sequential_in_draw_order():
    case = sc.draws_case()
    bl, mv = sc.draws(case, 7, seed=9)
    eng = _engine(case, 8)
    rows = eng.evaluate_rows(bl, mv)
    want = np.zeros(eng.row_len)
    for r in rows:
        want = want + r
    for split in ([7], [3, 4], [1] * 7):
        eng.reset()
        at, ll = 0, []
        for n in split:
            ll.append(eng.add(bl[at:at + n], mv[at:at + n]))
            at += n
        total, nfin = eng.read()
        assert nfin == 7
        np.testing.assert_array_equal(np.concatenate(ll), rows[:, 0])
        np.testing.assert_array_equal(total, want)
    eng.reset()
    total, nfin = eng.read()
    assert nfin == 0 and not total.any()
    eng.close()


def test_a_call_split_into_launches_keeps_bits_and_order():
    """A draw's workspace of 264 MB: the fixed budget gives 3 draws a launch, so
    a call of 5 is two launches -- the rows and the sum do not change."""
    case = cases.random_case(12, S=64, P=4096, C=16, model="HKY")
    plan = seqsum.plan_seqsum(case.tipcodes, case.peel0, True, 16, 5, "HKY")
    assert 1 <= plan["draws_per_launch"] < 5 and plan["workspace_bytes"] == 2 * 63 * 16 * 4 * 4096 * 8
    bl, mv = sc.draws(case, 5)
    eng = _engine(case, 5)
    rows = eng.evaluate_rows(bl, mv)
    assert np.all(np.isfinite(rows[:, 0]))
    for k in (0, 2, 3, 4):
        np.testing.assert_array_equal(eng.evaluate_rows(bl[k:k + 1], mv[k:k + 1])[0], rows[k])
    eng.reset()
    np.testing.assert_array_equal(eng.add(bl, mv), rows[:, 0])
    total, nfin = eng.read()
    want = np.zeros(eng.row_len)
    for r in rows:
        want = want + r
    assert nfin == 5
    np.testing.assert_array_equal(total, want)
    eng.close()


def test_rejected_draws():
    case = sc.draws_case()
    bl, mv = sc.draws(case, 5)
    eng = _engine(case, 8)
    good = eng.evaluate_rows(bl, mv)
    bl[2, 3] = np.nan      # a NaN branch length in draw 2
    mv[0, 1] = -0.1        # a negative frequency in draw 0
    rows = eng.evaluate_rows(bl, mv)
    for k in (0, 2):
        assert rows[k, 0] == -np.inf and not rows[k, 1:].any()
    for k in (1, 3, 4):
        np.testing.assert_array_equal(rows[k], good[k])
    eng.reset()
    ll = eng.add(bl, mv)
    total, nfin = eng.read()
    assert nfin == 3 and list(ll == -np.inf) == [True, False, True, False, False]
    np.testing.assert_array_equal(ll[[1, 3, 4]], good[[1, 3, 4], 0])
    want = np.zeros(eng.row_len)
    for k in (1, 3, 4):
        want = want + good[k]
    np.testing.assert_array_equal(total, want)
    eng.close()


def test_misuse_returns_the_documented_codes():
    case = sc.draws_case()
    eng = _engine(case, 4)
    lib, ctx = eng.lib, eng.ctx
    bl, mv = sc.draws(case, 5)
    rows, ll = np.empty((5, eng.row_len)), np.empty(5)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
    EINVAL, ERANGE = 1, 4
    for n in (0, 5):
        assert lib.phy_seqsum_eval(ctx, n, p(bl), p(mv), p(rows)) == ERANGE
        assert lib.phy_seqsum_add(ctx, n, p(bl), p(mv), p(ll)) == ERANGE
    assert lib.phy_seqsum_eval(ctx, 1, None, p(mv), p(rows)) == EINVAL
    assert lib.phy_seqsum_eval(ctx, 1, p(bl), None, p(rows)) == EINVAL
    assert lib.phy_seqsum_eval(ctx, 1, p(bl), p(mv), None) == EINVAL
    assert lib.phy_seqsum_add(ctx, 1, p(bl), p(mv), None) == EINVAL
    assert lib.phy_seqsum_read(ctx, None, None) == EINVAL
    assert lib.phy_seqsum_eval(None, 1, p(bl), p(mv), p(rows)) == EINVAL
    assert lib.phy_seqsum_add(None, 1, p(bl), p(mv), p(ll)) == EINVAL
    assert lib.phy_seqsum_reset(None) == EINVAL and lib.phy_seqsum_read(None, p(rows), None) == EINVAL
    assert lib.phy_seqsum_num_branches(None) == -1 and lib.phy_seqsum_row_len(None) == -1
    assert lib.phy_seqsum_num_branches(ctx) == case.blens.size
    out = ctypes.c_void_p()
    tips, w, peel = case.tipcodes, np.ascontiguousarray(case.weights), np.ascontiguousarray(case.peel0, np.int32)
    assert lib.phy_seqsum_create(2, case.P, case.C, 1, 2, p(tips), p(w), p(peel), 4, 0, ctypes.byref(out)) == EINVAL
    assert lib.phy_seqsum_create(case.S, case.P, 17, 1, 2, p(tips), p(w), p(peel), 4, 0, ctypes.byref(out)) == EINVAL
    assert lib.phy_seqsum_create(case.S, case.P, case.C, 1, 2, p(tips), p(w), p(peel), 0, 0, ctypes.byref(out)) == EINVAL
    assert not out.value
    assert eng.evaluate_rows(bl[:1], mv[:1]).shape == (1, eng.row_len)  # the context still works
    eng.close()


@pytest.mark.parametrize("model", ["GTR", "JC69"])
def test_expected_substitutions_from_device_rows(model):
    from phylostan_amd.engine import TreeLikelihood
    case = cases.random_case(21, S=7, P=40, C=3, model=model)
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C)
    res = eng.evaluate(case.blens, case.model_vec())
    eng.close()
    got = models.expected_substitutions(res.dLdP, case.blens, case.rs, case.freqs, case.rates)
    want = seqsum_truth.expected_substitutions(case)
    err = float(np.abs(got - want).max() / np.abs(want).max())
    print("%s: expected substitutions from device rows, max error / largest entry %.2e" % (model, err))
    assert err < 1e-9


def test_cli_ancestral_seq_on_the_device(tmp_path, capsys):
    from tests.test_seqsum_cpu import MODEL, _args, check_outputs
    S = 8
    case = cases.random_case(8, S=S, P=40, C=1, model="HKY")
    # an alignment of 40 distinct columns (a repeat of some: weights 1..4)
    t, _ = fixture_files.write_random_dataset(str(tmp_path), seed=6, S=S, sites=10)
    sym = {1: "A", 2: "C", 4: "G", 8: "T"}
    cols = np.repeat(np.arange(40), case.weights.astype(int))
    a = str(tmp_path / "forty.fa")
    with open(a, "w") as fp:
        for s in range(S):
            fp.write(">t%d_%d\n%s\n" % (s, s, "".join(sym.get(int(c), "-") for c in case.tipcodes[s, cols])))
    out = str(tmp_path / "dev")
    lines = []
    cli.run(_args(["-s", str(tmp_path / "m.stan")] + MODEL + ["-t", t, "-i", a, "-o", out, "-S", "3", "--ancestral_seq",
                                                             "-a", "vb", "--iter", "200", "--samples", "20",
                                                             "--elbo_samples", "10", "--tol_rel_obj", "0.01"]),
            log=lines.append)
    capsys.readouterr()
    P = check_outputs(out, S, cols.size, 4, lines, 20)
    assert 30 <= P <= 40
    assert os.path.exists(out + ".trees") and os.path.exists(out)
