"""GPU: the K-state sequence engine and its mixture (``csrc/kseq_engine.inc``)
where the shape lists of ``test_kseq_gpu`` and ``test_kseq_mix_gpu`` do not go.

* ``kseq_truth.edge_cases()`` and ``kseq_mix_truth.edge_cases()`` against their
  recorded truths at the project's bars: zero-length and 1e-8 branches, short
  codon branches, the +I category 1023 bits and more below a deep tree's shift,
  KT = 48 (K = 33, 40, 48: three row blocks, 192-thread workgroups), K = 32 and
  49, C = 16, M = 8 with G = 16.
* The work-distribution loops: 2560 items on a grid of at most half as many
  workgroups (``item += gridDim.x`` of the up and down kernels), and more draws
  than the device has compute units (``dm += gridDim.x`` of the eigen and combine
  kernels, ``dl += gridDim.x`` of the site kernel), with refused draws among the
  good ones.  Each asserts from the live plan that its loop turns; rows are
  compared bit for bit with the same draws where no loop turns, and with the
  truth.
* Zero-weight patterns, of positive and of exactly zero likelihood.
"""
import numpy as np
import pytest

from phylostan_amd.kseq import DeviceKStateLikelihood, DeviceKStateMixLikelihood
from tests import kseq_mix_truth as mt
from tests import kseq_truth as kt
from tests import test_kseq_cpu as tk
from tests import test_kseq_mix_cpu as tm

pytestmark = pytest.mark.gpu

EDGES = kt.edge_cases()
MIX_EDGES = mt.edge_cases()
BAD = (7, 40)  # the refused draws of the item-loop test: a negative rate, a NaN ps


def _device(case, **kw):
    return DeviceKStateLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.C, **kw)


def _mix_device(case, **kw):
    return DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C, **kw)


@pytest.mark.parametrize("case", EDGES, ids=[c.name for c in EDGES])
def test_device_on_the_edge_cases(case):
    lik = _device(case, max_draws=2)
    info = lik.info()
    rows, site = lik.evaluate_rows(case.blens[None], case.params[None], site_ll=True)
    lik.close()
    assert info["KT"] == 16 * ((case.K + 15) // 16) and info["threads"] == 4 * info["KT"]
    tk.check_edge_case(case, rows, site)


@pytest.mark.parametrize("case", MIX_EDGES, ids=[c.name for c in MIX_EDGES])
def test_mix_device_on_the_edge_cases(case):
    lik = _mix_device(case, max_draws=2)
    err, _, _, _ = tm.check_against_truth(lik, case)
    lik.close()
    assert not mt.bars(err), err


def _scaled(n):
    """n distinct factors for the branch lengths, 0.5 .. 1.5."""
    return 0.5 + np.arange(n) / float(n)


def _item_loop_draws(case, n=64):
    blens = case.blens[None] * _scaled(n)[:, None]
    params = np.repeat(case.params[None], n, 0)
    params[BAD[0], 3] = -0.1  # a rate of the first model
    params[BAD[1], -1] = np.nan  # the last ps
    return blens, params


def _assert_items_loop(info, n):
    assert info["chunk_draws"] >= n and info["items_per_draw"] == 40
    assert info["workgroups"] * 2 <= n * info["items_per_draw"], info  # every workgroup takes two items or more


def test_item_loop_with_bad_draws_among_the_good():
    # K = 4, S = 3, P = 145 (10 tiles), C = 4: 40 items a draw, 2560 in a call of 64
    case = kt.random_case("K4_S3_P145_C4_rooted", 3, 4, 145, 4, True, 60)
    n = 64
    blens, params = _item_loop_draws(case, n)
    lik = _device(case, max_draws=n)
    _assert_items_loop(lik.info(), n)
    rows, site = lik.evaluate_rows(blens, params, site_ll=True)
    for k in range(n):
        if k in BAD:
            assert rows[k, 0] == -np.inf and not rows[k, 1:].any() and np.all(site[k] == -np.inf)
            continue
        one, one_site = lik.evaluate_rows(blens[k:k + 1], params[k:k + 1], site_ll=True)  # 40 items: no second turn
        np.testing.assert_array_equal(rows[k], one[0])
        np.testing.assert_array_equal(site[k], one_site[0])
    lik.close()
    for k in (0, BAD[0] + 1, BAD[1] + 1, n - 1):
        at = kt.Case("%s_draw%d" % (case.name, k), case.masks, case.weights, case.peel, case.rooted, blens[k],
                     case.args["rates"], case.args["freqs"], case.args["rs"], case.args["ps"])
        err = kt.compare(at, rows[k], site[k], at.truth_row())
        print(at.name, {q: "%.2e" % v for q, v in err.items()})
        assert not kt.bars(err), (k, err)


def test_item_loop_of_the_mixture():
    # the same 2560 items as M = 2, C = 2; the class posteriors too
    case = mt.random_mix("K4_S3_P145_M2_C2_rooted", 3, 4, 145, 2, 2, True, 61)
    n = 64
    blens, params = _item_loop_draws(case, n)
    lik = _mix_device(case, max_draws=n)
    _assert_items_loop(lik.info(), n)
    rows, site, post = lik.evaluate_rows(blens, params, site_ll=True, class_post=True)
    for k in range(n):
        if k in BAD:
            assert rows[k, 0] == -np.inf and not rows[k, 1:].any() and np.all(site[k] == -np.inf) and not post[k].any()
            continue
        one = lik.evaluate_rows(blens[k:k + 1], params[k:k + 1], site_ll=True, class_post=True)
        for got, want in zip((rows[k], site[k], post[k]), one):
            np.testing.assert_array_equal(got, want[0])
    lik.close()
    for k in (0, BAD[0] + 1, BAD[1] + 1, n - 1):
        at = mt.MixCase("%s_draw%d" % (case.name, k), case.masks, case.weights, case.peel, case.rooted, blens[k],
                        [(case.params[m * 10:m * 10 + 6], case.params[m * 10 + 6:m * 10 + 10]) for m in range(2)],
                        case.rs, case.ps)
        np.testing.assert_array_equal(at.params, case.params)
        err = mt.compare(at, rows[k], site[k], post[k], at.truth_row())
        print(at.name, {q: "%.2e" % v for q, v in err.items()})
        assert not mt.bars(err), (k, err)


def test_draw_and_component_loops():
    # K = 5, M = 8, C = 2: more draws than compute units, so the site kernel's draw loop turns; the eigen and combine
    # kernels' (draw, component) loops turn 8 times as often
    case = MIX_EDGES[0]
    wide = _mix_device(case, max_draws=1024)
    info = wide.info()
    cus = info["draw_workgroups"]  # min(compute units, max_draws)
    n = cus + cus // 2 + 3
    assert n <= 1024, "the device has %d compute units or more: no loop would turn" % cus
    assert info["chunk_draws"] >= n  # one chunk: the site kernel's grid is cus workgroups for n draws
    blens = case.blens[None] * _scaled(n)[:, None]
    params = np.repeat(case.params[None], n, 0)
    got = wide.evaluate_rows(blens, params, site_ll=True, class_post=True)
    wide.close()
    narrow = _mix_device(case, max_draws=8)  # calls of 8 draws: 8 draws, 64 pairs, 256 items, no second turn
    ninfo = narrow.info()
    assert ninfo["draw_workgroups"] == 8 and ninfo["workgroups"] == 8 * ninfo["items_per_draw"] and cus >= 64
    want = narrow.evaluate_rows(blens, params, site_ll=True, class_post=True)
    narrow.close()
    assert np.isfinite(got[0]).all()
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    for k in (0, cus, n - 1):
        at = mt.MixCase("%s_draw%d" % (case.name, k), case.masks, case.weights, case.peel, case.rooted, blens[k],
                        [(case.params[m * 15:m * 15 + 10], case.params[m * 15 + 10:m * 15 + 15]) for m in range(8)],
                        case.rs, case.ps)
        np.testing.assert_array_equal(at.params, case.params)
        err = mt.compare(at, got[0][k], got[1][k], got[2][k], at.truth_row())
        print(at.name, {q: "%.2e" % v for q, v in err.items()})
        assert not mt.bars(err), (k, err)


def test_zero_weight_column_of_positive_likelihood():
    case = tm.zero_weight_case()
    lik = _mix_device(case, max_draws=1)
    tm.check_zero_weight_column(lik, case)
    lik.close()


def test_zero_weight_column_of_zero_likelihood():
    full, live = tm.dead_column_cases()
    lik = _mix_device(full, max_draws=1)
    tm.check_dead_zero_weight_column(lik, full, live)
    lik.close()
    one = DeviceKStateLikelihood(full.masks, full.weights, full.peel, False, 2, 1, max_draws=1)
    params = np.concatenate([[1.0], [0.5, 0.5], [1.0], [1.0]])
    rows, site = one.evaluate_rows(np.zeros((1, 3)), params[None], site_ll=True)
    one.close()
    assert np.isfinite(rows).all() and site[0, 0] == -np.inf
    assert abs(rows[0, 0] - 2.0 * np.log(0.5)) <= 1e-15 and abs(site[0, 1] - np.log(0.5)) <= 1e-15  # L = pi_1
