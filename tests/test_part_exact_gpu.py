"""GPU: the partitioned engine against the complex-step reference (oracle/
complex_step.py) -- not against the C oracle, which runs the device's Jacobi
eigensolver and divided-difference tie rule operation for operation -- on the
edge draws of tests/part_exact_cases.py: spectral ties, near ties,
ill-conditioned models, extreme and zero site rates on the three partitions
(64, 65 and 1 columns) of a draw, short, zero and saturated branches and
mu = (1e-4, 1, 200) per draw, all draws of a context in ONE call.

The engine launches only the six ``sweep_kernel<., ., ., false, false, false,
true>`` instantiations of ``row_kernel_for<false, true>``, one workgroup per (draw,
partition) row walking its partition's blocks; every form below is named by
its ``partition.plan_partitions`` facts, which the live context's ``info()``
must equal, before it evaluates (the table of tests/test_part_exact_cpu.py):

  cols2                      <512,2,true>    the default of 600 draws
  cols2-deep-global          <512,2,false>   PHY_DEEP=2: the deep stack in global memory
  no-deep-entries            <512,2,false>   the caterpillar: an empty deep stack
  cols1-latency              <512,1,true>    9 draws: one column per lane, the 65-column partition in two blocks
  cols1-latency-deep-global  <512,1,false>   PHY_DEEP=2 at 9 draws
  C10                        <1024,1,true>   ten categories (HKY, its own truth)
  C10-deep-global            <1024,1,false>  PHY_DEEP=2 at ten categories
  cols1-split-stack          <1024,1,false>  PHY_COLS=1: one deep entry in LDS, one in global memory
  lds16k                     <512,2,false>   PHY_LDS_BUDGET=16384: the matrix records staged in three chunks
  lds16k-latency             <512,1,false>   the same at 9 draws, one column per lane
  norecompute                <512,2,true>    PHY_RECOMPUTE=0
  fin0                       PHY_FIN=0: the chain rule in finalize_kernel
  qgrad-after-finalize       PHY_FIN=0 PHY_QFUSE=0: qgrad_kernel after finalize_kernel
  qgrad-after-sweep          PHY_QFUSE=0: qgrad_kernel after the sweep's own finalize

Bounds as tests/test_gpu_exact_gradients.py: log L and site_ll 1e-10,
gradients 1e-9, Q-parameter gradients 1e-8 of each array's largest entry,
d/dmu_k 1e-9 of sum_b |t_b g_kb|; the rows with branches of 1e-4 or less (the
two short draws, the mu = 1e-4 partition) at max(bar, 10 x the numpy oracle's
own error at that row); a draw's bound is the largest of its partitions'.
"""
import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

from phylostan_amd import partition as pt
from tests import exact_cases as ec, part_exact_cases as px, report
from tests.test_gpu_parity import RTOL_G, RTOL_LL
from tests.test_part_exact_cpu import FORMS, KERNELS, assert_form, models_of, set_form

pytestmark = pytest.mark.gpu

assert (ec.BAR_LL, ec.BAR_G) == (RTOL_LL, RTOL_G)

UNROOTED_FORMS = ("cols2", "cols1-latency", "C10", "cols2-deep-global", "lds16k")
CONTEXTS = [(form, model, True) for form in FORMS for model in models_of(form)] + \
           [(form, model, False) for form in UNROOTED_FORMS for model in models_of(form)]


def _ctx_id(c):
    return "%s-%s-%s" % (c[0], c[1], "rooted" if c[2] else "unrooted")


def make_engine(form, model, rooted, monkeypatch):
    """A partitioned context that runs ``form``, with the evidence that it does."""
    max_draws, C, tree, facts = set_form(form, monkeypatch)
    e = px.edge_part(model, rooted, C, tree)
    eng = e.engine(max_draws)
    info = eng.info()
    assert set(info) == set(pt.PLAN_FACTS)
    plan = assert_form(e, form, max_draws, facts, info=info)
    assert (eng.K, eng.B, eng.rowlen, eng.outlen) == (e.K, e.B, e.rowlen, e.outlen)
    return e, eng, KERNELS[(plan["cols"], plan["latency"], plan["deep_all_in_lds"])]


def other_legs(e, eng, out, rows, site):
    """The contracts 2 to 5 of tests/test_part_gpu.py on the edge draws, in the same context."""
    bl, mu, mv, n = e.blens, e.mu, e.model_vecs, e.n
    for d in range(n):                                                   # 2: the fold, bit for bit
        np.testing.assert_array_equal(out[d], pt.partition_combine_host(rows[d], bl[d], mu[d]),
                                      err_msg="the fold of draw %d" % d)
    for k in range(e.K):                                                 # 3: (t, mu) against (mu_k t, 1)
        _, r1 = eng.evaluate_rows(mu[:, k:k + 1] * bl, np.ones_like(mu), mv, part_rows=True)
        np.testing.assert_array_equal(r1[:, k], rows[:, k], err_msg="partition %d at (mu_k t, 1)" % k)
    o2, r2, s2 = eng.evaluate_rows(bl, mu, mv, part_rows=True, site_ll=True)  # 4: a repeated call
    np.testing.assert_array_equal(o2, out)
    np.testing.assert_array_equal(r2, rows)
    np.testing.assert_array_equal(s2, site)
    bad = mv.copy()                                                      # 5: a rejected partition
    d_bad, k_bad = n // 2, e.K - 1
    bad[d_bad, k_bad, 0] = -bad[d_bad, k_bad, 0]
    o3, r3 = eng.evaluate_rows(bl, mu, bad, part_rows=True)
    assert o3[d_bad, 0] == -np.inf and not o3[d_bad, 1:].any()
    assert r3[d_bad, k_bad, 0] == -np.inf and not r3[d_bad, k_bad, 1:].any()
    keep = np.arange(n) != d_bad
    np.testing.assert_array_equal(o3[keep], out[keep])
    np.testing.assert_array_equal(r3[keep], rows[keep])
    np.testing.assert_array_equal(r3[d_bad, :k_bad], rows[d_bad, :k_bad])


@pytest.mark.parametrize("ctx", CONTEXTS, ids=_ctx_id)
def test_edge_draws_in_one_call(ctx, monkeypatch):
    form, model, rooted = ctx
    e, eng, kernel = make_engine(form, model, rooted, monkeypatch)
    out, rows, site = eng.evaluate_rows(e.blens, e.mu, e.model_vecs, part_rows=True, site_ll=True)
    failures = []
    row_errs, draw_errs = px.check_call(e, out, rows, site, failures, what=form)
    tag = "part-exact[%-25s %-14s %s %s]" % (form, kernel, model, "rooted  " if rooted else "unrooted")
    near = px.largest(e, row_errs, (px.NEAR,))
    line = "%s worst error/bound %.2g (%s %s)" % (tag, *px.worst(e, row_errs, draw_errs))
    if near:
        line += "; near ties: drates %.1e dfreqs %.1e, any array %.1e" % (near["grad_rates"], near["grad_freqs"],
                                                                          max(near.values()))
    report.record(line)
    assert not failures, failures
    other_legs(e, eng, out, rows, site)
    eng.close()


@pytest.mark.parametrize("rooted", [True, False], ids=["rooted", "unrooted"])
@pytest.mark.parametrize("model", ["HKY", "GTR"])
@pytest.mark.parametrize("form", ["cols2", "cols1-latency"])
def test_edge_rows_are_their_own(form, model, rooted, monkeypatch):
    """The tie marks and the near window are a row's own, not its draw's: the
    call's rows (a near-tie partition between a generic and an exact-tie one
    in the opening HKY draw) are, bit for bit, the rows of one-draw calls and
    of the reversed and a permuted call."""
    e, eng, _ = make_engine(form, model, rooted, monkeypatch)
    if model == "HKY":
        assert [r.kind for r in e.rows[0]] == [px.GENERIC, px.NEAR, px.TIE]
    out, rows, site = eng.evaluate_rows(e.blens, e.mu, e.model_vecs, part_rows=True, site_ll=True)
    for d in range(e.n):
        o1, r1, s1 = eng.evaluate_rows(e.blens[d:d + 1], e.mu[d:d + 1], e.model_vecs[d:d + 1], part_rows=True,
                                       site_ll=True)
        np.testing.assert_array_equal(o1[0], out[d], err_msg="draw %d (%s) alone" % (d, e.draw_kinds[d]))
        np.testing.assert_array_equal(r1[0], rows[d], err_msg="draw %d (%s) alone" % (d, e.draw_kinds[d]))
        np.testing.assert_array_equal(s1[0], site[d], err_msg="draw %d (%s) alone" % (d, e.draw_kinds[d]))
    for perm in (np.arange(e.n)[::-1], np.random.default_rng(5).permutation(e.n)):
        o2, r2, s2 = eng.evaluate_rows(e.blens[perm], e.mu[perm], e.model_vecs[perm], part_rows=True, site_ll=True)
        np.testing.assert_array_equal(o2, out[perm])
        np.testing.assert_array_equal(r2, rows[perm])
        np.testing.assert_array_equal(s2, site[perm])
    eng.close()
