"""GPU: the forest and the partitioned engine on the shared host path of
csrc/row_engine.inc, and the sequence-summary engine on its helpers, give bit
for bit the rows an MI355X gave at the commit before the move
(tests/golden/row_engine_rows_parent.npz, written there by
tests/golden/record_row_engine_rows.py): every form of the two exact suites
-- both K = 1 budgets, K = 2, both deep-stack placements, the finalize and the
chain rule in the sweep, in finalize_kernel and as a separate qgrad_kernel --
on the suites' own edge calls (S = 12, P = 130), HKY, rooted."""
import numpy as np
import pytest

from tests.golden import record_row_engine_rows as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return rec.load()


def test_the_fixture_holds_every_case(parent):
    want = {"%s/%s/%s" % (engine, form, k) for engine, form in rec.CASES
            for k in {"forest": ("rows", "site"), "part": ("out", "rows", "site"),
                      "seqsum": ("rows", "ll", "total", "nfin")}[engine]}
    assert set(parent) == want - set(rec.LEFT_OUT)


@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: "%s-%s" % c)
def test_rows_are_the_parents_bits(case, parent, monkeypatch):
    engine, form = case
    got = rec.compute(engine, form, monkeypatch)
    keys = [k for k in got if "%s/%s/%s" % (engine, form, k) not in rec.LEFT_OUT]
    assert keys
    for k in keys:
        np.testing.assert_array_equal(np.asarray(got[k], np.float64), parent["%s/%s/%s" % (engine, form, k)],
                                      err_msg="%s/%s/%s" % (engine, form, k))
