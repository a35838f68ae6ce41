"""GPU: the two quad sweeps (csrc/quad_engine.inc), with each shared phase and
each LDS layout stated once, give bit for bit the rows an MI355X gave at the
commit before (tests/golden/quad_rows_parent.npz, written there by
tests/golden/record_quad_rows.py, which lists the cases, forms and calls):
qsweep_kernel<256> and <1024>, qmw_kernel at 4 and at <= 3 waves per category,
built and copied records, the store and the atomic-add path of the dL/dP slot,
the matrix-less root step, C > 8 and JC69."""
import numpy as np
import pytest

from tests.golden import record_quad_rows as rec

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def parent():
    return rec.load()


def _arrays(name):
    out = []
    for call in rec.CALLS[name]:
        ids = {"n1": [0], "n32": [0, rec.NDRAWS - 1], "n4dev": [rec.DEV_DRAWS[0], rec.DEV_DRAWS[-1]]}[call]
        out += ["%s/compact" % call] + ["%s/full_d%d" % (call, k) for k in ids] + (["n1/site"] if call == "n1" else [])
    return out


def test_the_fixture_holds_every_case(parent):
    want = {rec.key(name, form, k) for name, form in rec.CASES for k in _arrays(name)}
    assert set(rec.LEFT_OUT) <= want
    assert set(parent) == want - set(rec.LEFT_OUT)


@pytest.mark.parametrize("case", rec.CASES, ids=lambda c: "%s-%s" % c)
def test_rows_are_the_parents_bits(case, parent, monkeypatch):
    name, form = case
    got = rec.compute(name, form, monkeypatch)  # asserts the form too (record_quad_rows.assert_form)
    assert sorted(got) == sorted(_arrays(name))
    keys = [k for k in got if rec.key(name, form, k) not in rec.LEFT_OUT]
    assert keys
    for k in keys:
        np.testing.assert_array_equal(got[k], parent[rec.key(name, form, k)], err_msg=rec.key(name, form, k))
