"""GPU: live contexts report the class plan that tests/golden/class_plans.json
recorded from the commit before the planner was split out into
csrc/class_plan.h, and the plan phy_plan_class makes of the same inputs
without a device.  Contexts are created and queried, never evaluated."""
import pytest

from tests import class_plan_cases as cpc
from tests.test_class_plan_cpu import RECORDED, plan, set_knobs
from tests.test_gpu_parity import _engine

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("spec", cpc.SPECS, ids=cpc.spec_name)
def test_live_class_plan_equals_recorded_and_planned(spec, monkeypatch):
    rows = [r for r in cpc.load_golden()["rows"] if r["case"] == spec]
    assert [r["setting"] for r in rows] == [s[0] for s in cpc.SETTINGS]
    case = cpc.make_case(spec)
    for row in rows:
        set_knobs(monkeypatch, row["env"])
        eng = _engine(case)
        eng.set_engine("class")
        live = eng.class_info()
        eng.close()
        assert live == row["facts"], row["setting"]
        got = plan(spec)
        assert {k: got[k] for k in RECORDED} == live, row["setting"]
