"""GPU: live contexts report the plans recorded in tests/golden/host_plans.json
(fluA, HCV and DS1 at max_draws 1, 4, 100 and 8192 under every recorded
setting; contexts are created and queried, nothing is evaluated).  A row is
skipped on a device whose compute-unit count differs from the recorded one:
the automatic plans depend on it."""
import pytest

from tests.test_plan_host import golden_rows, make_case, reported, row_id

pytestmark = pytest.mark.gpu


def _cu_count():
    import torch
    return int(torch.cuda.get_device_properties(0).multi_processor_count)


@pytest.mark.parametrize("row", golden_rows(("fluA", "HCV", "DS1"))[1], ids=row_id)
def test_live_context_reports_recorded_plan(row):
    from phylostan_amd.engine import TreeLikelihood
    cu, _ = golden_rows()
    if _cu_count() != cu:
        pytest.skip("recorded on a device of %d compute units" % cu)
    case = make_case(row["case"])
    st = row["tuning"]
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                         max_draws=row["max_draws"], device=0)
    try:
        if "cols" in st or "lds_budget" in st:
            eng.set_tuning(0, st.get("cols", 0), st.get("lds_budget", 0))
        if "deep" in st:
            eng.set_deep_stack(st["deep"])
        if "recompute" in st:
            eng.set_recompute(bool(st["recompute"]))
        got = reported(eng.program_info(), eng.lds_plan(), eng.quad_plan(), eng.clade_compression())
        assert got == reported(row["program_info"], row["lds_plan"], row["quad_plan"], row["clade_compression"])
        assert eng.engine() == row["engine"]
    finally:
        eng.close()
