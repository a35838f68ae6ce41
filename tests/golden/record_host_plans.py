"""Writes tests/golden/host_plans.json: what live contexts report on an MI355X.

    PHYLO_HIP_AB=1 PHYLO_HIP_LIB=<libphylo_hip.so of commit 445dfa1> python tests/golden/record_host_plans.py [OUT]

The committed file was recorded once from the build of the commit before the
host planner was split out (445dfa1), so that tests/test_plan_host.py and
tests/test_gpu_host_plans.py pin the plan across the split; rerun it against
that build only.  Contexts are created and queried, never evaluated.  Getters
the recorded build did not have (resident workgroups, the latency plan) are
not in the file."""
import json
import os
import sys

import torch  # before the engine's runtime

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from phylostan_amd.engine import TreeLikelihood  # noqa: E402
from tests import cases  # noqa: E402

CU = int(torch.cuda.get_device_properties(0).multi_processor_count)

SETTINGS = [
    ("auto", {}),
    ("cols1", {"cols": 1}),
    ("cols2", {"cols": 2}),
    ("lds40000", {"lds_budget": 40000}),
    ("deep1", {"deep": 1}),
    ("deep2", {"deep": 2}),
    ("norecompute", {"recompute": 0}),
]
BUDGETS = [("cols2_lds%d" % b, {"cols": 2, "lds_budget": b}) for b in (60000, 80000, 100000)]

SPECS = []
for kind in ("fluA", "HCV", "DS1"):
    for md in (1, 4, 100, 8192):
        SPECS.append(({"kind": kind}, md, SETTINGS))
SPECS.append(({"kind": "random", "seed": 44, "S": 128, "P": 300, "C": 4}, 32, SETTINGS + BUDGETS))
SPECS.append(({"kind": "random", "seed": 35, "S": 9, "P": 100, "C": 8}, 32, SETTINGS))
SPECS.append(({"kind": "random", "seed": 7, "S": 12, "P": 130, "C": 16}, 32, SETTINGS))


def make_case(spec):
    if spec["kind"] == "fluA":
        return cases.fluA_case()
    if spec["kind"] == "HCV":
        return cases.hcv_case()
    if spec["kind"] == "DS1":
        return cases.ds1_case()
    return cases.random_case(spec["seed"], S=spec["S"], P=spec["P"], C=spec["C"])


rows = []
for spec, md, settings in SPECS:
    case = make_case(spec)
    for name, st in settings:
        eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                             max_draws=md, device=0)
        row = {"case": spec, "max_draws": md, "setting": name, "tuning": st}
        try:
            if "cols" in st or "lds_budget" in st:
                eng.set_tuning(0, st.get("cols", 0), st.get("lds_budget", 0))
            if "deep" in st:
                eng.set_deep_stack(st["deep"])
            if "recompute" in st:
                eng.set_recompute(bool(st["recompute"]))
            row["program_info"] = eng.program_info()
            row["lds_plan"] = eng.lds_plan()
            row["quad_plan"] = eng.quad_plan()
            cc = eng.clade_compression()
            row["clade_compression"] = cc
            row["engine"] = eng.engine()
        except Exception as e:  # noqa: BLE001
            row["error"] = str(e)
        eng.close()
        rows.append(row)
        print(json.dumps(row), flush=True)

out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "host_plans.json")
with open(out, "w") as fp:
    json.dump({"recorded_from": "commit 445dfa1 (the commit before the planner was split out), contexts created "
                                "and queried on one MI355X", "cu_count": CU, "rows": rows}, fp, indent=1)
print("recorded %d rows, cu_count %d" % (len(rows), CU))
