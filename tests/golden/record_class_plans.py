"""Writes tests/golden/class_plans.json: the class-plan facts live contexts report on an MI355X.

    PHYLO_HIP_AB=1 PHYLO_HIP_LIB=<libphylo_hip.so of commit f87a69b> \
        python tests/golden/record_class_plans.py facts f87a69b [OUT]
    python tests/golden/record_class_plans.py digests

`facts`: the committed rows were recorded once from the build of the commit
before the class planner was split out into csrc/class_plan.h (f87a69b), so
that tests/test_class_plan_cpu.py and tests/test_gpu_class_plans.py pin the
plan across the split; rerun it against that build only.  Contexts are
created, switched to the class sweep and queried (phy_class_info,
phy_class_clades, phy_class_chain, phy_class_fused), never evaluated.

`digests` (no device): adds phy_plan_class's per-table digests of the current
build to every row.  That build could not produce them; they were added from
the split-out planner once its rows had been compared bit for bit with that
build's on every case of the file, and are there to hold later edits of the
planner."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from tests import class_plan_cases as cpc  # noqa: E402


def set_knobs(env):
    for k in cpc.KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)


def record_facts(commit, out):
    import torch  # before the engine's runtime
    from phylostan_amd.engine import TreeLikelihood
    cu = int(torch.cuda.get_device_properties(0).multi_processor_count)
    rows = []
    for spec in cpc.SPECS:
        case = cpc.make_case(spec)
        for name, env in cpc.SETTINGS:
            set_knobs(env)
            eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                                 max_draws=1, device=0)
            eng.set_engine("class")  # the knobs are read here (and at phy_create for an automatic class plan)
            assert eng.engine() == "class"
            row = {"case": spec, "setting": name, "env": env, "facts": eng.class_info()}
            eng.close()
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(out, "w") as fp:
        json.dump({"recorded_from": "commit %s (the commit before the class planner was split out), contexts "
                                    "created, switched to the class sweep and queried on one MI355X, never "
                                    "evaluated" % commit,
                   "commit": commit, "cu_count": cu, "rows": rows}, fp, indent=1)
    print("recorded %d rows, cu_count %d" % (len(rows), cu))


def add_digests(path):
    from phylostan_amd.engine import plan_class
    g = cpc.load_golden()
    g["digests"] = ("FNV-1a of every uploaded table (phy_plan_class), added from the split-out planner "
                    "(csrc/class_plan.h) after its output rows matched commit %s's bit for bit on every case here: "
                    "they hold later edits of the planner, they were not produced by that commit" % g["commit"])
    for row in g["rows"]:
        case = cpc.make_case(row["case"])
        set_knobs(row["env"])
        row["digests"] = plan_class(case.tipcodes, case.peel0, case.rooted, case.C, case.weights)["digests"]
    with open(path, "w") as fp:
        json.dump(g, fp, indent=1)
    print("digests added to %d rows" % len(g["rows"]))


if __name__ == "__main__":
    if sys.argv[1] == "facts":
        record_facts(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else cpc.GOLDEN)
    else:
        add_digests(cpc.GOLDEN)
