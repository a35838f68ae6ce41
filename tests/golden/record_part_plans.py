"""Writes tests/golden/part_plans.json: the partitioned engine's plan
(phy_part_plan: no device, 256 compute units, no PHY_* preference set) of
every case the GPU tests of tests/test_part_gpu.py create a context for.

    python tests/golden/record_part_plans.py [OUT]

The rows hold later edits of csrc/part_plan.h and of sweep_plan.h's plan_lds /
choose_launch: rerun only when a plan is meant to change."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phylostan_amd import partition as pt  # noqa: E402
from tests import part_cases as pc  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "part_plans.json")
CU_COUNT = 256


def _row(name, c, max_draws):
    plan = c.plan(max_draws, cu_count=CU_COUNT)
    return {"case": name, "widths": list(c.widths), "S": c.S, "C": c.C, "model": c.model, "rooted": bool(c.rooted),
            "max_draws": max_draws, "facts": {k: plan[k] for k in pt.PLAN_FACTS}, "block_ranges": plan["blocks"],
            "first_columns": [int((plan["col_part"] == k).argmax()) for k in range(c.K)],
            "live_columns": int((plan["col_part"] >= 0).sum())}


def cases():
    """[(name, case, max_draws)]"""
    out = [(pc.SHAPE_IDS[i], pc.shape_case(i), 9) for i in range(len(pc.SHAPES))]
    out += [(pc.SHAPE_IDS[3], pc.shape_case(3), m) for m in (1, 64, 300)]
    out.append(("ambiguity", pc.ambiguity_case(), 9))
    return out


def record():
    saved = {k: os.environ.pop(k) for k in [k for k in os.environ if k.startswith("PHY_")]}
    try:
        rows = [_row(*c) for c in cases()]
    finally:
        os.environ.update(saved)
    return {"cu_count": CU_COUNT, "rows": rows}


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as fp:
        json.dump(record(), fp, indent=1)
        fp.write("\n")
    print("recorded %d rows" % len(record()["rows"]))
