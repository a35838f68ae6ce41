"""The cases and knob settings of tests/golden/class_plans.json, shared by its
recorder (tests/golden/record_class_plans.py) and the tests that read it
(tests/test_class_plan_cpu.py, tests/test_gpu_class_plans.py)."""
import json
import os

import numpy as np

from tests import cases

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "class_plans.json")

# fluA, HCV, DS1 unrooted; seeds 2, 4, 5, 7, 9 of test_class_sweep_random_trees; the repetitive alignment
SPECS = [
    {"kind": "fluA"}, {"kind": "HCV"}, {"kind": "DS1"},
    {"kind": "random", "seed": 2, "S": 12, "P": 63, "C": 3, "model": "GTR", "rooted": True, "caterpillar": False},
    {"kind": "random", "seed": 4, "S": 17, "P": 257, "C": 5, "model": "GTR", "rooted": False, "caterpillar": False},
    {"kind": "random", "seed": 5, "S": 40, "P": 200, "C": 2, "model": "GTR", "rooted": True, "caterpillar": True},
    {"kind": "random", "seed": 7, "S": 128, "P": 3000, "C": 4, "model": "GTR", "rooted": True, "caterpillar": False},
    {"kind": "random", "seed": 9, "S": 300, "P": 500, "C": 4, "model": "GTR", "rooted": True, "caterpillar": False},
    {"kind": "repetitive"},
]

# the default knobs, then every setting tests/test_gpu_class.py uses
SETTINGS = [
    ("default", {}),
    ("clade0", {"PHY_CLADE": "0"}),
    ("clade3_nochain", {"PHY_CLADE": "3", "PHY_CHAIN": "0"}),
    ("nochain", {"PHY_CHAIN": "0"}),
    ("nopair", {"PHY_PAIR": "0"}),
    ("norevfix", {"PHY_REVFIX": "0"}),
    ("stage0", {"PHY_STAGE_ORDER": "0"}),
    ("stage2p40", {"PHY_STAGE_ORDER": str(1 << 40)}),
]

KNOBS = ("PHY_CLADE", "PHY_CHAIN", "PHY_ROOT_WGS", "PHY_STAGE_ORDER", "PHY_PAIR", "PHY_PAIR_MAX", "PHY_REVFIX",
         "PHY_ROOT_CHAIN")


def make_case(spec):
    if spec["kind"] == "random":
        return cases.random_case(spec["seed"], S=spec["S"], P=spec["P"], C=spec["C"], model=spec["model"],
                                 rooted=spec["rooted"], caterpillar=spec["caterpillar"])
    if spec["kind"] == "repetitive":  # test_class_sweep_repetitive_alignment's
        rng = np.random.default_rng(70)
        base = cases.random_case(70, S=48, P=5000, C=4, model="GTR")
        codes = np.where(rng.random((48, 5000)) < 0.9, 1, rng.choice([1, 2, 4, 8, 15], size=(48, 5000)))
        return cases.Case("rep", codes.astype(np.uint8), base.weights, base.peel0, True, "GTR", 4, base.blens,
                          base.freqs, base.rates, base.rs, base.ps)
    return {"fluA": cases.fluA_case, "HCV": cases.hcv_case, "DS1": cases.ds1_case}[spec["kind"]]()


def spec_name(spec):
    return spec["kind"] if spec["kind"] != "random" else "rand%d" % spec["seed"]


def load_golden():
    with open(GOLDEN) as fp:
        return json.load(fp)


def row_id(row):
    return "%s-%s" % (spec_name(row["case"]), row["setting"])
