"""CPU: the device-free class planner (phylostan_amd/csrc/class_plan.h).

* tests/class_plan_check.cpp, built by g++ alone with the address and
  undefined-behaviour sanitizers (no HIP include path: the header is
  device-free), run as a child process over generated trees and alignments;
* phy_plan_class reproduces, number for number, the class-plan facts live
  contexts of the commit before the planner was split out reported on an
  MI355X (tests/golden/class_plans.json, written by
  tests/golden/record_class_plans.py: contexts created and queried, never
  evaluated), and the table digests recorded beside them;
* every PHY_* class knob reaches the plan through the environment.
"""
import functools
import os
import subprocess

import pytest

from tests import class_plan_cases as cpc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RECORDED = ("classes", "levels", "root_classes", "stage", "staged", "tiles", "spans", "clade_levels", "clades",
            "clade_max", "chain_levels", "chain_lowest", "chain_top_classes", "level_pairs", "chunk_spans",
            "parent_order_levels")


def test_class_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "class_plan_check")
    # the sanitizer runtimes linked in: the program needs nothing preloaded
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "class_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "class_plan_check: " in run.stdout and " plans, 0 failures" in run.stdout


def _lib_built():
    from phylostan_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


needs_lib = pytest.mark.skipif(not _lib_built(), reason="HIP library not built (run __graft_entry__.build())")


@functools.lru_cache(maxsize=None)
def _case(name):
    return cpc.make_case(next(s for s in cpc.SPECS if cpc.spec_name(s) == name))


def plan(spec):
    from phylostan_amd.engine import plan_class
    case = _case(cpc.spec_name(spec))
    return plan_class(case.tipcodes, case.peel0, case.rooted, case.C, case.weights)


def set_knobs(monkeypatch, env):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


@needs_lib
@pytest.mark.parametrize("row", cpc.load_golden()["rows"], ids=cpc.row_id)
def test_plan_class_reproduces_recorded_contexts(row, monkeypatch):
    set_knobs(monkeypatch, row["env"])
    got = plan(row["case"])
    assert {k: got[k] for k in RECORDED} == row["facts"]
    assert got["ntiles"] == got["tiles"] and got["nclong"] == got["chunk_spans"]
    assert got["digests"] == row["digests"]  # (of the split-out planner itself: they hold its later edits)


FLU, REP, R9 = {"kind": "fluA"}, {"kind": "repetitive"}, next(s for s in cpc.SPECS if s.get("seed") == 9)
# (knob, value, case, the fact it moves, the golden setting that recorded it; None: stated here)
KNOBS = [
    ("PHY_CLADE", "0", FLU, "clade_levels", "clade0"),
    ("PHY_CHAIN", "0", FLU, "chain_levels", "nochain"),
    ("PHY_PAIR", "0", R9, "level_pairs", "nopair"),
    ("PHY_REVFIX", "0", REP, "chunk_spans", "norevfix"),
    ("PHY_STAGE_ORDER", "0", REP, "parent_order_levels", "stage0"),
    ("PHY_STAGE_ORDER", str(1 << 40), REP, "parent_order_levels", "stage2p40"),
    ("PHY_PAIR_MAX", "1", R9, "level_pairs", None),   # no upper level has a single class: no pair
    ("PHY_ROOT_WGS", "1", REP, "nrootch", None),      # one root workgroup, every round its own
    ("PHY_ROOT_CHAIN", "0", FLU, "root_chain", None),  # a launch preference: nothing else moves
]


@needs_lib
@pytest.mark.parametrize("knob,value,spec,fact,setting", KNOBS, ids=["%s=%s" % (k[0], k[1]) for k in KNOBS])
def test_plan_class_reads_each_knob(knob, value, spec, fact, setting, monkeypatch):
    rows = {r["setting"]: r for r in cpc.load_golden()["rows"] if r["case"] == spec}
    set_knobs(monkeypatch, {})
    base = plan(spec)
    assert {k: base[k] for k in RECORDED} == rows["default"]["facts"]
    set_knobs(monkeypatch, {knob: value})
    got = plan(spec)
    if setting is not None:
        assert got[fact] == rows[setting]["facts"][fact]
        # (the default threshold already puts no level of this case in parent order: against every level)
        other = rows["stage0"]["facts"] if setting == "stage2p40" else base
        assert got[fact] != other[fact], "the case does not show this knob"
    elif knob == "PHY_PAIR_MAX":
        assert base["level_pairs"] > 0 and got["level_pairs"] == 0
    elif knob == "PHY_ROOT_WGS":
        assert base["nrootch"] > 1 and got["nrootch"] == 1 and got["rootr"] == (got["root_classes"] + 63) // 64
    else:
        assert base["root_chain"] == 1 and got == dict(base, root_chain=0)
