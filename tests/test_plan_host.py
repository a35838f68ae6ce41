"""CPU: the device-free planner (phylostan_amd/csrc/sweep_plan.h).

* tests/plan_host_check.cpp, built by g++ alone with the address and
  undefined-behaviour sanitizers (no HIP include path: the header is
  device-free), run as a child process over generated trees;
* phy_plan_sweep reproduces, number for number, what live contexts of the
  commit before the planner was split out reported on an MI355X
  (tests/golden/host_plans.json, written by tests/golden/record_host_plans.py:
  contexts created and queried, never evaluated);
* the launch choice, row by row against the documents that state it.
"""
import functools
import json
import os
import subprocess

import pytest

from tests import cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "host_plans.json")


def make_case(spec):
    if spec["kind"] == "random":
        return cases.random_case(spec["seed"], S=spec["S"], P=spec["P"], C=spec["C"])
    return {"fluA": cases.fluA_case, "HCV": cases.hcv_case, "DS1": cases.ds1_case}[spec["kind"]]()


def golden_rows(kinds=None):
    with open(GOLDEN) as fp:
        g = json.load(fp)
    rows = [r for r in g["rows"] if kinds is None or r["case"]["kind"] in kinds]
    return g["cu_count"], rows


def row_id(r):
    c = r["case"]
    name = c["kind"] if c["kind"] != "random" else "rand%d" % c["seed"]
    return "%s-%d-%s" % (name, r["max_draws"], r["setting"])


def reported(program_info, lds_plan, quad_plan, clade):
    """The recorded numbers of one context, in one flat dict."""
    out = {k: program_info[k] for k in ("nsteps", "nslots", "depth", "nblocks")}
    out.update(lds_plan)
    out.update({"quad_" + k: v for k, v in quad_plan.items()})
    out.update({"clade_" + k: v for k, v in clade.items() if k not in ("clade_list", "mode")})
    return out


def planned(plan):
    """The same numbers from engine.plan_sweep's dict."""
    out = {k: plan[k] for k in ("nsteps", "nslots", "depth", "nblocks", "n_chunks", "matrices_per_chunk", "lds_bytes",
                                "cols", "deep_lds_entries", "recomputed")}
    out.update(quad_waves=plan["quad_waves"], quad_span=plan["quad_span"], quad_slots=plan["quad_slots"])
    out.update({"clade_" + k: v for k, v in plan["clade"].items()})
    return out


def test_planner_under_host_sanitizers(tmp_path):
    exe = str(tmp_path / "plan_host_check")
    # the sanitizer runtimes linked in: the program needs nothing preloaded
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "plan_host_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    assert "0 failures" in run.stdout


def _lib_built():
    from phylostan_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


needs_lib = pytest.mark.skipif(not _lib_built(), reason="HIP library not built (run __graft_entry__.build())")


@functools.lru_cache(maxsize=None)
def _case(key):
    return make_case(dict(key))


def plan(spec, max_draws, n, cu=256, **tuning):
    from phylostan_amd.engine import plan_sweep
    case = _case(tuple(sorted(spec.items())))
    return plan_sweep(case.tipcodes, case.peel0, case.rooted, case.C, max_draws, cu, n, **tuning)


@needs_lib
@pytest.mark.parametrize("row", golden_rows()[1], ids=row_id)
def test_plan_sweep_reproduces_recorded_contexts(row, monkeypatch):
    from phylostan_amd import _lib
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    cu, _ = golden_rows()
    tuning = dict(row["tuning"])
    if "error" in row:  # the one refused setting: two columns per lane at C = 16
        with pytest.raises(_lib.PhyloHipError, match="two columns per lane need C <= 8"):
            plan(row["case"], row["max_draws"], 1, cu, **tuning)
        assert "two columns per lane need C <= 8" in row["error"]
        return
    got = plan(row["case"], row["max_draws"], 1, cu, **tuning)
    want = reported(row["program_info"], row["lds_plan"], row["quad_plan"], row["clade_compression"])
    assert planned(got) == want


FLU, DS1 = {"kind": "fluA"}, {"kind": "DS1"}
QUAD_MW = dict(path="quad_mw", g_direct=0, fin=0, qf=0)
# (case, max_draws, tuning, environment, n, expected launch facts, the sentence restated)
LAUNCHES = [
    (FLU, 8192, {}, {}, 1, QUAD_MW,
     "phylo_hip_diag.h phy_set_engine: 'a call of at most 32 draws takes its quad form'; phy_quad_plan: '2 up to "
     "16 / C: the multi-wave form'"),
    (FLU, 8192, {}, {}, 4, QUAD_MW, "as above"),
    (FLU, 8192, {}, {}, 32, QUAD_MW, "as above (32 is the last quad call size)"),
    (FLU, 8192, {}, {}, 33, dict(path="pattern", gx=2, g_direct=0, fin=0, qf=0, gsum_in=1),
     "phylo_hip_diag.h phy_set_clade_compression: 'A launch takes the compressed plan only when it is one workgroup "
     "per draw of the two-column sweep without rescaling; every other launch (... draws over several workgroups ...) "
     "runs what it ran without it'"),
    (FLU, 8192, {}, {}, 100, dict(path="pattern", gx=2, g_direct=0, fin=0, qf=0, gsum_in=1), "as above"),
    (FLU, 8192, {}, {}, 8192, dict(path="pattern_cc", gx=1, g_direct=1, fin=1, qf=1, gsum_in=0),
     "commit 445dfa1: 'A launch takes it only at one workgroup per draw, K = 2, no rescaling' (fluA, 8,192 draws); "
     "DESIGN.md 2: finalize and chain rule inside the sweep when one workgroup runs a draw"),
    (DS1, 8192, {}, {}, 8192, dict(path="pattern", gx=1, g_direct=1),
     "commit 445dfa1: 'DS1 unchanged (no clade kept)'"),
    (DS1, 8192, {}, {}, 100, dict(path="pattern"), "as above"),
    (FLU, 8192, {"rescaling": True}, {}, 4, dict(path="pattern"),
     "phylo_hip_diag.h phy_set_rescaling: 'calls of <= 32 draws take the column sweep instead of its quad form'"),
    (FLU, 8192, {"rescaling": True}, {}, 8192, dict(path="pattern", gx=1, g_direct=1),
     "phylo_hip_diag.h phy_set_clade_compression: '... without rescaling'"),
    (FLU, 8192, {"rescaling": True}, {}, 33, dict(path="pattern", gx=2), "as above"),
    (FLU, 8192, {"cols": 1}, {}, 4, dict(path="pattern"),
     "sweep_plan.h choose_launch: 'unless a column plan is set explicitly (phy_set_tuning(cols > 0))'"),
    (FLU, 8192, {"cols": 2}, {}, 4, dict(path="pattern"), "as above"),
    (FLU, 8192, {"clade_mode": 0}, {}, 8192, dict(path="pattern", gx=1, g_direct=1, fin=1, qf=1),
     "phylo_hip_diag.h phy_set_clade_compression: 'mode: 0 off'"),
    (FLU, 8192, {"clade_mode": 0}, {}, 100, dict(path="pattern"), "as above"),
    (FLU, 8192, {}, {"PHY_QMW": "0"}, 4, dict(path="quad", g_direct=0),
     "phylo_hip_diag.h phy_quad_plan: 'PHY_QMW=0 at phy_create keeps the one-wave form'"),
    (FLU, 8192, {}, {"PHY_QUAD": "0"}, 4, dict(path="pattern"),
     "phylo_hip_diag.h phy_set_engine: 'PHY_QUAD=0 at phy_create keeps the column sweep'"),
]


@needs_lib
@pytest.mark.parametrize("spec,max_draws,tuning,env,n,expect,cites", LAUNCHES,
                         ids=["%s-%s%s-n%d" % (r[0]["kind"], "-".join("%s%s" % kv for kv in r[2].items()) or "auto",
                                               "".join("-%s%s" % kv for kv in r[3].items()), r[4]) for r in LAUNCHES])
def test_launch_choice(spec, max_draws, tuning, env, n, expect, cites, monkeypatch):
    for k in [k for k in os.environ if k.startswith("PHY_")]:
        monkeypatch.delenv(k)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    got = plan(spec, max_draws, n, 256, **tuning)["launch"]
    assert {k: got[k] for k in expect} == expect, cites
