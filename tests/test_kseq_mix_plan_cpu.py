"""CPU: the planner and the boundary of the K-state mixture engine.

* tests/kseq_mix_plan_check.cpp, built by g++ alone with the address and
  undefined-behaviour sanitizers (the header is device-free), run as a child
  process: every offset the kernels form with the component index against the
  sizes the plan gives, the plan at M = 1 against ``kseq_plan``'s, the refusals;
* with the library built, on a machine without a device: the refusals of
  ``phy_kseq_mix_create`` come back as PHY_EINVAL with their own message,
  ``phy_kseq_mix_eval(NULL, ...)`` is refused, and ``plan_kseq_mix`` gives the
  numbers the check program prints;
* ``_lib.KSEQ_MIX_SIGNATURES`` against the prototypes of the header;
* ``DeviceKStateMixLikelihood``'s own checks, made before the library is touched;
* the committed resource table: no scratch on any of the five kernels.
"""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import _lib, kseq
from tests import kseq_mix_truth as mt
from tests import kseq_truth as kt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHY_EINVAL = 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kseq_mix_plan") / "kseq_mix_plan_check")
    # the sanitizer runtimes linked in: the program needs nothing preloaded
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "kseq_mix_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout


def test_planner_under_host_sanitizers(check_output):
    assert "0 failures" in check_output and "FAIL" not in check_output


needs_lib = pytest.mark.skipif(not os.path.exists(_lib.LIB_PATH),
                               reason="HIP library not built (run __graft_entry__.build())")


def _flu_codon_shape():
    rng = np.random.default_rng(3)
    S, P = 69, 242
    return kt.random_masks(S, P, 61, rng), np.ones(P), kt.rooted_peel(S, rng)


@needs_lib
def test_plan_kseq_mix_agrees_with_the_check_program(check_output):
    line = [ln for ln in check_output.splitlines() if ln.startswith("fluA_codon_mix ")]
    assert len(line) == 1
    want = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line[0])}
    masks, w, peel = _flu_codon_shape()
    got = kseq.plan_kseq_mix(masks, w, peel, True, 61, 3, 4, max_draws=32, cu_count=256)
    assert got == want
    # fluA codon at M = 3, C = 4: 192 items and about 650 MB a draw: one draw in flight
    assert got["items_per_draw"] == 192 and got["chunk_draws"] == 1 and 600e6 < got["workspace_bytes"] < 700e6
    # M = 1 is plan_kseq
    assert kseq.plan_kseq_mix(masks, w, peel, True, 61, 1, 4, max_draws=32) == kseq.plan_kseq(masks, w, peel, True, 61,
                                                                                             4, max_draws=32)


def _create(S, P, K, M, C, rooted, masks, w, peel, max_draws=1):
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.phy_kseq_mix_create(S, P, K, M, C, rooted, ptr(masks), ptr(w), ptr(peel), max_draws, 0, ctypes.byref(ctx))
    msg = lib.phy_last_error().decode()
    if rc == 0:
        lib.phy_kseq_mix_destroy(ctx)
    return rc, msg


@needs_lib
def test_create_refusals_come_before_the_device():
    case = mt.small_cases()[2]  # K = 17, S = 7, P = 17, M = 3, C = 1, unrooted
    S, P, K, M, C = case.S, case.P, case.K, case.M, case.C
    m, w, peel = case.masks, case.weights, np.ascontiguousarray(case.peel, np.int32)
    bad_mask = m.copy()
    bad_mask[2, 3] = 0
    rows = [
        ((S, P, K, 0, C, 0, m, w, peel), "phy_kseq_mix_create: M = 0 components, supported 1..8"),
        ((S, P, K, 9, C, 0, m, w, peel), "M = 9 components, supported 1..8"),
        ((S, P, K, M, 0, 0, m, w, peel), "C = 0 categories, supported 1..16"),
        ((S, P, K, M, 6, 0, m, w, peel), "M * C = 18 component-categories, supported up to 16"),
        ((S, P, 65, M, C, 0, m, w, peel), "K = 65 states, supported 2..64"),
        ((2, P, K, M, C, 0, m, w, peel), "S = 2"),
        ((S, P, K, M, C, 0, m, w, peel, 0), "max_draws must be >= 1"),
        ((S, P, K, M, C, 0, None, w, peel), "tipmasks is NULL"),
        ((S, P, K, M, C, 0, bad_mask, w, peel), "tipmasks[2][3] has no bit set"),
    ]
    for args, needle in rows:
        rc, msg = _create(*args)
        assert rc == PHY_EINVAL, (needle, rc, msg)
        assert needle in msg and "device" not in msg, (needle, msg)
    # a shape whose single draw passes the budget: refused with a message, through the Python planner too
    rng = np.random.default_rng(1)
    big = kt.random_masks(2000, 1300, 64, rng)
    with pytest.raises(_lib.PhyloHipError, match="exceeds the budget"):
        kseq.plan_kseq_mix(big, np.ones(1300), kt.caterpillar_peel(2000), False, 64, 4, 4)


@needs_lib
def test_eval_refuses_a_null_context():
    lib = _lib.load()
    x = np.zeros(8)
    rc = lib.phy_kseq_mix_eval(None, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data, None, None)
    assert rc == PHY_EINVAL and "phy_kseq_mix_eval: NULL ctx" in lib.phy_last_error().decode()
    assert lib.phy_kseq_mix_row_len(None) == -1 and lib.phy_kseq_mix_num_branches(None) == -1
    assert lib.phy_kseq_mix_info(None, 0, None, None) == PHY_EINVAL


def test_signatures_match_the_header():
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "phylo_hip_kseq_mix.h")).read(), flags=re.S)
    protos = {}
    for name, args in re.findall(r"\bint\s+(phy_kseq_mix_\w+)\s*\(([^)]*)\)\s*;", text):
        protos[name] = ["ptr" if "*" in a else "int" for a in args.split(",")]
    assert sorted(protos) == ["phy_kseq_mix_create", "phy_kseq_mix_destroy", "phy_kseq_mix_eval", "phy_kseq_mix_info",
                              "phy_kseq_mix_num_branches", "phy_kseq_mix_plan", "phy_kseq_mix_row_len"]
    assert sorted(protos) == sorted(_lib.KSEQ_MIX_SIGNATURES)
    for name, kinds in protos.items():
        res, args = _lib.KSEQ_MIX_SIGNATURES[name]
        assert res is ctypes.c_int
        assert ["int" if a is ctypes.c_int else "ptr" for a in args] == kinds, name
    # phylo_hip_kseq.h brings the header in and declares nothing of it itself
    main = open(os.path.join(ROOT, "include", "phylo_hip_kseq.h")).read()
    assert '#include "phylo_hip_kseq_mix.h"' in main and "phy_kseq_mix_create(" not in main


def test_wrapper_validates_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    case = mt.small_cases()[1]
    ok = (case.masks, case.weights, case.peel, case.rooted, case.K, case.M, case.C)
    with pytest.raises(ValueError, match="tipmasks must be \\[S, P\\]"):
        kseq.DeviceKStateMixLikelihood(case.masks[0], *ok[1:])
    with pytest.raises(ValueError, match="weights must be"):
        kseq.DeviceKStateMixLikelihood(case.masks, case.weights[:-1], *ok[2:])
    with pytest.raises(ValueError, match="peel must be integer"):
        kseq.DeviceKStateMixLikelihood(case.masks, case.weights, case.peel[:, :2], *ok[3:])
    with pytest.raises(ValueError, match="M \\* C <= 16"):
        kseq.DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, 4, 5)
    with pytest.raises(ValueError, match="M 1..8"):
        kseq.DeviceKStateMixLikelihood(case.masks, case.weights, case.peel, case.rooted, case.K, 0, 1)
    with pytest.raises(ValueError, match="params must be"):
        kseq.check_mix_draws(case.blens[None], case.params[None, :-1], case.B, case.K, case.M, case.C)
    with pytest.raises(ValueError, match="blens must be"):
        kseq.check_mix_draws(case.blens[None, :-1], case.params[None], case.B, case.K, case.M, case.C)
    with pytest.raises(AssertionError, match="the library was touched"):  # valid data reaches the library
        kseq.DeviceKStateMixLikelihood(*ok)


def test_resource_table_has_no_scratch():
    """profiles/kseq_mix_resources.json: the gfx950 cross-compile's figures of the five kernels beside the parent's."""
    table = json.load(open(os.path.join(ROOT, "profiles", "kseq_mix_resources.json")))
    assert sorted(table["kernels"]) == ["kseq_combine_kernel", "kseq_down_kernel", "kseq_eig_kernel",
                                        "kseq_site_kernel", "kseq_up_kernel"]
    for name, k in table["kernels"].items():
        assert k["scratch_bytes_per_lane"] == 0 and k["parent"]["scratch_bytes_per_lane"] == 0, name
        assert k["vgprs"] <= 256 and k["agprs"] <= 256, name
