"""CPU: the planner and the boundary of the K-state sequence engine.

* tests/kseq_plan_check.cpp, built by g++ alone with the address and
  undefined-behaviour sanitizers (the header is device-free), run as a child
  process: every offset the kernels form against the sizes the plan gives,
  every host array written end to end, every refusal;
* with the library built, on a machine without a device: the refusals of
  ``phy_kseq_create`` come back as PHY_EINVAL with their own message (they are
  made before the first device call), ``phy_kseq_eval(NULL, ...)`` is refused,
  and ``plan_kseq`` gives the numbers the check program prints;
* ``_lib.KSEQ_SIGNATURES`` against the prototypes of the headers;
* ``DeviceKStateLikelihood``'s own checks, made before the library is touched.
"""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from phylostan_amd import _lib, kseq
from tests import kseq_truth as kt

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PHY_EINVAL = 1


@pytest.fixture(scope="module")
def check_output(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("kseq_plan") / "kseq_plan_check")
    # the sanitizer runtimes linked in: the program needs nothing preloaded
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
           "-static-libasan", "-static-libubsan", "-I" + os.path.join(ROOT, "include"),
           "-I" + os.path.join(ROOT, "phylostan_amd", "csrc"), "-o", exe,
           os.path.join(ROOT, "tests", "kseq_plan_check.cpp")]
    built = subprocess.run(cmd, capture_output=True, text=True)
    if built.returncode != 0 and ("asan" in built.stderr or "ubsan" in built.stderr) and "cannot find" in built.stderr:
        pytest.skip("g++ cannot link the sanitizer runtime")
    assert built.returncode == 0, built.stderr[-2000:]
    run = subprocess.run([exe], capture_output=True, text=True)
    assert run.returncode == 0, (run.stdout + run.stderr)[-2000:]
    return run.stdout


def test_planner_under_host_sanitizers(check_output):
    assert "0 failures" in check_output and "FAIL" not in check_output


def _lib_built():
    return os.path.exists(_lib.LIB_PATH)


needs_lib = pytest.mark.skipif(not _lib_built(), reason="HIP library not built (run __graft_entry__.build())")


def _flu_codon_shape():
    """S = 69, P = 242, K = 61, C = 4, rooted: the numbers of a plan depend on the shape alone."""
    rng = np.random.default_rng(3)
    S, P = 69, 242
    masks = kt.random_masks(S, P, 61, rng)
    return masks, np.ones(P), kt.rooted_peel(S, rng)


@needs_lib
def test_plan_kseq_agrees_with_the_check_program(check_output):
    line = [ln for ln in check_output.splitlines() if ln.startswith("fluA_codon ")]
    assert len(line) == 1
    want = {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", line[0])}
    masks, w, peel = _flu_codon_shape()
    got = kseq.plan_kseq(masks, w, peel, True, 61, 4, max_draws=32, cu_count=256)
    assert got == want
    assert got["items_per_draw"] == 64 and got["chunk_draws"] >= 1 and got["KT"] == 64
    assert max(got["lds_up"], got["lds_down"], got["lds_draw"]) <= 160 * 1024


def _create(S, P, K, C, rooted, masks, w, peel, max_draws=1):
    lib = _lib.load()
    ctx = ctypes.c_void_p()
    ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    rc = lib.phy_kseq_create(S, P, K, C, rooted, ptr(masks), ptr(w), ptr(peel), max_draws, 0, ctypes.byref(ctx))
    msg = lib.phy_last_error().decode()
    if rc == 0:
        lib.phy_kseq_destroy(ctx)
    return rc, msg


@needs_lib
def test_create_refusals_come_before_the_device():
    case = kt.small_cases()[4]  # K = 17, S = 7, P = 17, C = 4, unrooted
    S, P, K, C = case.S, case.P, case.K, case.C
    m, w, peel = case.masks, case.weights, np.ascontiguousarray(case.peel, np.int32)

    def edit(a, at, v):
        b = a.copy()
        b[at] = v
        return b

    swapped = peel.copy()
    swapped[-1, 0], swapped[-1, 1] = peel[-1, 1], peel[-1, 0]
    rows = [
        ((2, P, K, C, 0, m, w, peel), "S = 2"),
        ((S, 0, K, C, 0, m, w, peel), "P = 0"),
        ((S, P, 1, C, 0, m, w, peel), "K = 1 states, supported 2..64"),
        ((S, P, 65, C, 0, m, w, peel), "K = 65 states, supported 2..64"),
        ((S, P, K, 0, 0, m, w, peel), "C = 0 categories, supported 1..16"),
        ((S, P, K, 17, 0, m, w, peel), "C = 17 categories, supported 1..16"),
        ((S, P, K, C, 0, m, w, peel, 0), "max_draws must be >= 1"),
        ((S, P, K, C, 0, None, w, peel), "tipmasks is NULL"),
        ((S, P, K, C, 0, m, None, peel), "weights is NULL"),
        ((S, P, K, C, 0, m, w, None), "peel is NULL"),
        ((S, P, K, C, 0, edit(m, (2, 3), 0), w, peel), "tipmasks[2][3] has no bit set"),
        ((S, P, K, C, 0, edit(m, (2, 3), 1 << 17), w, peel), "tipmasks[2][3] has a bit >= K set"),
        ((S, P, K, C, 0, m, edit(w, 5, -1.0), peel), "weights[5] is negative or not finite"),
        ((S, P, K, C, 0, m, edit(w, 5, np.inf), peel), "weights[5] is negative or not finite"),
        ((S, P, K, C, 0, m, w, edit(peel, (1, 0), 99)), "peel row 1: node id out of range"),
        ((S, P, K, C, 0, m, w, edit(peel, (1, 1), peel[1, 0])), "peel row 1: the two children are the same node"),
        ((S, P, K, C, 0, m, w, edit(peel, (1, 2), peel[0, 2])), "peel row 1: the parent is computed twice"),
        ((S, P, K, C, 0, m, w, swapped), "the last peel row must be (child1, 2S-3, 2S-2)"),
    ]
    for args, needle in rows:
        rc, msg = _create(*args)
        assert rc == PHY_EINVAL, (needle, rc, msg)
        assert needle in msg and "device" not in msg, (needle, msg)


@needs_lib
def test_eval_refuses_a_null_context():
    lib = _lib.load()
    x = np.zeros(8)
    rc = lib.phy_kseq_eval(None, 1, x.ctypes.data, x.ctypes.data, x.ctypes.data, None)
    assert rc == PHY_EINVAL and "NULL ctx" in lib.phy_last_error().decode()
    assert lib.phy_kseq_row_len(None) == -1 and lib.phy_kseq_num_branches(None) == -1
    assert lib.phy_kseq_info(None, 0, None, None) == PHY_EINVAL


def _prototypes(path):
    """name -> list of 'ptr' / 'int' per argument, of every phy_kseq_* prototype of a header."""
    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\bint\s+(phy_kseq_\w+)\s*\(([^)]*)\)\s*;", text):
        out[name] = ["ptr" if "*" in a else "int" for a in args.split(",")]
        assert all(re.match(r"\s*(const\s+)?(long\s+)?\w+\s*\**\s*\w+\s*$", a) for a in args.split(",")), (name, args)
    return out


def test_signatures_match_the_headers():
    protos = _prototypes(os.path.join(ROOT, "include", "phylo_hip_kseq.h"))
    assert sorted(protos) == ["phy_kseq_create", "phy_kseq_destroy", "phy_kseq_eval", "phy_kseq_num_branches",
                              "phy_kseq_row_len"]
    diag = _prototypes(os.path.join(ROOT, "include", "phylo_hip_diag.h"))
    assert sorted(diag) == ["phy_kseq_info", "phy_kseq_plan"]
    protos.update(diag)
    assert sorted(protos) == sorted(_lib.KSEQ_SIGNATURES)
    for name, kinds in protos.items():
        res, args = _lib.KSEQ_SIGNATURES[name]
        assert res is ctypes.c_int
        got = ["int" if a is ctypes.c_int else "ptr" for a in args]
        assert got == kinds, name
    # phylo_hip.h includes the new header after the seqsum one and declares nothing of it itself
    main = open(os.path.join(ROOT, "include", "phylo_hip.h")).read()
    assert main.index('#include "phylo_hip_seqsum.h"') < main.index('#include "phylo_hip_kseq.h"')
    assert "phy_kseq_create(" not in main


def test_wrapper_validates_before_the_library(monkeypatch):
    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(_lib, "load", no_library)
    case = kt.small_cases()[1]
    ok = (case.masks, case.weights, case.peel, case.rooted, case.K, case.C)
    with pytest.raises(ValueError, match="tipmasks must be \\[S, P\\]"):
        kseq.DeviceKStateLikelihood(case.masks[0], *ok[1:])
    with pytest.raises(ValueError, match="integer masks"):
        kseq.DeviceKStateLikelihood(case.masks.astype(float), *ok[1:])
    with pytest.raises(ValueError, match="weights must be"):
        kseq.DeviceKStateLikelihood(case.masks, case.weights[:-1], *ok[2:])
    with pytest.raises(ValueError, match="peel must be integer"):
        kseq.DeviceKStateLikelihood(case.masks, case.weights, case.peel[:, :2], *ok[3:])
    with pytest.raises(ValueError, match="peel must be integer"):
        kseq.DeviceKStateLikelihood(case.masks, case.weights, case.peel.astype(float), *ok[3:])
    with pytest.raises(ValueError, match="params must be"):
        kseq.check_draws(case.blens[None], case.params[None, :-1], case.B, case.K, case.C)
    with pytest.raises(ValueError, match="blens must be"):
        kseq.check_draws(case.blens[None, :-1], case.params[None], case.B, case.K, case.C)
    with pytest.raises(AssertionError, match="the library was touched"):  # valid data reaches the library
        kseq.DeviceKStateLikelihood(*ok)


def test_main_binds_the_device_likelihood(monkeypatch):
    """``cli.main`` hands ``run --codon`` the device class; ``cli.run`` without a likelihood still refuses."""
    from phylostan_amd import cli
    seen = {}
    monkeypatch.setattr(cli, "run", lambda arg, **kw: seen.update(kw, codon=arg.codon))
    cli.main(["run", "-s", "x.stan", "-m", "HKY", "--codon", "-t", "t", "-i", "a", "-o", "o"])
    assert seen == {"likelihood_factory": kseq.DeviceKStateLikelihood, "codon": True}
    seen.clear()
    cli.main(["run", "-s", "x.stan", "-m", "HKY", "-t", "t", "-i", "a", "-o", "o"])
    assert seen == {"codon": False}
