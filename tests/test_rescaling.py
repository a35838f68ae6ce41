"""CPU: the extended-range reference of the rescaled sweep's GPU tests
(tests/extended_oracle.py) and the rescaling switch's declarations: the diag
header, the ctypes binding and the run parser's --rescaling."""
import argparse
import os
import re

import numpy as np

from tests import cases
from tests.extended_oracle import extended_oracle, require_extended

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_extended_oracle_equals_the_oracle_where_nothing_underflows():
    require_extended()
    case = cases.random_case(901, S=12)
    ref, ext = case.oracle(), extended_oracle(case)
    assert set(ext) == set(ref)
    for k in ref:
        a, b = np.asarray(ext[k]), np.asarray(ref[k])
        assert a.dtype == np.float64 or np.ndim(ext[k]) == 0
        assert np.max(np.abs(a - b)) <= 1e-14 * np.max(np.abs(b)), k


def test_extended_oracle_is_finite_where_fp64_underflows():
    require_extended()
    case = cases.random_case(911, S=700, P=130, C=2, model="GTR")
    ref = case.oracle()
    assert ref["loglik"] == -np.inf and np.all(np.isneginf(ref["site_ll"]))
    ext = extended_oracle(case)
    for k, v in ext.items():
        assert np.all(np.isfinite(v)), k
    assert ext["site_ll"].shape == (130,) and np.all(ext["site_ll"] < np.log(np.finfo(np.float64).tiny))


def test_switch_is_declared_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "phylo_hip_diag.h")).read(), flags=re.S)
    assert re.search(r"\bint\s+phy_set_rescaling\s*\(\s*phy_ctx\s*\*\s*\w+\s*,\s*int\s+\w+\s*\)\s*;", text)
    assert re.search(r"\bint\s+phy_rescaling\s*\(\s*const\s+phy_ctx\s*\*\s*\w+\s*\)\s*;", text)
    import ctypes
    from phylostan_amd import _lib
    assert _lib.SIGNATURES["phy_set_rescaling"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int])
    assert _lib.SIGNATURES["phy_rescaling"] == (ctypes.c_int, [ctypes.c_void_p])


def test_run_parser_takes_rescaling():
    from phylostan_amd import cli
    parser = argparse.ArgumentParser()
    p = cli.create_run_parser(parser.add_subparsers())
    base = ["run", "-s", "m.stan", "-t", "t.tree", "-o", "out"]
    assert parser.parse_args(base).rescaling is False
    assert parser.parse_args(base + ["--rescaling"]).rescaling is True
    # the reference's --rescaling_geo (phylogeography) stays a separate option
    assert parser.parse_args(base + ["--rescaling"]).rescaling_geo is False
    assert "rescaling_geo" in p.format_help()
