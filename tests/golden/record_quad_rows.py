"""Writes tests/golden/quad_rows_parent.npz: the bits an MI355X gave at the
commit before the two quad sweeps (csrc/quad_engine.inc: qsweep_kernel,
qmw_kernel) took their shared phases and their LDS layouts from one statement
each, on the smallest calls at which every path of the two kernels is live.

    python tests/golden/record_quad_rows.py [OUT]

  hky3  exact_cases ctl_hky3 (S 12, P 130: 9 blocks, C 4, HKY, rooted, ambiguity codes: R = 9)
  unr5  an unrooted GTR tree of 8 taxa, P 257: 17 blocks, C 5 (the merged root branch is the matrix-less
        step; qsweep_kernel<1024>; at most 3 waves per category) -- exact_cases' ctl_gtr4_unrooted has
        this shape at 17 taxa, and its four distinct full rows alone are 80 KB of the file's 100
  c16   test_gpu_quad's rand_C16_HKY (C > 8: one wave per category only)
  jc1   JC69, C 1, S 17, P 333 (qbuild_records' JC69 branch)

Forms "one" (PHY_QMW=0) and "mw" (the default); calls of one context, all on the same 32 draws:
  n1     evaluate of draw 0 with site_ll (host buffers: the kernel builds its records)
  n32    evaluate_rows of the 32 draws (host buffers; fewer workgroups than blocks: the later blocks of a
         workgroup add to its dL/dP slot)
  n4dev  evaluate_device of draws 0, 1, 2, 31 (no eigensystems: the kernel copies pmat_kernel's records)
Kept of a call: `compact`, the rows up to the dL/dP block; `full_d<k>`, the whole row of its first and last
draw, where LEFT_OUT does not name it; `site` of n1.  Every array is computed twice, in two contexts, and
kept only if the two runs agree bit for bit; record_row_engine_rows' encode / load store a form's array as
the XOR with the case's first array of that name and shape (the forms equal by contract -- one wave and
several, built records and copied -- are then zeros).  tests/test_quad_bits_gpu.py holds every later change
of the two kernels to these rows: rerun only on a commit whose rows are meant to change."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phylostan_amd import engine as eng_mod  # noqa: E402
from tests import cases, exact_cases  # noqa: E402
from tests.golden.record_row_engine_rows import encode, load as _load  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "quad_rows_parent.npz")
NDRAWS = 32
DEV_DRAWS = (0, 1, 2, 31)

MAKE = {
    "hky3": exact_cases.CASES["ctl_hky3"],
    "unr5": lambda: cases.random_case(4, S=8, P=257, C=5, model="GTR", rooted=False),
    "c16": lambda: cases.random_case(303, S=12, P=77, C=16, model="HKY"),
    "jc1": lambda: cases.random_case(301, S=17, P=333, C=1, model="JC69"),
}
# (case, form): the calls; waves: what quad_plan() must say of the context
CASES = [("hky3", "one"), ("hky3", "mw"), ("unr5", "one"), ("unr5", "mw"), ("c16", "mw"), ("jc1", "one"), ("jc1", "mw")]
CALLS = {"hky3": ("n1", "n32", "n4dev"), "unr5": ("n4dev", "n32"), "c16": ("n4dev",), "jc1": ("n4dev",)}
WAVES = {("hky3", "mw"): (4, 4), ("unr5", "mw"): (2, 3), ("c16", "mw"): (1, 1), ("jc1", "mw"): (2, 4)}
# full rows left out: 16 categories make a row 45 KB, two of them half the file's budget; their compact
# parts (every gradient is a sum over the dL/dP block) stay
LEFT_OUT = tuple("c16/mw.n4dev/full_d%d" % k for k in (DEV_DRAWS[0], DEV_DRAWS[-1]))


def draws(case):
    rng = np.random.default_rng(41)
    bl = case.blens[None, :] * rng.uniform(0.7, 1.4, (NDRAWS, case.blens.size))
    return bl, np.repeat(case.model_vec()[None], NDRAWS, axis=0)


def assert_form(eng, case, name, form, cu_count):
    """The form under test is the one a call of this context launches."""
    assert eng.engine() == "pattern" and not eng.rescaling()
    assert eng.lds_plan()["cols"] in (1, 2)  # no explicit column plan displaces the quad sweep: see `launch`
    plan = eng.quad_plan()
    lo, hi = WAVES.get((name, form), (1, 1))
    assert lo <= plan["waves"] <= hi, plan
    assert (plan["span"] == case.S - 1) == (plan["waves"] == 1), plan
    nblk = (case.P + 15) // 16
    for call in CALLS[name]:
        n = {"n1": 1, "n32": NDRAWS, "n4dev": len(DEV_DRAWS)}[call]
        launch = eng_mod.plan_sweep(case.tipcodes, case.peel0, case.rooted, case.C, NDRAWS, cu_count, n)["launch"]
        assert launch["path"] == ("quad_mw" if plan["waves"] > 1 else "quad"), launch
        # one block per workgroup in the small calls; at 32 draws a workgroup walks several
        assert launch["gx"] == (nblk if n < NDRAWS or name == "jc1" else {"hky3": 8, "unr5": 6}[name]), launch


def compute(name, form, monkeypatch):
    """{"call/array": array} of one (case, form), in a context of its own."""
    case = MAKE[name]()
    monkeypatch.setenv("PHY_QUAD", "1")
    monkeypatch.setenv("PHY_QMW", "0" if form == "one" else "1")
    eng = eng_mod.TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C,
                                 max_draws=NDRAWS)
    assert_form(eng, case, name, form, torch.cuda.get_device_properties(0).multi_processor_count)
    bl, mv = draws(case)
    nc = 1 + eng.B + 2 * case.C + 14  # the compact part of a row
    out = {}

    def keep(call, rows, ids):
        out["%s/compact" % call] = rows[:, :nc]
        for k in sorted({0, len(ids) - 1}):
            out["%s/full_d%d" % (call, ids[k])] = rows[k]

    for call in CALLS[name]:
        if call == "n1":
            vec = np.empty((1, eng.outlen))
            site = np.empty((1, case.P))
            eng_mod._lib.check(eng.lib.phy_eval(eng.ctx, 1, eng_mod._ptr(np.ascontiguousarray(bl[:1])),
                                                eng_mod._ptr(np.ascontiguousarray(mv[:1])), eng_mod._ptr(vec),
                                                eng_mod._ptr(site)), "phy_eval")
            keep(call, vec, [0])
            out["%s/site" % call] = site[0]
        elif call == "n32":
            keep(call, eng.evaluate_rows(bl, mv), list(range(NDRAWS)))
        else:
            ids = list(DEV_DRAWS)
            d_bl, d_mv = torch.tensor(bl[ids], device="cuda:0"), torch.tensor(mv[ids], device="cuda:0")
            d_out = torch.zeros((len(ids), eng.outlen), dtype=torch.float64, device="cuda:0")
            eng.evaluate_device(d_bl.data_ptr(), d_mv.data_ptr(), d_out.data_ptr(), 0, n_draws=len(ids))
            torch.cuda.synchronize()
            keep(call, d_out.cpu().numpy(), ids)
    eng.close()
    return {k: np.ascontiguousarray(v, np.float64) for k, v in out.items()}


def key(name, form, k):
    call, arr = k.split("/")
    return "%s/%s.%s/%s" % (name, form, call, arr)


def record():
    """{"case/form.call/array": float64 array}: what two runs agree on."""
    runs = []
    for _ in range(2):
        got = {}
        for name, form in CASES:
            with pytest.MonkeyPatch.context() as mp:
                for k, v in compute(name, form, mp).items():
                    if key(name, form, k) not in LEFT_OUT:
                        got[key(name, form, k)] = v
        runs.append(got)
    keep = {}
    for k, v in runs[0].items():
        if v.tobytes() == runs[1][k].tobytes():
            keep[k] = v
        else:
            print("NOT reproducible run to run, left out: %s" % k)
    return keep


def load(path=GOLDEN):
    return _load(path)


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = record()
    np.savez_compressed(out, **encode(arrays))
    back = load(out)
    assert set(back) == set(arrays) and all(back[k].tobytes() == arrays[k].tobytes() for k in arrays)
    print("recorded %d arrays, %d bytes" % (len(arrays), os.path.getsize(out)))
