"""Writes tests/golden/row_engine_rows_parent.npz: the bits an MI355X gave at
the commit before the forest and the partitioned engine moved onto the shared
host path of csrc/row_engine.inc, for every form their exact suites construct
(HKY, rooted), and one sequence-summary case.

    python tests/golden/record_row_engine_rows.py [OUT]

  forest/<form>/{rows,site}     the mixed call of tests/forest_exact_cases.py, the six forms of
                                tests/test_forest_exact_cpu.py (all four epilogue placements)
  part/<form>/{out,rows,site}   the call of tests/part_exact_cases.py (S = 12, P = 130 cut 64 / 65 / 1),
                                the 14 forms of tests/test_part_exact_cpu.py
  seqsum/{rows,ll,total,nfin}   seqsum_cases.shape_case(0): evaluate_rows, then add twice and read

(site of forest/C10 and part/no-deep-entries is left out: LEFT_OUT.)  Every array is computed twice, in two contexts, and kept only if the two runs
agree bit for bit.  A form's array is stored as the XOR of its bits with the
bits of the engine's first form of that array's shape (the forms of one engine
mostly agree to the last bit or nearly, so these compress to little); load()
undoes it.  tests/test_row_engine_bits_gpu.py holds every later host-side
change to these rows: rerun only on a commit whose rows are meant to change."""
import os
import sys

import numpy as np
import pytest
import torch  # noqa: F401 -- torch's own HIP runtime must load before the engine's

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from phylostan_amd import seqsum  # noqa: E402
from tests import forest_exact_cases as fx, part_exact_cases as px, seqsum_cases as sc  # noqa: E402
from tests import test_forest_exact_cpu as fcpu, test_part_exact_cpu as pcpu  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden", "row_engine_rows_parent.npz")
CASES = [("forest", form) for form in fcpu.FORMS] + [("part", form) for form in pcpu.FORMS] + [("seqsum", "rows")]
# site_ll that shares no bits with another form's (ten categories; another tree): with them the file passes 100 KB
LEFT_OUT = ("forest/C10/site", "part/no-deep-entries/site")


def compute(engine, form, monkeypatch):
    """{array name: array} of one case, in a context of its own."""
    if engine == "forest":
        max_rows, C, facts = fcpu.set_form(form, monkeypatch)
        f = fx.edge_forest("HKY", True, C)
        eng = f.engine(max_rows)
        fcpu.assert_form(f, form, max_rows, facts, info=eng.info())
        rows, site = eng.evaluate_rows(f.tree_of_row, f.blens, f.model_vecs, site_ll=True)
        eng.close()
        return {"rows": rows, "site": site}
    if engine == "part":
        max_draws, C, tree, facts = pcpu.set_form(form, monkeypatch)
        e = px.edge_part("HKY", True, C, tree)
        eng = e.engine(max_draws)
        pcpu.assert_form(e, form, max_draws, facts, info=eng.info())
        out, rows, site = eng.evaluate_rows(e.blens, e.mu, e.model_vecs, part_rows=True, site_ll=True)
        eng.close()
        return {"out": out, "rows": rows, "site": site}
    case = sc.shape_case(0)
    bl, mv = sc.draws(case, 3)
    eng = seqsum.SequenceSummaries(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C, max_draws=2)
    rows = eng.evaluate_rows(bl, mv)
    ll = np.concatenate([eng.add(bl[:2], mv[:2]), eng.add(bl[2:], mv[2:])])
    total, nfin = eng.read()
    eng.close()
    return {"rows": rows, "ll": ll, "total": total, "nfin": np.array([nfin], np.float64)}


def record():
    """{"engine/form/array": float64 array}: what two runs agree on."""
    runs = []
    for _ in range(2):
        got = {}
        for engine, form in CASES:
            with pytest.MonkeyPatch.context() as mp:
                for k, v in compute(engine, form, mp).items():
                    if "%s/%s/%s" % (engine, form, k) in LEFT_OUT:
                        continue
                    got["%s/%s/%s" % (engine, form, k)] = np.ascontiguousarray(v, np.float64)
        runs.append(got)
    keep = {}
    for k, v in runs[0].items():
        if v.tobytes() == runs[1][k].tobytes():
            keep[k] = v
        else:
            print("NOT reproducible run to run, left out: %s" % k)
    return keep


def encode(arrays):
    base, out = {}, {}
    for key, v in arrays.items():
        engine, _, name = key.split("/")
        b = base.setdefault((engine, name, v.shape), key)
        if b == key:
            out[key] = v
        else:
            out["%s^%s" % (key, b)] = v.view(np.uint64) ^ arrays[b].view(np.uint64)
    return out


def load(path=GOLDEN):
    with np.load(path) as z:
        stored = {k: z[k] for k in z.files}
    out = {k: v for k, v in stored.items() if "^" not in k}
    for k, v in stored.items():
        if "^" in k:
            key, b = k.split("^")
            out[key] = (v ^ out[b].view(np.uint64)).view(np.float64)
    return out


if __name__ == "__main__":
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    arrays = record()
    np.savez_compressed(out, **encode(arrays))
    back = load(out)
    assert set(back) == set(arrays) and all(back[k].tobytes() == arrays[k].tobytes() for k in arrays)
    print("recorded %d arrays, %d bytes" % (len(arrays), os.path.getsize(out)))
