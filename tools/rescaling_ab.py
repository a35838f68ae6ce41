#!/usr/bin/env python3
"""What the rescaled pattern sweep costs where the plain one also works.

One context per workload, rescaling toggled between rounds (the plan, the
buffers and the inputs stay the same), the sweep launch timed with HIP
events (phy_timing_start / phy_timing_read):

  fluA, 8,192 draws             the batched throughput plan (two columns per lane)
  430 taxa x 300 x C=16, 32     tests/test_gpu_large_cb.py's tree (one column per lane)

and the absolute time of one evaluation of a tree that only the rescaled
sweep can evaluate (700 taxa, tests/test_gpu_rescaling.py's first case), at 1
and 40 draws.  Writes profiles/rescaling_ab.json.

    python tools/rescaling_ab.py [--rounds 3] [--launches 5] [--out profiles/rescaling_ab.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def draws_of(case, n, seed=5):
    rng = np.random.default_rng(seed)
    bl = case.blens[None, :] * rng.uniform(0.8, 1.25, (n, case.blens.size))
    return bl, np.repeat(case.model_vec()[None], n, axis=0)


def timed(eng, bl, mv, launches):
    eng.evaluate_rows(bl, mv)  # warm
    eng.timing_start()
    for _ in range(launches):
        eng.evaluate_rows(bl, mv)
    ms, n = eng.timing_read()
    return ms / n


def ab(case, n, rounds, launches):
    from phylostan_amd.engine import TreeLikelihood
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C, max_draws=n)
    eng.set_output(compact=True)
    eng.set_engine("pattern")
    bl, mv = draws_of(case, n)
    off, on = [], []
    for _ in range(rounds):
        eng.set_rescaling(False)
        off.append(timed(eng, bl, mv, launches))
        eng.set_rescaling(True)
        on.append(timed(eng, bl, mv, launches))
    eng.set_rescaling(False)
    a = eng.evaluate_rows(bl[:4], mv[:4])
    eng.set_rescaling(True)
    b = eng.evaluate_rows(bl[:4], mv[:4])
    plan, quad = eng.lds_plan(), eng.quad_plan()
    eng.close()
    return {"taxa": case.S, "patterns": case.P, "C": case.C, "model": case.model, "draws": n,
            "cols": plan["cols"], "quad_sweep_applies_when_off": bool(quad["waves"]) and n <= 32,
            "ms_per_launch_off": off, "ms_per_launch_on": on,
            "median_off_ms": float(np.median(off)), "median_on_ms": float(np.median(on)),
            "ratio_on_over_off": float(np.median(on) / np.median(off)),
            "rows_max_rel_diff": float(np.max(np.abs(a - b)) / np.max(np.abs(a)))}


def absolute(case, n, rounds, launches):
    from phylostan_amd.engine import TreeLikelihood
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C, max_draws=n,
                         rescaling=True)
    eng.set_output(compact=True)
    bl, mv = draws_of(case, n)
    ms = [timed(eng, bl, mv, launches) for _ in range(rounds)]
    ll = float(eng.evaluate_rows(bl, mv)[0, 0])
    eng.close()
    return {"taxa": case.S, "patterns": case.P, "C": case.C, "model": case.model, "draws": n,
            "ms_per_launch_on": ms, "median_on_ms": float(np.median(ms)), "loglik_draw0": ll}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rescaling_ab.json"))
    arg = ap.parse_args()
    import torch  # noqa: F401 -- before the engine's runtime
    from tests import cases
    doc = {"timed": "the sweep launch (HIP events, phy_timing_start / phy_timing_read), median over rounds of the "
                    "mean over %d launches, rescaling toggled on one context between rounds" % arg.launches,
           "fluA_8192": ab(cases.fluA_case(), 8192, arg.rounds, arg.launches),
           "taxa430_32": ab(cases.random_case(901, S=430, P=300, C=16, model="GTR"), 32, arg.rounds, arg.launches),
           "taxa700_1": absolute(cases.random_case(911, S=700, P=130, C=2, model="GTR"), 1, arg.rounds, arg.launches),
           "taxa700_40": absolute(cases.random_case(911, S=700, P=130, C=2, model="GTR"), 40, arg.rounds,
                                  arg.launches)}
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
        fp.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
