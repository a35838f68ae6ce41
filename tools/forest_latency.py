"""Latency of the forest call (phy_forest_eval, one launch for T trees x g
rows) against the same work on T single-tree contexts, on one MI355X.

Shapes: the 42 DS1 topologies (tests/golden/DS1_topologies.npz in topology 0's
tip order; JC69, C = 1, unrooted) and a fluA-sized forest (S = 69, P = 238,
C = 4, HKY, rooted: fluA's peel plus 41 seeded random peels), each at g = 1, 4
and 100 rows per tree.  Baselines, both the engine as it was:
  (a) T ``TreeLikelihood`` contexts set up as the CLI sets them (compact rows,
      ``prefer_latency_engine()`` where max_draws * C <= 256), ``evaluate_rows``
      one after another;
  (b) the same contexts, ``submit_rows`` on all, then ``wait_rows`` on all
      (g <= 128: phy_eval_submit's limit).
Timing as tools/geo_latency.py: host clock around the synchronous calls,
median of 5 windows of >= 0.5 s, fastest and slowest window beside it.

    python tools/forest_latency.py [--out profiles/forest_latency.json] [--window 0.5]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from phylostan_amd.engine import TreeLikelihood  # noqa: E402
from phylostan_amd.forest import ForestLikelihood  # noqa: E402
from tests import cases, forest_cases  # noqa: E402

ROWS_PER_TREE = [1, 4, 100]


def windows(fn, min_seconds=0.5, n_windows=5):
    """Seconds per call: median, fastest and slowest of n_windows windows."""
    for _ in range(3):
        fn()
    t0 = time.perf_counter()
    fn()
    reps = max(3, int(min_seconds / max(time.perf_counter() - t0, 1e-6)))
    out = []
    for _ in range(n_windows):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps)
    out.sort()
    return out[len(out) // 2], out[0], out[-1], reps


def shapes():
    tip0, w, peels, blens, _, _ = forest_cases.ds1_forest()
    mv = cases.ds1_case().model_vec()
    yield "DS1", tip0, w, peels, False, "JC69", 1, blens, mv
    flu = cases.fluA_case()
    fpeels = np.array([flu.peel0] + [cases.random_peel(flu.S, np.random.default_rng(100 + s)) for s in range(41)],
                      dtype=np.int32)
    yield "fluA-sized", flu.tipcodes, flu.weights, fpeels, True, "HKY", 4, np.repeat(flu.blens[None], 42, axis=0), \
        flu.model_vec()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forest_latency.json"))
    ap.add_argument("--window", type=float, default=0.5)
    arg = ap.parse_args()
    rows = []
    for name, tip, w, peels, rooted, model, C, blens, mv in shapes():
        T = peels.shape[0]
        rng = np.random.default_rng(1)
        for g in ROWS_PER_TREE:
            n = T * g
            tree = np.repeat(np.arange(T, dtype=np.int32), g)
            bl = np.repeat(blens, g, axis=0) * rng.uniform(0.8, 1.25, (n, 1))
            mvs = np.repeat(mv[None], n, axis=0)
            forest = ForestLikelihood(tip, w, peels, rooted, model, C, max_rows=n)
            singles = []
            for t in range(T):
                lk = TreeLikelihood(tip, w, peels[t], rooted, model, C, max_draws=g)
                lk.set_output(compact=True)
                if g * C <= 256:
                    lk.prefer_latency_engine()
                singles.append(lk)
            parts = [(bl[tree == t], mvs[tree == t]) for t in range(T)]
            ref = forest.evaluate_rows(tree, bl, mvs)
            for t in range(T):  # the three ways compute the same rows
                got = singles[t].evaluate_rows(*parts[t])
                err = np.max(np.abs(got[:, :forest.outlen] - ref[tree == t])) / np.max(np.abs(ref[tree == t]))
                assert err < 1e-9, (name, g, t, err)

            def serial():
                for lk, (b, m) in zip(singles, parts):
                    lk.evaluate_rows(b, m)

            def overlapped():
                for lk, (b, m) in zip(singles, parts):
                    lk.submit_rows(b, m)
                for lk in singles:
                    lk.wait_rows()

            f = windows(lambda: forest.evaluate_rows(tree, bl, mvs), arg.window)
            a = windows(serial, arg.window)
            b = windows(overlapped, arg.window) if g <= 128 else None
            row = {"shape": name, "trees": T, "rows_per_tree": g, "rows": n, "forest_plan": forest.info(),
                   "forest_us": f[0] * 1e6, "forest_us_min": f[1] * 1e6, "forest_us_max": f[2] * 1e6,
                   "forest_reps_per_window": f[3],
                   "serial_contexts_us": a[0] * 1e6, "serial_contexts_us_min": a[1] * 1e6,
                   "serial_contexts_us_max": a[2] * 1e6, "serial_over_forest": a[0] / f[0]}
            if b:
                row.update({"overlapped_contexts_us": b[0] * 1e6, "overlapped_contexts_us_min": b[1] * 1e6,
                            "overlapped_contexts_us_max": b[2] * 1e6, "overlapped_over_forest": b[0] / f[0]})
            rows.append(row)
            print(json.dumps(row), flush=True)
            forest.close()
            for lk in singles:
                lk.close()
    doc = {"what": "phy_forest_eval (one call, T trees x g rows) against T single-tree contexts evaluated one after "
                   "another (serial_contexts) and submitted together then collected (overlapped_contexts); host clock "
                   "around the synchronous calls through the Python bindings, median of 5 windows of >= %g s" % arg.window,
           "rows": rows}
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
