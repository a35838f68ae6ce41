"""Latency of the sequence-summary engine (phy_seqsum_add: node posteriors,
category posteriors and site rates of n draws, summed on the device) on one
MI355X, against a plain evaluation (phy_eval, compact rows) of the same draws
on the same machine and against the numpy restatement (seqsum_host) on one
host thread.

Shapes: fluA (S = 69, P = 238, C = 4, HKY) at 1 and 100 draws, and the first of
8 pattern shards of the synthetic workload (S = 128, C = 4, GTR; bench.py's
problem) at 1 draw.  Timing as tools/forest_latency.py: host clock around the
synchronous calls, median of 5 windows of >= 0.5 s, fastest and slowest window
beside it; the host restatement is timed over whole calls (at least one).

    python tools/seqsum_latency.py [--out profiles/seqsum_latency.json] [--window 0.5] [--sites 1000000]
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

from phylostan_amd import models, seqsum  # noqa: E402
from phylostan_amd.engine import TreeLikelihood  # noqa: E402
from tests import cases  # noqa: E402


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


def shapes(sites):
    flu = cases.fluA_case()
    for n in (1, 100):
        yield "fluA", flu.tipcodes, flu.weights, flu.peel0, True, "HKY", 4, flu.blens, flu.model_vec(), n
    from bench import synthetic_problem
    p = synthetic_problem(sites)
    P8 = (p["tipcodes"].shape[1] + 7) // 8
    mv = models.model_vector(p["freqs"], p["rates"], p["rs"], p["ps"])
    yield ("synthetic shard 1 of 8", np.ascontiguousarray(p["tipcodes"][:, :P8]), p["weights"][:P8], p["peel0"], True,
           "GTR", 4, p["blens"], mv, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "seqsum_latency.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--sites", type=int, default=1_000_000)
    arg = ap.parse_args()
    rows = []
    for name, tip, w, peel0, rooted, model, C, blens, mv, n in shapes(arg.sites):
        rng = np.random.default_rng(1)
        bl = blens[None, :] * rng.uniform(0.8, 1.25, (n, 1))
        mvs = np.repeat(mv[None], n, axis=0)
        summ = seqsum.SequenceSummaries(tip, w, peel0, rooted, model, C, max_draws=n)
        lik = TreeLikelihood(tip, w, peel0, rooted, model, C, max_draws=n)
        lik.set_output(compact=True)
        if n * C <= 256:
            lik.prefer_latency_engine()
        host = seqsum.seqsum_host(tip, w, peel0, rooted, model, C)
        # the three compute the same things
        dev_rows = summ.evaluate_rows(bl, mvs)
        ev = lik.evaluate_rows(bl, mvs)
        assert np.max(np.abs(dev_rows[:, 0] - ev[:, 0]) / np.abs(ev[:, 0])) < 1e-10
        t0 = time.perf_counter()
        host_row = host.evaluate_rows(bl[:1], mvs[:1])[0]
        host_s = time.perf_counter() - t0
        assert np.max(np.abs(host_row[1:] - dev_rows[0, 1:])) < 1e-9

        def add():
            summ.add(bl, mvs)

        a = windows(add, arg.window)
        e = windows(lambda: lik.evaluate_rows(bl, mvs), arg.window)
        plan = seqsum.plan_seqsum(tip, peel0, rooted, C, n, model)
        row = {"shape": name, "S": int(tip.shape[0]), "P": int(tip.shape[1]), "C": C, "draws": n,
               "draws_per_launch": plan["draws_per_launch"], "workspace_bytes_per_draw": plan["workspace_bytes"],
               "row_doubles": plan["row_len"],
               "seqsum_add_us": a[0] * 1e6, "seqsum_add_us_min": a[1] * 1e6, "seqsum_add_us_max": a[2] * 1e6,
               "seqsum_reps_per_window": a[3],
               "phy_eval_us": e[0] * 1e6, "phy_eval_us_min": e[1] * 1e6, "phy_eval_us_max": e[2] * 1e6,
               "seqsum_over_phy_eval": a[0] / e[0],
               "seqsum_host_one_draw_us": host_s * 1e6, "host_per_draw_over_seqsum_per_draw": host_s / (a[0] / n)}
        rows.append(row)
        print(json.dumps(row), flush=True)
        summ.close()
        lik.close()
    doc = {"what": "phy_seqsum_add (n draws evaluated and added to the device sum) against phy_eval (compact rows, the "
                   "engine the CLI picks) on the same draws, and seqsum_host (numpy, one thread, one draw); host clock "
                   "around the synchronous calls through the Python bindings, median of 5 windows of >= %g s" % arg.window,
           "rows": rows}
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
