"""Latency of the discrete-trait engine: ``phy_geo_eval`` at 1, 4 and 100
draws for (S, K) = (69, 5), (69, 20), (69, 64) on fluA's tree with seeded
synthetic locations, beside the one-thread time of ``geo_gradients_host``
(numpy, LAPACK's eigh) on the same box -- the yardstick: a 100-draw call
should beat 100 host evaluations.

Each shape is warmed up (3 calls), then timed over repetitions that fill at
least 0.5 s (host clock around the synchronous call), five such windows, the
median window reported with the fastest and slowest.  The Jacobi sweep counts
of the timed draws are read back.  Writes profiles/geo_latency.json (or
--out).

``--summaries`` times ``phy_geo_eval_summaries`` beside ``phy_geo_eval`` at the
same nine shapes, each in the same windows on the same context, and writes
profiles/geo_summaries_latency.json: the plain call's latency again (to set
beside geo_latency.json) and the summaries call's overhead over it.

    python tools/geo_latency.py [--summaries] [--out FILE] [--device N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the host yardstick is one thread
    os.environ[_v] = "1"

import numpy as np  # noqa: E402

from phylostan_amd import data as dataio  # noqa: E402
from phylostan_amd import geo  # noqa: E402

SHAPES = [(69, 5), (69, 20), (69, 64)]
DRAWS = [1, 4, 100]


def flu_tree():
    tree = dataio.read_tree(os.path.join(ROOT, "tests", "golden", "examples", "fluA", "fluA.tree"))
    tree.resolve_polytomies(update_bipartitions=True)
    dataio.setup_indexes(tree)
    peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
    bl = geo.tree_branch_lengths(tree, peel0)
    return peel0, bl * (0.3 / bl.mean())


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


def summaries(arg):
    peel, blens1 = flu_tree()
    rows = []
    for S, K in SHAPES:
        rng = np.random.default_rng(1000 + K)
        tips = np.zeros((S, K))
        tips[np.arange(S), rng.integers(0, K, S)] = 1.0
        R = geo.rate_count(K)
        params = np.concatenate([0.1 + rng.exponential(1.0, (100, R)), rng.dirichlet(np.ones(K) * 3.0, 100)], axis=1)
        blens = np.tile(blens1, (100, 1))
        eng = geo.GeoLikelihood(tips, peel, max_draws=100, device=arg.device)
        info = eng.info()
        for n in DRAWS:
            plain = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]))
            summ = windows(lambda: eng.evaluate_summaries(blens[:n], params[:n]))
            row = {"S": S, "K": K, "draws": n, "summary_doubles_per_draw": geo.summary_len(S, K),
                   "eval_us": plain[0] * 1e6, "eval_us_min": plain[1] * 1e6, "eval_us_max": plain[2] * 1e6,
                   "summaries_us": summ[0] * 1e6, "summaries_us_min": summ[1] * 1e6, "summaries_us_max": summ[2] * 1e6,
                   "summaries_over_eval": summ[0] / plain[0], **info}
            rows.append(row)
            print("S %d K %2d n %3d: eval %9.1f us (%.1f..%.1f), summaries %9.1f us (%.1f..%.1f), x %.3f"
                  % (S, K, n, row["eval_us"], row["eval_us_min"], row["eval_us_max"], row["summaries_us"],
                     row["summaries_us_min"], row["summaries_us_max"], row["summaries_over_eval"]), flush=True)
        eng.close()
    doc = {"what": "phy_geo_eval_summaries beside phy_geo_eval (host clock around the synchronous call through the "
                   "Python binding, median of 5 windows of >= 0.5 s, fastest and slowest window beside it)",
           "tool": "tools/geo_latency.py --summaries", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--summaries", action="store_true",
                    help="time phy_geo_eval_summaries beside phy_geo_eval (profiles/geo_summaries_latency.json)")
    arg = ap.parse_args()
    if arg.out is None:
        arg.out = os.path.join(ROOT, "profiles", "geo_summaries_latency.json" if arg.summaries else "geo_latency.json")
    if arg.summaries:
        return summaries(arg)
    peel, blens1 = flu_tree()
    rows = []
    for S, K in SHAPES:
        rng = np.random.default_rng(1000 + K)
        tips = np.zeros((S, K))
        tips[np.arange(S), rng.integers(0, K, S)] = 1.0
        R = geo.rate_count(K)
        params = np.concatenate([0.1 + rng.exponential(1.0, (100, R)), rng.dirichlet(np.ones(K) * 3.0, 100)], axis=1)
        blens = np.tile(blens1, (100, 1))
        host = windows(lambda: geo.geo_gradients_host(tips, peel, blens1, params[0, :R], params[0, R:]), 0.3, 3)
        eng = geo.GeoLikelihood(tips, peel, max_draws=100, device=arg.device)
        info = eng.info()
        for n in DRAWS:
            med, lo, hi, reps = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]))
            sw = eng.sweeps(n)
            row = {"S": S, "K": K, "draws": n, "call_us": med * 1e6, "call_us_min": lo * 1e6, "call_us_max": hi * 1e6,
                   "us_per_draw": med * 1e6 / n, "reps_per_window": reps, "host_us_per_draw": host[0] * 1e6,
                   "host_us_for_n": host[0] * 1e6 * n, "speedup_over_host": host[0] * n / med,
                   "jacobi_sweeps_min": int(sw.min()), "jacobi_sweeps_max": int(sw.max()), **info}
            rows.append(row)
            print("S %d K %2d n %3d: call %9.1f us (%.1f..%.1f), host x n %10.1f us, speedup %6.2f, sweeps %d..%d"
                  % (S, K, n, row["call_us"], row["call_us_min"], row["call_us_max"], row["host_us_for_n"],
                     row["speedup_over_host"], sw.min(), sw.max()), flush=True)
        eng.close()
    doc = {"what": "phy_geo_eval latency (host clock around the synchronous call, median of 5 windows of >= 0.5 s) "
                   "against geo_gradients_host on one thread of the same box",
           "tool": "tools/geo_latency.py", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
