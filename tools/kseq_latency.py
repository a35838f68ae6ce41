"""Latency of the K-state sequence engine: ``phy_kseq_eval`` at S = 69 (fluA's
tree, rooted), P = 242 patterns, C = 4, K in {20, 61}, 1, 4 and 32 draws, beside
the one-thread time of ``kseq_host`` (numpy, LAPACK's eigh) on the same box --
the yardstick: the one-draw call at K = 61 should beat one host evaluation.

Each shape is warmed up (3 calls), then timed over repetitions that fill at
least 0.5 s (host clock around the synchronous call), five such windows, the
median window reported with the fastest and slowest.  The Jacobi sweeps of the
timed draws are read back.  The share of a call spent in ``kseq_eig_kernel`` is
bounded from above without a profiler: the same draws through a context on a
3-tip, 1-pattern, 1-category tree of the same K, whose call is the eigensolve
plus four nearly empty launches and the copies ("eig_call_us").  Writes
profiles/kseq_latency.json (or --out).

    python tools/kseq_latency.py [--out FILE] [--device N] [--window S]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):  # the host yardstick is one thread
    os.environ[_v] = "1"

import numpy as np  # noqa: E402

from phylostan_amd import codon, kseq  # noqa: E402
from tools.geo_latency import flu_tree, windows  # noqa: E402

S, P, C = 69, 242, 4
KS = [20, 61]
DRAWS = [1, 4, 32]


def rooted_flu():
    """fluA's topology as a rooted peel: the unrooted peel's last row joins two subtrees under the root, and node
    2S-3 gets a branch of its own."""
    peel, bl = flu_tree()
    return peel, np.concatenate([bl, [bl.mean()]])


def draws(K, n, rng):
    R = kseq.rate_count(K)
    if K == 61:  # the codon structure of zeros: kappa and omega vary by draw
        rates = np.stack([codon.codon_rates(np.asarray([1.0, k, 1.0, 1.0, k, 1.0]), w)
                          for k, w in zip(rng.uniform(2.0, 8.0, n), rng.uniform(0.05, 0.8, n))])
    else:
        rates = 0.1 + rng.exponential(1.0, (n, R))
    freqs = rng.dirichlet(np.ones(K) * 3.0, n)
    rs = np.sort(rng.exponential(1.0, (n, C)), axis=1)
    ps = rng.dirichlet(np.ones(C) * 4.0, n)
    return np.concatenate([rates, freqs, rs, ps], axis=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq_latency.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--window", type=float, default=0.5)
    arg = ap.parse_args()
    peel, blens1 = rooted_flu()
    tiny_peel = np.asarray([[0, 1, 3], [2, 3, 4]], np.int32)
    rows = []
    for K in KS:
        rng = np.random.default_rng(2000 + K)
        states = rng.integers(0, K, (S, P))
        main_state = rng.integers(0, K, P)
        states = np.where(rng.random((S, P)) < 0.7, main_state[None, :], states)
        masks = kseq.onehot_masks(states).astype(np.uint64)
        w = rng.integers(1, 5, P).astype(float)
        params = draws(K, max(DRAWS), rng)
        blens = np.tile(blens1, (max(DRAWS), 1)) * rng.uniform(0.8, 1.2, (max(DRAWS), 1))
        eng = kseq.DeviceKStateLikelihood(masks, w, peel, True, K, C, max_draws=max(DRAWS), device=arg.device)
        tiny = kseq.DeviceKStateLikelihood(masks[:3, :1], np.ones(1), tiny_peel, False, K, 1, max_draws=max(DRAWS),
                                           device=arg.device)
        tiny_params = np.concatenate([params[:, :kseq.rate_count(K) + K], np.ones((max(DRAWS), 2))], axis=1)
        host = windows(lambda: kseq.kseq_host(masks, w, peel, True, blens[:1], params[:1], C), arg.window, 3,
                       long_call=0.5)
        ref = kseq.kseq_host(masks, w, peel, True, blens[:1], params[:1], C)[0]
        got = eng.evaluate_rows(blens[:1], params[:1])
        agree = float(np.max(np.abs(got - ref)) / np.max(np.abs(ref)))
        for n in DRAWS:
            dev = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), arg.window)
            info = eng.info(n)
            eig = windows(lambda: tiny.evaluate_rows(np.full((n, 3), 0.1), tiny_params[:n]), arg.window)
            row = {"S": S, "P": P, "C": C, "K": K, "draws": n, "eval_us": dev[0] * 1e6, "eval_us_min": dev[1] * 1e6,
                   "eval_us_max": dev[2] * 1e6, "reps_per_window": dev[3], "host_one_draw_us": host[0] * 1e6,
                   "host_over_device_per_draw": host[0] * n / dev[0], "eig_call_us": eig[0] * 1e6,
                   "eig_share_upper_bound": eig[0] / dev[0], "sweeps": info.pop("sweeps"),
                   "row_rel_diff_to_host": agree, **info}
            rows.append(row)
            print("K %2d n %2d: eval %9.1f us (%.1f..%.1f), host x n %10.1f us (x %.2f), eigen call %8.1f us (%.0f%%), "
                  "sweeps %s" % (K, n, row["eval_us"], row["eval_us_min"], row["eval_us_max"], host[0] * n * 1e6,
                                 row["host_over_device_per_draw"], row["eig_call_us"],
                                 100 * row["eig_share_upper_bound"], sorted(set(row["sweeps"]))), flush=True)
        eng.close()
        tiny.close()
    out = {"tool": "tools/kseq_latency.py", "clock": "host perf_counter around the synchronous phy_kseq_eval",
           "window_seconds": arg.window, "windows": 5, "host": "kseq_host, numpy, one thread", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
