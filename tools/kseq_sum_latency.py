"""Latency of the K-state engine's posterior summaries: ``phy_kseq_sum_add`` at
the fluA codon shape (S = 69 rooted, P = 242 patterns, K = 61) with the two
codon labellings (synonymous, nonsynonymous), for (M, C) = (1, 4) and (3, 1), at
1 and 32 draws, each against

* ``phy_kseq_mix_eval`` on the same draws in the same visit: one way down
  without the extras, the honest yardstick;
* ``phy_kseq_sum_eval`` with and without node_post coming back to the host;
* ``kseq_sum_host`` on one thread, one draw.

The method is tools/kseq_latency.py's: 3 warm-up calls, then repetitions that
fill at least 0.5 s (host clock around the synchronous call), five such
windows, the median reported with the fastest and slowest.  The alignment and
the draws are tools/kseq_mix_latency.py's.  Writes
profiles/kseq_sum_latency.json (or --out).

    python tools/kseq_sum_latency.py [--out FILE] [--device N] [--window S] [--no-host]
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
from tools.geo_latency import windows  # noqa: E402
from tools.kseq_latency import rooted_flu  # noqa: E402
from tools.kseq_mix_latency import K, P, S, mix_draws  # noqa: E402

SHAPES = [(1, 4), (3, 1)]
DRAWS = [1, 32]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq_sum_latency.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread kseq_sum_host yardstick")
    arg = ap.parse_args()
    peel, blens1 = rooted_flu()
    rng = np.random.default_rng(2061)
    states = rng.integers(0, K, (S, P))
    main_state = rng.integers(0, K, P)
    states = np.where(rng.random((S, P)) < 0.7, main_state[None, :], states)
    masks = kseq.onehot_masks(states).astype(np.uint64)
    w = rng.integers(1, 5, P).astype(float)
    nmax = max(DRAWS)
    blens = np.tile(blens1, (nmax, 1)) * rng.uniform(0.8, 1.2, (nmax, 1))
    labels = codon.codon_labels()
    rows = []
    for M, C in SHAPES:
        params, _ = mix_draws(M, C, nmax, np.random.default_rng(3000 + 10 * C + M))
        mix = kseq.DeviceKStateMixLikelihood(masks, w, peel, True, K, M, C, max_draws=nmax, device=arg.device)
        summ = kseq.DeviceKStateSummaries(masks, w, peel, True, K, M, C, labels, max_draws=nmax, device=arg.device)
        host = None
        if not arg.no_host:
            host = windows(lambda: kseq.kseq_sum_host(masks, w, peel, True, blens[:1], params[:1], K, M, C, labels),
                           arg.window, 3, long_call=0.3)
            ref = kseq.kseq_sum_host(masks, w, peel, True, blens[:1], params[:1], K, M, C, labels)
            got = summ.evaluate(blens[:1], params[:1])
            agree = {"counts_rel_diff_to_host": float(np.max(np.abs(got[1] - ref[1])) / np.max(np.abs(ref[1]))),
                     "node_post_abs_diff_to_host": float(np.max(np.abs(got[2] - ref[2])))}
        info = mix.info(0)
        for n in DRAWS:
            base = windows(lambda: mix.evaluate_rows(blens[:n], params[:n]), arg.window)
            summ.reset()
            add = windows(lambda: summ.add(blens[:n], params[:n]), arg.window)
            counts = windows(lambda: summ.evaluate(blens[:n], params[:n], node_post=False), arg.window)
            full = windows(lambda: summ.evaluate(blens[:n], params[:n]), arg.window)
            row = {"S": S, "P": P, "K": K, "M": M, "C": C, "labels": 2, "draws": n, "add_us": add[0] * 1e6,
                   "add_us_min": add[1] * 1e6, "add_us_max": add[2] * 1e6, "reps_per_window": add[3],
                   "mix_eval_us": base[0] * 1e6, "mix_eval_us_min": base[1] * 1e6, "mix_eval_us_max": base[2] * 1e6,
                   "add_over_mix_eval": add[0] / base[0], "eval_counts_only_us": counts[0] * 1e6,
                   "eval_with_node_post_us": full[0] * 1e6, "node_post_bytes_per_draw": (S - 1) * K * P * 8,
                   "items_per_draw": info["items_per_draw"], "chunk_draws": info["chunk_draws"],
                   "workgroups": info["workgroups"]}
            if host is not None:
                row.update(host_one_draw_us=host[0] * 1e6, host_over_device_per_draw=host[0] * n / add[0], **agree)
            rows.append(row)
            print("M %d C %d n %2d: add %9.1f us (%.1f..%.1f) = %.2f x mix_eval %9.1f us; counts only %9.1f us; with "
                  "node_post %9.1f us%s" % (M, C, n, row["add_us"], row["add_us_min"], row["add_us_max"],
                                            row["add_over_mix_eval"], row["mix_eval_us"], row["eval_counts_only_us"],
                                            row["eval_with_node_post_us"],
                                            "" if host is None else "; host x n %.0f us" % (host[0] * n * 1e6)),
                  flush=True)
        mix.close()
        summ.close()
    out = {"tool": "tools/kseq_sum_latency.py", "clock": "host perf_counter around the synchronous call",
           "window_seconds": arg.window, "windows": 5, "host": "kseq_sum_host, numpy, one thread", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
