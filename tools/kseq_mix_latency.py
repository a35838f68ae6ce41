"""Latency of the K-state mixture engine: ``phy_kseq_mix_eval`` at the fluA codon
shape (S = 69 rooted, P = 242 patterns, K = 61) for C in {1, 4}, M in {1, 2, 3}
and 1, 4 and 32 draws, each against

* M = 1 of the same build and shape;
* M sequential ``phy_kseq_eval`` calls of the same draws, one per component with
  its own rates -- the only emulation of the work, though it does not yield the
  mixture's number (no shared shifts, M rows of the wrong function);
* ``kseq_mix_host`` on one thread, one draw.

The method is tools/kseq_latency.py's: 3 warm-up calls, then repetitions that
fill at least 0.5 s (host clock around the synchronous call), five such
windows, the median reported with the fastest and slowest.  The alignment is
that tool's: random codons, many of them three changes apart, where an eigen
route holds L_i absolutely and not relatively, so ``loglik_rel_diff_to_host`` is
a sanity figure here and no accuracy bar (the tests pin accuracy).  Writes
profiles/kseq_mix_latency.json (or --out).

    python tools/kseq_mix_latency.py [--out FILE] [--device N] [--window S] [--no-host]
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

S, P, K = 69, 242, 61
CS = [1, 4]
MS = [1, 2, 3]
DRAWS = [1, 4, 32]


def mix_draws(M, C, n, rng):
    """Codon site-model draws as ``CodonSitesPosterior`` forms them: shared kappa and pi, omegas ascending."""
    kappa = rng.uniform(2.0, 8.0, n)
    x6 = np.stack([np.ones(n), kappa, np.ones(n), np.ones(n), kappa, np.ones(n)], axis=1)
    om = np.sort(rng.uniform(0.05, 2.5, (n, M)), axis=1)
    rates = np.stack([codon.codon_rates(x6, om[:, m]) for m in range(M)], axis=1)
    pi = rng.dirichlet(np.ones(K) * 3.0, n)
    p = rng.dirichlet(np.ones(M) * 4.0, n)
    r = np.sort(rng.exponential(1.0, (n, C)), axis=1)
    q = rng.dirichlet(np.ones(C) * 4.0, n)
    ratio = codon.class_scale(rates, pi, p)
    rs = (ratio[:, :, None] * r[:, None, :]).reshape(n, -1)
    ps = (p[:, :, None] * q[:, None, :]).reshape(n, -1)
    comps = np.concatenate([rates, np.repeat(pi[:, None, :], M, axis=1)], axis=2).reshape(n, -1)
    singles = [np.concatenate([rates[:, m], pi, ratio[:, m:m + 1] * r, q], axis=1) for m in range(M)]
    return np.concatenate([comps, rs, ps], axis=1), singles


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq_mix_latency.json"))
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-host", action="store_true", help="skip the one-thread kseq_mix_host yardstick")
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
    rows = []
    for C in CS:
        one = kseq.DeviceKStateLikelihood(masks, w, peel, True, K, C, max_draws=nmax, device=arg.device)
        base = {}
        for M in MS:
            params, singles = mix_draws(M, C, nmax, np.random.default_rng(3000 + 10 * C + M))
            eng = kseq.DeviceKStateMixLikelihood(masks, w, peel, True, K, M, C, max_draws=nmax, device=arg.device)
            host = None
            if not arg.no_host:
                host = windows(lambda: kseq.kseq_mix_host(masks, w, peel, True, blens[:1], params[:1], K, M, C),
                               arg.window, 3, long_call=0.3)
                ref = kseq.kseq_mix_host(masks, w, peel, True, blens[:1], params[:1], K, M, C)[0]
                got = eng.evaluate_rows(blens[:1], params[:1])
                agree = float(abs(got[0, 0] - ref[0, 0]) / abs(ref[0, 0]))
            for n in DRAWS:
                dev = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), arg.window)
                seq = windows(lambda: [one.evaluate_rows(blens[:n], s[:n]) for s in singles], arg.window)
                info = eng.info(n)
                if M == 1:
                    base[n] = dev[0]
                row = {"S": S, "P": P, "K": K, "C": C, "M": M, "draws": n, "eval_us": dev[0] * 1e6,
                       "eval_us_min": dev[1] * 1e6, "eval_us_max": dev[2] * 1e6, "reps_per_window": dev[3],
                       "over_M1": dev[0] / base[n], "sequential_kseq_eval_us": seq[0] * 1e6,
                       "sequential_over_mix": seq[0] / dev[0],
                       "sweeps_max": max(max(r) for r in info["sweeps"]), "items_per_draw": info["items_per_draw"],
                       "chunk_draws": info["chunk_draws"], "workgroups": info["workgroups"],
                       "workspace_bytes": info["workspace_bytes"]}
                if host is not None:
                    row.update(host_one_draw_us=host[0] * 1e6, host_over_device_per_draw=host[0] * n / dev[0],
                               loglik_rel_diff_to_host=agree)
                rows.append(row)
                print("C %d M %d n %2d: mix %9.1f us (%.1f..%.1f) = %.2f x M1; %d sequential calls %9.1f us (x %.2f)%s"
                      % (C, M, n, row["eval_us"], row["eval_us_min"], row["eval_us_max"], row["over_M1"], M,
                         row["sequential_kseq_eval_us"], row["sequential_over_mix"],
                         "" if host is None else "; host x n %.0f us" % (host[0] * n * 1e6)), flush=True)
            eng.close()
        one.close()
    out = {"tool": "tools/kseq_mix_latency.py", "clock": "host perf_counter around the synchronous phy_kseq_mix_eval",
           "window_seconds": arg.window, "windows": 5, "host": "kseq_mix_host, numpy, one thread", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
