"""Latency of the partitioned call (phy_part_eval, one launch for K partitions
x n draws) against the same work on K single-alignment contexts, on one
MI355X.

Shapes: fluA (tests/golden/examples/fluA, 69 taxa, 987 sites) split by codon
position, K = 2 (positions 1+2 | 3: 119 / 137 patterns) and K = 3 (65 / 60 /
137 patterns); HKY, C = 4, rooted; calls of 1, 4 and 100 draws.  Baselines,
both the engine as it was:
  (a) K ``TreeLikelihood`` contexts set up as the CLI sets them (compact rows,
      ``prefer_latency_engine()`` where max_draws * C <= 256), ``evaluate_rows``
      one after another at the scaled lengths;
  (b) the same contexts, ``submit_rows`` on all, then ``wait_rows`` on all
      (phy_eval_submit / phy_eval_wait: the only way to overlap them today).
Neither baseline forms mu_k t or folds the rows: that host work is left out of
their time.  Timing as tools/forest_latency.py: host clock around the
synchronous calls, median of 5 windows of >= 0.5 s, fastest and slowest window
beside it.

    python tools/part_latency.py [--out profiles/part_latency.json] [--window 0.5]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

from phylostan_amd import data as dataio, models, partition as pt  # noqa: E402
from phylostan_amd.engine import TreeLikelihood  # noqa: E402
from tools.forest_latency import windows  # noqa: E402

DRAWS = [1, 4, 100]
SCHEMES = {2: [("pos12", (0, 1)), ("pos3", (2,))], 3: [("pos1", (0,)), ("pos2", (1,)), ("pos3", (2,))]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "part_latency.json"))
    ap.add_argument("--window", type=float, default=0.5)
    arg = ap.parse_args()
    base = os.path.join(ROOT, "tests", "golden", "examples", "fluA")
    d = dataio.load(os.path.join(base, "fluA.tree"), os.path.join(base, "fluA.fa"), rooted=True)
    chars = dataio.alignment_matrix(dataio.read_alignment(os.path.join(base, "fluA.fa")), d.tree.taxon_namespace)
    C, model = 4, "HKY"
    rows = []
    for K, scheme in SCHEMES.items():
        parts = [pt.Partition(name, np.sort(np.concatenate([np.arange(p, chars.shape[1], 3) for p in pos])))
                 for name, pos in scheme]
        split = [(tip, w) for tip, w, _ in pt.split_alignment(chars, parts)]
        rng = np.random.default_rng(1)
        for n in DRAWS:
            bl = rng.uniform(0.001, 0.05, (n, d.B))
            mu = rng.uniform(0.5, 1.5, (n, K))
            mv = np.empty((n, K, 10 + 2 * C))
            for i in range(n):
                for k in range(K):
                    rs, ps = models.weibull_site_rates(rng.uniform(0.4, 1.2), C)
                    mv[i, k] = models.model_vector(rng.dirichlet(np.full(4, 8.0)),
                                                   models.hky_exchangeabilities(rng.uniform(2.0, 8.0)), rs, ps)
            part = pt.PartitionedLikelihood(split, d.peel0, True, model, C, max_draws=n)
            singles = []
            for tip, w in split:
                lk = TreeLikelihood(tip, w, d.peel0, True, model, C, max_draws=n)
                lk.set_output(compact=True)
                if n * C <= 256:
                    lk.prefer_latency_engine()
                singles.append(lk)
            scaled = [np.ascontiguousarray(mu[:, k:k + 1] * bl) for k in range(K)]
            mvk = [np.ascontiguousarray(mv[:, k]) for k in range(K)]
            _, ref = part.evaluate_rows(bl, mu, mv, part_rows=True)
            for k in range(K):  # the three ways compute the same rows
                got = singles[k].evaluate_rows(scaled[k], mvk[k])[:, :part.rowlen]
                err = np.max(np.abs(got - ref[:, k])) / np.max(np.abs(ref[:, k]))
                assert err < 1e-9, (K, n, k, err)

            def serial():
                for lk, b, m in zip(singles, scaled, mvk):
                    lk.evaluate_rows(b, m)

            def overlapped():
                for lk, b, m in zip(singles, scaled, mvk):
                    lk.submit_rows(b, m)
                for lk in singles:
                    lk.wait_rows()

            f = windows(lambda: part.evaluate_rows(bl, mu, mv), arg.window)
            a = windows(serial, arg.window)
            b = windows(overlapped, arg.window) if n <= 128 else None
            row = {"shape": "fluA codon positions", "partitions": K, "patterns": [int(t.shape[1]) for t, _ in split],
                   "draws": n, "plan": part.info(),
                   "partition_us": f[0] * 1e6, "partition_us_min": f[1] * 1e6, "partition_us_max": f[2] * 1e6,
                   "partition_reps_per_window": f[3],
                   "serial_contexts_us": a[0] * 1e6, "serial_contexts_us_min": a[1] * 1e6,
                   "serial_contexts_us_max": a[2] * 1e6, "serial_over_partition": a[0] / f[0]}
            if b:
                row.update({"overlapped_contexts_us": b[0] * 1e6, "overlapped_contexts_us_min": b[1] * 1e6,
                            "overlapped_contexts_us_max": b[2] * 1e6, "overlapped_over_partition": b[0] / f[0]})
            rows.append(row)
            print(json.dumps(row), flush=True)
            part.close()
            for lk in singles:
                lk.close()
    doc = {"what": "phy_part_eval (one call, K partitions x n draws) against K single-alignment contexts evaluated one "
                   "after another (serial_contexts) and submitted together then collected (overlapped_contexts); host "
                   "clock around the synchronous calls through the Python bindings, median of 5 windows of >= %g s"
                   % arg.window,
           "rows": rows}
    os.makedirs(os.path.dirname(arg.out), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
        fp.write("\n")


if __name__ == "__main__":
    main()
