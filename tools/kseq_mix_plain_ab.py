"""The existing paths against the parent commit's library, alternated in one
visit: ``phy_kseq_eval`` at the six shapes of profiles/kseq_latency.json (fluA's
tree, P = 242, C = 4, K in {20, 61}, 1 / 4 / 32 draws) and ``bench.py``'s fluA
headline, parent, this, parent, this, parent, this, one fresh child process
each (``PHYLO_HIP_LIB`` / ``PHYLO_HIP_AB=1`` select the parent's library).  The
margin is the parent's own run-to-run spread measured in that visit.  Writes
profiles/kseq_mix_plain_ab.json (or --out).

    python tools/kseq_mix_plain_ab.py --parent-lib variants/libphylo_parent.so [--out FILE] [--no-bench]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BENCH = ["bench.py", "--gpus", "1", "--steps", "200", "--warmup", "20", "--no-synthetic", "--no-cpu-baseline",
         "--no-sampler-latency", "--no-multidev"]


def child(window):
    """One process, one library: median seconds per call of the six shapes, as tools/kseq_latency.py times them."""
    import numpy as np

    from phylostan_amd import kseq
    from tools.geo_latency import windows
    from tools.kseq_latency import C, DRAWS, KS, P, S, draws, rooted_flu
    peel, blens1 = rooted_flu()
    out = {}
    for K in KS:
        rng = np.random.default_rng(2000 + K)
        states = rng.integers(0, K, (S, P))
        main_state = rng.integers(0, K, P)
        states = np.where(rng.random((S, P)) < 0.7, main_state[None, :], states)
        masks = kseq.onehot_masks(states).astype(np.uint64)
        w = rng.integers(1, 5, P).astype(float)
        params = draws(K, max(DRAWS), rng)
        blens = np.tile(blens1, (max(DRAWS), 1)) * rng.uniform(0.8, 1.2, (max(DRAWS), 1))
        eng = kseq.DeviceKStateLikelihood(masks, w, peel, True, K, C, max_draws=max(DRAWS))
        for n in DRAWS:
            out["K%d_n%d" % (K, n)] = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), window)[0] * 1e6
        eng.close()
    print("AB_RESULT " + json.dumps(out), flush=True)


def run_child(env, cmd, marker, limit, strip=True):
    run = subprocess.run([sys.executable] + cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=limit)
    if run.returncode != 0:
        raise SystemExit("child failed (%d): %s" % (run.returncode, (run.stdout + run.stderr)[-2000:]))
    line = [ln for ln in run.stdout.splitlines() if ln.startswith(marker)][-1]
    return json.loads(line[len(marker):] if strip else line)


def summarise(parent, this):
    """Per key: the three figures of each side, the parent's spread, and whether this side's median is slower
    than the parent's slowest by more than that spread (times: larger is slower)."""
    out = {}
    for k in parent[0]:
        p, t = sorted(r[k] for r in parent), sorted(r[k] for r in this)
        spread = p[-1] - p[0]
        out[k] = {"parent_us": p, "this_us": t, "parent_spread_us": spread, "this_median_over_parent_median": t[1] / p[1],
                  "slower_beyond_spread": bool(t[1] > p[-1] + spread)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq_mix_plain_ab.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--no-bench", action="store_true")
    ap.add_argument("--child", action="store_true")
    arg = ap.parse_args()
    if arg.child:
        return child(arg.window)
    if not arg.parent_lib or not os.path.exists(arg.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libphylo_hip.so is needed")
    sides = {"parent": dict(os.environ, PHYLO_HIP_LIB=os.path.abspath(arg.parent_lib), PHYLO_HIP_AB="1"),
             "this": {k: v for k, v in os.environ.items() if k not in ("PHYLO_HIP_LIB", "PHYLO_HIP_AB")}}
    kseq_runs = {"parent": [], "this": []}
    bench_runs = {"parent": [], "this": []}
    for rep in range(3):
        for side in ("parent", "this"):
            kseq_runs[side].append(run_child(sides[side], ["tools/kseq_mix_plain_ab.py", "--child", "--window",
                                                           str(arg.window)], "AB_RESULT ", 240))
            print(side, rep, "kseq", {k: round(v, 1) for k, v in kseq_runs[side][-1].items()}, flush=True)
            if not arg.no_bench:
                res = run_child(sides[side], BENCH, "{", 300, strip=False)
                bench_runs[side].append(res)
                print(side, rep, "bench", res.get("value"), res.get("unit"), flush=True)
    out = {"what": "phy_kseq_eval (median us per call of five 0.5 s windows) and bench.py's fluA headline, the parent "
                   "commit's library and this commit's in alternation (parent, this, parent, this, parent, this), one "
                   "process each in one GPU visit",
           "kseq_eval": summarise(kseq_runs["parent"], kseq_runs["this"])}
    if not arg.no_bench:
        key = "value" if "value" in bench_runs["parent"][0] else sorted(bench_runs["parent"][0])[0]
        p = sorted(float(r[key]) for r in bench_runs["parent"])
        t = sorted(float(r[key]) for r in bench_runs["this"])
        out["bench"] = {"command": "python " + " ".join(BENCH), "key": key, "unit": bench_runs["parent"][0].get("unit"),
                        "parent": p, "this": t, "parent_spread_max_minus_min": p[-1] - p[0],
                        "this_median_over_parent_median": t[1] / p[1],
                        "condition": "this_median >= parent_lowest - parent_spread",
                        "holds": bool(t[1] >= p[0] - (p[-1] - p[0]))}
    with open(arg.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
