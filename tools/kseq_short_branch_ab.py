"""The K-state engine before and after the short-branch form of its messages
(msg = x + (P - I) x through expm1), the parent commit's library against this
commit's in alternation: parent, this, parent, this, parent, this, one fresh
child process each in one visit (``PHYLO_HIP_LIB`` / ``PHYLO_HIP_AB=1`` select
the parent's library).  Each child times, as tools/kseq_latency.py and
tools/kseq_mix_latency.py do (median of five 0.5 s windows), at the fluA codon
shape (S = 69 rooted, P = 242, K = 61):

* ``phy_kseq_eval`` at C = 4, 1 and 32 draws;
* ``phy_kseq_mix_eval`` at M = 3, C = 1 (the M2a site model), 1 and 32 draws.

The margin is the parent's own run-to-run spread in that visit.  Writes
profiles/kseq_short_branch_ab.json (or --out).

    python tools/kseq_short_branch_ab.py --parent-lib variants/libphylo_parent.so [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.kseq_mix_plain_ab import run_child, summarise  # noqa: E402

DRAWS = [1, 32]


def child(window):
    import numpy as np

    from phylostan_amd import kseq
    from tools.geo_latency import windows
    from tools.kseq_latency import draws, rooted_flu
    from tools.kseq_mix_latency import K, P, S, mix_draws
    peel, blens1 = rooted_flu()
    rng = np.random.default_rng(2061)
    states = rng.integers(0, K, (S, P))
    main_state = rng.integers(0, K, P)
    states = np.where(rng.random((S, P)) < 0.7, main_state[None, :], states)
    masks = kseq.onehot_masks(states).astype(np.uint64)
    w = rng.integers(1, 5, P).astype(float)
    nmax = max(DRAWS)
    blens = np.tile(blens1, (nmax, 1)) * rng.uniform(0.8, 1.2, (nmax, 1))
    out = {}
    params = draws(K, nmax, rng)  # C = 4
    eng = kseq.DeviceKStateLikelihood(masks, w, peel, True, K, 4, max_draws=nmax)
    for n in DRAWS:
        out["kseq_C4_n%d" % n] = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), window)[0] * 1e6
    eng.close()
    mparams, _ = mix_draws(3, 1, nmax, np.random.default_rng(3013))
    mix = kseq.DeviceKStateMixLikelihood(masks, w, peel, True, K, 3, 1, max_draws=nmax)
    for n in DRAWS:
        out["mix_M3_C1_n%d" % n] = windows(lambda: mix.evaluate_rows(blens[:n], mparams[:n]), window)[0] * 1e6
    mix.close()
    print("AB_RESULT " + json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kseq_short_branch_ab.json"))
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--child", action="store_true")
    arg = ap.parse_args()
    if arg.child:
        return child(arg.window)
    if not arg.parent_lib or not os.path.exists(arg.parent_lib):
        raise SystemExit("--parent-lib: the parent commit's libphylo_hip.so is needed")
    sides = {"parent": dict(os.environ, PHYLO_HIP_LIB=os.path.abspath(arg.parent_lib), PHYLO_HIP_AB="1"),
             "this": {k: v for k, v in os.environ.items() if k not in ("PHYLO_HIP_LIB", "PHYLO_HIP_AB")}}
    runs = {"parent": [], "this": []}
    for rep in range(3):
        for side in ("parent", "this"):
            runs[side].append(run_child(sides[side], ["tools/kseq_short_branch_ab.py", "--child", "--window",
                                                      str(arg.window)], "AB_RESULT ", 240))
            print(side, rep, {k: round(v, 1) for k, v in runs[side][-1].items()}, flush=True)
    out = {"what": "phy_kseq_eval (C = 4) and phy_kseq_mix_eval (M = 3, C = 1) at the fluA codon shape (S = 69, P = 242, "
                   "K = 61), median us per call of five %.1f s windows; the parent commit's library and this commit's "
                   "in alternation (parent, this, parent, this, parent, this), one process each in one GPU visit"
                   % arg.window,
           "tool": "tools/kseq_short_branch_ab.py", "eval": summarise(runs["parent"], runs["this"])}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(out, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
