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

``--trees`` times the tree-sample engine, ``phy_geo_trees_eval``, at K in {5,
20, 64} x T in {1, 64, 1024} x draws in {1, 4, 100} on fluA's tree with T
seeded branch-length vectors (the same clock and windows, one process), and
writes profiles/geo_trees_latency.json.  The yardstick of each shape is the
only way to get the number without it, on the same device: ``phy_geo_eval`` on
draws x T rows (one parameter point per draw, the T branch-length vectors) in
chunks of its context's max_draws, then the host log-sum-exp and the
posterior-weighted sum of the gradient blocks.  A yardstick call of more than
0.5 s is timed once per window over 3 windows after one warm-up call.  One
more row: 42 seeded random topologies on 27 tips at K = 5 against
``geo_trees_host`` on one thread.

``--trees --clock`` times ``phy_geo_trees_eval_clock`` (a trait clock rate per
draw) beside ``phy_geo_trees_eval`` on the same context at the same 27 shapes,
the two calls' windows interleaved, and writes
profiles/geo_trees_clock_latency.json: both latencies and their ratio, and a
digest of the plain call's rows.  A library without the clock entry points (an
older build under ``PHYLO_HIP_LIB`` with ``PHYLO_HIP_AB=1``) is timed on the
plain call alone: two builds run in alternation give the plain call's noise and
whether a change moved it; the digests say whether its rows are the same bits.

``--digest`` times nothing: it prints and writes (profiles/geo_digest.json) a
sha1 of every array returned by the six evaluation calls of both engines on
small inputs that reach every arm -- K in {2, 3, 5, 33, 64}, S in {3, 7, 69}, T
in {1, 3, more trees than resident groups}, a refused draw, tied eigenvalues, a
zero branch, a missing tip, two 600-tip trees that rescale, a tree term that
underflows -- so that two builds can be told to compute the same bits.

    python tools/geo_latency.py [--summaries | --trees [--clock] | --digest] [--out FILE] [--device N]
        [--window S] [--plain-only]
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


def windows(fn, min_seconds=0.5, n_windows=5, long_call=None):
    """Seconds per call: median, fastest and slowest of n_windows windows.
    ``long_call``: a first call of more than that many seconds is its only
    warm-up, and 3 windows of one call each are timed."""
    t0 = time.perf_counter()
    fn()
    first = time.perf_counter() - t0
    if long_call is not None and first > long_call:
        out = []
        for _ in range(3):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)
        out.sort()
        return out[1], out[0], out[-1], 1
    for _ in range(2):
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
            plain = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), arg.window)
            summ = windows(lambda: eng.evaluate_summaries(blens[:n], params[:n]), arg.window)
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
                   "Python binding, median of 5 windows of >= %g s, fastest and slowest window beside it)" % arg.window,
           "tool": "tools/geo_latency.py --summaries", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


TREES_K = [5, 20, 64]
TREES_T = [1, 64, 1024]
YARD_MAX_DRAWS = 128  # GeoLikelihood's default


def emulate(one, blens, params, logw):
    """The mixture rows of ``params [n, R + K]`` over the T branch-length
    vectors ``blens`` from the single-tree engine: n x T rows of phy_geo_eval in
    chunks of its max_draws, then log-sum-exp and the posterior-weighted sum of
    the gradient blocks on the host."""
    n, T, B = params.shape[0], blens.shape[0], blens.shape[1]
    m = np.full(n, -np.inf)
    z = np.zeros(n)
    acc = np.zeros((n, params.shape[1]))
    for at in range(0, n * T, YARD_MAX_DRAWS):  # row r is draw r // T on tree r % T
        r = np.arange(at, min(at + YARD_MAX_DRAWS, n * T))
        rows = one.evaluate_rows(blens[r % T], params[r // T])
        x = rows[:, 0] + logw[r % T]
        for d in range(r[0] // T, r[-1] // T + 1):  # a running maximum per draw, as the chunks arrive
            sel = r // T == d
            mn = max(m[d], x[sel].max())
            old, w = np.exp(m[d] - mn), np.exp(x[sel] - mn)
            z[d] = z[d] * old + w.sum()
            acc[d] = acc[d] * old + w @ rows[sel, 1 + B:]
            m[d] = mn
    return np.concatenate([(m + np.log(z))[:, None], acc / z[:, None]], axis=1)


def trees(arg):
    peel, blens1 = flu_tree()
    S = peel.shape[0] + 1
    rows = []
    for K in TREES_K:
        rng = np.random.default_rng(1000 + K)
        tips = np.zeros((S, K))
        tips[np.arange(S), rng.integers(0, K, S)] = 1.0
        R = geo.rate_count(K)
        params = np.concatenate([0.1 + rng.exponential(1.0, (100, R)), rng.dirichlet(np.ones(K) * 3.0, 100)], axis=1)
        one = geo.GeoLikelihood(tips, peel, max_draws=YARD_MAX_DRAWS, device=arg.device)
        for T in TREES_T:
            blens = blens1[None, :] * rng.uniform(0.5, 1.5, (T, blens1.size))
            logw = np.full(T, -np.log(T))
            eng = geo.GeoTreesLikelihood(tips, np.broadcast_to(peel, (T,) + peel.shape), blens, max_draws=100,
                                         device=arg.device)
            info = eng.info()
            agree = np.abs(eng.evaluate_rows(params[:2]) - emulate(one, blens, params[:2], logw)).max()
            for n in DRAWS:
                new = windows(lambda: eng.evaluate_rows(params[:n]))
                old = windows(lambda: emulate(one, blens, params[:n], logw), long_call=0.5)
                row = {"S": S, "K": K, "T": T, "draws": n, "trees_us": new[0] * 1e6, "trees_us_min": new[1] * 1e6,
                       "trees_us_max": new[2] * 1e6, "emulated_us": old[0] * 1e6, "emulated_us_min": old[1] * 1e6,
                       "emulated_us_max": old[2] * 1e6, "emulated_reps_per_window": old[3],
                       "trees_over_emulated": new[0] / old[0], "max_abs_difference_of_rows": float(agree), **info}
                rows.append(row)
                print("K %2d T %4d n %3d: trees %10.1f us (%.1f..%.1f), emulated %12.1f us (%.1f..%.1f), ratio %.4f"
                      % (K, T, n, row["trees_us"], row["trees_us_min"], row["trees_us_max"], row["emulated_us"],
                         row["emulated_us_min"], row["emulated_us_max"], row["trees_over_emulated"]), flush=True)
            eng.close()
        one.close()
    # a multi-topology sample: 42 seeded random trees on 27 tips, K = 5, against the host restatement on one thread
    from tests import geo_oracle as go
    S, K, T = 27, 5, 42
    rng = np.random.default_rng(42)
    peels = np.stack([go.random_peel(S, rng) for _ in range(T)])
    tips = go.random_tips(S, K, rng, missing=())
    blens = rng.exponential(0.1, (T, 2 * S - 3))
    _, params = go.random_draws(4, 2 * S - 3, K, rng)
    R = geo.rate_count(K)
    eng = geo.GeoTreesLikelihood(tips, peels, blens, max_draws=4, device=arg.device)
    host = windows(lambda: geo.geo_trees_host(tips, peels, blens, params[0, :R], params[0, R:]), 0.3, 3)
    multi = []
    for n in (1, 4):
        new = windows(lambda: eng.evaluate_rows(params[:n]))
        multi.append({"S": S, "K": K, "T": T, "draws": n, "trees_us": new[0] * 1e6, "trees_us_min": new[1] * 1e6,
                      "trees_us_max": new[2] * 1e6, "host_us_for_n": host[0] * 1e6 * n,
                      "speedup_over_host": host[0] * n / new[0], **eng.info()})
        print("42 topologies, S 27 K 5 n %d: trees %.1f us, host x n %.1f us" % (n, new[0] * 1e6, host[0] * 1e6 * n),
              flush=True)
    eng.close()
    doc = {"what": "phy_geo_trees_eval latency (host clock around the synchronous call through the Python binding, "
                   "median of 5 windows of >= 0.5 s) against phy_geo_eval emulating the same-topology sample on the "
                   "same device (draws x T rows in chunks of %d, host log-sum-exp combine)" % YARD_MAX_DRAWS,
           "tool": "tools/geo_latency.py --trees", "rows": rows, "multi_topology": multi}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


def trees_clock(arg):
    import hashlib
    peel, blens1 = flu_tree()
    S = peel.shape[0] + 1
    rows = []
    for K in TREES_K:
        rng = np.random.default_rng(1000 + K)
        tips = np.zeros((S, K))
        tips[np.arange(S), rng.integers(0, K, S)] = 1.0
        R = geo.rate_count(K)
        params = np.concatenate([0.1 + rng.exponential(1.0, (100, R)), rng.dirichlet(np.ones(K) * 3.0, 100)], axis=1)
        mus = np.exp(rng.normal(0.0, 1.0, 100))  # a different rate per draw
        for T in TREES_T:
            blens = blens1[None, :] * rng.uniform(0.5, 1.5, (T, blens1.size))
            eng = geo.GeoTreesLikelihood(tips, np.broadcast_to(peel, (T,) + peel.shape), blens, max_draws=100,
                                         device=arg.device)
            has_clock = hasattr(eng.lib, "phy_geo_trees_eval_clock") and not arg.plain_only
            info = eng.info()
            for n in DRAWS:
                digest = hashlib.sha1(eng.evaluate_rows(params[:n]).tobytes()).hexdigest()[:16]
                plain = windows(lambda: eng.evaluate_rows(params[:n]), arg.window)
                row = {"S": S, "K": K, "T": T, "draws": n, "plain_us": plain[0] * 1e6, "plain_us_min": plain[1] * 1e6,
                       "plain_us_max": plain[2] * 1e6, "plain_rows_sha1": digest, **info}
                if has_clock:
                    unit = eng.evaluate_rows_clock(params[:n], np.ones(n))[:, :-1]  # mu = 1: the plain rows, bitwise
                    row["unit_rate_rows_are_the_plain_rows"] = hashlib.sha1(unit.tobytes()).hexdigest()[:16] == digest
                    clock = windows(lambda: eng.evaluate_rows_clock(params[:n], mus[:n]), arg.window)
                    again = windows(lambda: eng.evaluate_rows(params[:n]), arg.window)  # the plain call once more
                    row.update({"clock_us": clock[0] * 1e6, "clock_us_min": clock[1] * 1e6, "clock_us_max": clock[2] * 1e6,
                                "plain_again_us": again[0] * 1e6,
                                "clock_over_plain": clock[0] / (0.5 * (plain[0] + again[0]))})
                rows.append(row)
                print("K %2d T %4d n %3d: plain %10.1f us (%.1f..%.1f)%s" % (
                    K, T, n, row["plain_us"], row["plain_us_min"], row["plain_us_max"],
                    ", clock %10.1f us (%.1f..%.1f), plain again %10.1f us, ratio %.4f" % (
                        row["clock_us"], row["clock_us_min"], row["clock_us_max"], row["plain_again_us"],
                        row["clock_over_plain"]) if has_clock else ""), flush=True)
            eng.close()
    doc = {"what": "phy_geo_trees_eval_clock beside phy_geo_trees_eval on the same context (host clock around the "
                   "synchronous call through the Python binding, median of 5 windows of >= %g s; plain, clock, plain "
                   "again; the ratio is clock over the mean of the two plain medians)" % arg.window,
           "tool": "tools/geo_latency.py --trees --clock", "library": os.environ.get("PHYLO_HIP_LIB", "in-tree"),
           "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


DIGEST_K = [2, 3, 5, 33, 64]  # even K, odd K (the Jacobi bye), K > 32, one workgroup per CU
DIGEST_S = [3, 7, 69]          # one schedule row, several levels, fluA's tree


def digest(arg):
    """sha1 of every array the six evaluation calls return, on small inputs
    that reach every arm of the kernels; two builds of the library give the
    same list exactly when they compute the same bits."""
    import hashlib
    from tests import geo_oracle as go
    from tests import geo_trees_truth as gt
    out = []

    def put(case, call, arrays):
        for name, arr in arrays:
            out.append({"case": case, "call": call, "array": name,
                        "sha1": hashlib.sha1(np.ascontiguousarray(arr).tobytes()).hexdigest()})

    def single(case, tips, peel, blens, params):
        eng = geo.GeoLikelihood(tips, peel, max_draws=3, device=arg.device)
        try:
            bl = np.tile(blens, (params.shape[0], 1))
            rows = eng.evaluate_rows(bl, params)
            put(case, "phy_geo_eval", [("rows", rows), ("sweeps", eng.sweeps(params.shape[0]))])
            srows, marg, jumps, bj = eng.evaluate_summaries(bl, params)
            put(case, "phy_geo_eval_summaries", [("rows", srows), ("marg", marg), ("jumps", jumps), ("bjumps", bj)])
            workgroups = eng.info()["workgroups"]
        finally:
            eng.close()
        return srows, marg, jumps, workgroups

    def sample(case, tips, peels, blens, logw, params, mus):
        eng = geo.GeoTreesLikelihood(tips, peels, blens, log_weights=logw, max_draws=3, device=arg.device)
        try:
            rows = eng.evaluate_rows(params)
            put(case, "phy_geo_trees_eval", [("rows", rows), ("tree_ll", eng.tree_loglik)])
            srows, jumps, root = eng.evaluate_summaries(params)
            put(case, "phy_geo_trees_eval_summaries", [("rows", srows), ("tree_ll", eng.tree_loglik), ("jumps", jumps),
                                                       ("root", root)])
            crows = eng.evaluate_rows_clock(params, mus)
            put(case, "phy_geo_trees_eval_clock", [("rows", crows), ("tree_ll", eng.tree_loglik)])
            cs, cj, cr = eng.evaluate_summaries_clock(params, mus)
            put(case, "phy_geo_trees_eval_clock_summaries", [("rows", cs), ("tree_ll", eng.tree_loglik), ("jumps", cj),
                                                             ("root", cr)])
            workgroups = eng.info()["workgroups"]
        finally:
            eng.close()
        return srows, jumps, root, workgroups

    def draws(K, B, rng):
        """Three draws: an ordinary one, all rates and frequencies equal (tied eigenvalues: phi_close), a negative rate."""
        R = geo.rate_count(K)
        _, params = go.random_draws(3, B, K, rng)
        params[1, :R], params[1, R:] = 1.0, 1.0 / K
        params[2, 0] = -1.0
        return params

    flu_peel, flu_blens = flu_tree()
    one_tree = []
    spare = {}  # (K, S) -> the T = resident groups + 1 sample, for the underflow cases below
    for K in DIGEST_K:
        for S in DIGEST_S:
            B = 2 * S - 3
            rng = np.random.default_rng(7000 + 100 * K + S)
            pool = gt.mixed_peels(S, 7, rng)
            if S == flu_peel.shape[0] + 1:
                pool[0] = flu_peel
            tips = go.random_tips(S, K, rng, missing=(0,))  # tip 0 is missing
            pblens = rng.exponential(0.3, (7, B))
            pblens[0, 1] = 0.0  # a zero branch
            params = draws(K, B, rng)
            mus = np.array([0.7, 1.3, 2.0])
            case = "K%d S%d" % (K, S)
            srows, marg, sjumps, _ = single(case, tips, pool[0], pblens[0], params)
            trows, tjumps, troot, W = sample(case + " T1", tips, pool[:1], pblens[:1], None, params, mus)
            R = geo.rate_count(K)
            one_tree.append({"S": S, "K": K,  # T = 1, weight 1, against the single-tree engine, draw by draw
                             "loglik": trows[:, 0].tobytes() == srows[:, 0].tobytes(),
                             "grad_rates": trows[:, 1:1 + R].tobytes() == srows[:, 1 + B:1 + B + R].tobytes(),
                             "grad_freqs": trows[:, 1 + R:].tobytes() == srows[:, 1 + B + R:].tobytes(),
                             "jumps": tjumps.tobytes() == sjumps.tobytes(),
                             "root": troot.tobytes() == np.ascontiguousarray(marg[:, 2 * S - 2]).tobytes(),
                             "max_abs_difference": float(max(np.abs(trows[:2, 1:] - srows[:2, 1 + B:]).max(),
                                                             np.abs(trows[:2, 0] - srows[:2, 0]).max()))})
            logw = np.log(rng.dirichlet(np.ones(3) * 2.0))
            sample(case + " T3", tips, pool[:3], pblens[:3], logw, params, mus)
            T = W + 1  # more trees than resident groups, cycling through the pool with their own weights
            cls = np.arange(T) % 7
            logw = rng.normal(0.0, 3.0, T) - np.log(T)
            sample(case + " T%d" % T, tips, pool[cls], pblens[cls], logw, params, mus)
            spare[K, S] = (tips, pool[cls], pblens[cls], logw, params, mus)
    # two 600-tip trees whose partials leave the fp64 range: the rescaling
    S, K = 600, 8
    rng = np.random.default_rng(600)
    peels = np.stack([go.random_peel(S, rng), go.random_peel(S, rng)])
    tips = go.random_tips(S, K, rng)
    blens = rng.exponential(0.3, (2, 2 * S - 3))
    params = draws(K, 2 * S - 3, rng)
    single("K8 S600", tips, peels[0], blens[0], params)
    sample("K8 S600 T2", tips, peels, blens, None, params, np.array([0.9, 1.1, np.nan]))  # and a refused rate
    # a tree whose weighted term underflows against its group's maximum.  With one tree more than groups the last
    # group alone walks two trees, T - 2 then T - 1 (geo_plan.h: grp_off[g] = g T / G).  "second": tree T - 1 is
    # dominated, exp(x - m) is 0 and the tree skips its reverse pass and adds nothing; "first": tree T - 2 is, and
    # what it left in the slot is rescaled by exp(m_old - m_new) = 0 when tree T - 1 raises the maximum
    for K, S in ((3, 7), (64, 69)):
        tips, peels, blens, logw, params, mus = spare[K, S]
        T = len(logw)
        for name, t in (("second", T - 1), ("first", T - 2)):
            lw = logw.copy()
            lw[t] = -800.0
            sample("K%d S%d T%d underflow %s" % (K, S, T, name), tips, peels, blens, lw, params, mus)
    doc = {"what": "sha1 of every array returned by phy_geo_eval, phy_geo_eval_summaries and the four phy_geo_trees_eval "
                   "calls on small inputs; one_tree: whether a one-tree sample gives the single-tree engine's bits",
           "tool": "tools/geo_latency.py --digest", "library": os.environ.get("PHYLO_HIP_LIB", "in-tree"),
           "digests": out, "one_tree": one_tree}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    whole = hashlib.sha1("".join(d["sha1"] for d in out).encode()).hexdigest()
    print("%d digests, sha1 of them all %s; wrote %s" % (len(out), whole, arg.out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--summaries", action="store_true",
                    help="time phy_geo_eval_summaries beside phy_geo_eval (profiles/geo_summaries_latency.json)")
    ap.add_argument("--trees", action="store_true",
                    help="time phy_geo_trees_eval against phy_geo_eval emulating the sample (profiles/geo_trees_latency.json)")
    ap.add_argument("--clock", action="store_true",
                    help="with --trees: time phy_geo_trees_eval_clock beside phy_geo_trees_eval "
                         "(profiles/geo_trees_clock_latency.json)")
    ap.add_argument("--plain-only", action="store_true",
                    help="--trees --clock: time the plain call alone (one leg of an alternation of two builds)")
    ap.add_argument("--window", type=float, default=0.5,
                    help="least seconds per timed window (not with --trees alone)")
    ap.add_argument("--digest", action="store_true",
                    help="no timing: sha1 of every array of the six evaluation calls (profiles/geo_digest.json)")
    arg = ap.parse_args()
    if arg.clock and not arg.trees:
        ap.error("--clock goes with --trees")
    if arg.out is None:
        arg.out = os.path.join(ROOT, "profiles", "geo_digest.json" if arg.digest else
                               "geo_trees_clock_latency.json" if arg.clock else
                               "geo_trees_latency.json" if arg.trees else
                               "geo_summaries_latency.json" if arg.summaries else "geo_latency.json")
    if arg.digest:
        return digest(arg)
    if arg.clock:
        return trees_clock(arg)
    if arg.trees:
        return trees(arg)
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
            med, lo, hi, reps = windows(lambda: eng.evaluate_rows(blens[:n], params[:n]), arg.window)
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
    doc = {"what": "phy_geo_eval latency (host clock around the synchronous call, median of 5 windows of >= %g s) "
                   "against geo_gradients_host on one thread of the same box" % arg.window,
           "tool": "tools/geo_latency.py", "rows": rows}
    os.makedirs(os.path.dirname(os.path.abspath(arg.out)), exist_ok=True)
    with open(arg.out, "w") as fp:
        json.dump(doc, fp, indent=1)
    print("wrote", arg.out)


if __name__ == "__main__":
    main()
