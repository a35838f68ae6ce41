"""The column sweeps on the paths the batched step records changed, against
the C port (oracle/cpu) at tests/test_gpu_00_configs.py's tolerances.

Small shapes that reach each path: 130 patterns (two blocks at two columns
per lane: the slot stores, then the atomic adds, and padding columns), 300
patterns (three blocks), an LDS budget that cuts the program into at least
three chunks with a cherry whose parent starts the next chunk (stored, not
rebuilt), an unrooted tree (the merged root branch: a step without a
matrix), ambiguous tip masks (R > 4), one and two columns per lane, the deep
stack in LDS and in global memory; three draws each.  An explicit column
plan keeps a small call on the column sweeps (no quad sweep)."""
import functools

import numpy as np
import pytest

from tests import cases
from tests.test_gpu_00_configs import RTOL_G, check, errors

pytestmark = pytest.mark.gpu

X, Y, FLAGS, VDPOS, CHUNK = 0, 1, 6, 10, 11
KIND = {"JC69": 0, "HKY": 1, "GTR": 2}
DRAWS = 3
S, C = 12, 6
BUDGET = 16384  # the smallest LDS budget phy_set_tuning takes


def _lds_bytes(S, C, R, cap, K, ndl):
    """include/phylo_hip_diag.h's LDS plan: tips, state vectors, chunks, tails."""
    tip = (S * 64 * K // 2 + 15) // 16 * 16
    tail = ndl * K * 2 * 64 * 2 if ndl > 0 else K * 64
    return tip + 16 * 4 * 8 + C * cap * R * 32 + C * tail * 8


def _cap(S, C, R, K, ndl, nmat):
    """Matrices per chunk under BUDGET (at least 3: one step's)."""
    cap = nmat
    while cap > 3 and _lds_bytes(S, C, R, cap, K, ndl) > BUDGET:
        cap -= 1
    return cap


def _records(case):
    return 4 + len(set(np.unique(case.tipcodes).tolist()) - {1, 2, 4, 8} | {15})


def _straddles(peel0, rooted, cap):
    """Steps whose previous step is a cherry in the chunk before theirs."""
    from phylostan_amd.engine import plan_records
    prog, _, _, nch = plan_records(peel0, rooted, 1, 4, 2, cap)
    hits = [s for s in range(1, len(prog))
            if prog[s - 1][X] >= 0 and prog[s - 1][Y] >= 0 and (prog[s][X] < 0 or prog[s][Y] < 0)
            and prog[s][CHUNK] != prog[s - 1][CHUNK]]
    return nch, hits, int(prog[:, VDPOS].max()) + 1  # ..., deep-stack entries


@functools.lru_cache(maxsize=None)
def _problem(P, rooted):
    """A 12-taxon GTR+6 case with ambiguous tips whose program uses the deep
    stack and whose plans under BUDGET (one and two columns, the deep stack in
    LDS and in global memory) all have at least three chunks and a cherry
    straddling a chunk boundary; its three draws and their C-port rows."""
    from oracle import cpu
    from phylostan_amd.engine import EvalResult
    for seed in range(200):
        case = cases.random_case(seed, S=S, P=P, C=C, model="GTR", rooted=rooted, ambiguous=0.1)
        depth = _straddles(case.peel0, rooted, 64)[2]
        caps = {_cap(S, C, _records(case), K, ndl, len(case.blens)) for K in (1, 2) for ndl in (0, depth)}
        if depth >= 1 and all(n >= 3 and hits for n, hits, _ in (_straddles(case.peel0, rooted, c) for c in caps)):
            break
    else:
        raise AssertionError("no tree with a straddling cherry")
    rng = np.random.default_rng(7)
    B = len(case.blens)
    blens = np.vstack([case.blens] + [rng.uniform(0.01, 0.3, B) for _ in range(DRAWS - 1)])
    mv = np.tile(case.model_vec(), (DRAWS, 1))
    refs = []
    for d in range(DRAWS):
        out, sl = cpu.evaluate(case.tipcodes, case.weights, case.peel0, rooted, KIND[case.model], mv[d], blens[d],
                               case.C, site_ll=True)
        r = EvalResult(out, B, case.C, sl)
        refs.append(r.as_dict())
    return case, blens, mv, refs


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


@pytest.mark.parametrize("deep", [1, 2], ids=["deep_lds", "deep_global"])
@pytest.mark.parametrize("chunks", ["one_chunk", "small_budget"])
@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("P,rooted", [(130, True), (300, True), (130, False)],
                         ids=["130_rooted", "300_rooted", "130_unrooted"])
def test_column_sweep_paths_vs_cport(P, rooted, K, chunks, deep):
    from phylostan_amd.engine import TreeLikelihood
    case, blens, mv, refs = _problem(P, rooted)
    R = _records(case)
    assert R > 4
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, rooted, case.model, case.C, max_draws=DRAWS)
    try:
        eng.set_engine("pattern")
        eng.set_deep_stack(deep)
        depth = eng.program_info()["depth"]
        if chunks == "small_budget":
            cap = _cap(S, C, R, K, depth if deep == 1 else 0, len(case.blens))
            eng.set_tuning(cols=K, lds_budget=BUDGET)
        else:
            eng.set_tuning(cols=K)
        plan = eng.lds_plan()
        assert plan["cols"] == K
        assert depth >= 1 and plan["deep_lds_entries"] == (depth if deep == 1 else 0)
        assert eng.program_info()["nblocks"] == -(-P // (64 * K)) >= 2
        if chunks == "small_budget":
            assert plan["matrices_per_chunk"] == cap and plan["n_chunks"] >= 3
            assert _straddles(case.peel0, rooted, cap)[1]
        else:
            assert plan["n_chunks"] == 1
        res = eng.evaluate_batch(blens, mv, site_ll=True)
    finally:
        eng.close()
    for d in range(DRAWS):
        check(errors(res[d], refs[d], case.model))
        assert max(_rel(res[d].grad_rates, refs[d]["grad_rates"]),
                   _rel(res[d].grad_freqs, refs[d]["grad_freqs"])) <= 1e-8
    assert RTOL_G == 1e-9
