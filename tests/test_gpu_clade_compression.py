"""Clade compression of the batched sweep (phy_set_clade_compression) against
the C port (oracle/cpu) at tests/test_gpu_00_configs.py's tolerances, and
against the uncompressed sweep.

Small shapes that reach every new path: 10 to 12 taxa, 129 to 200 patterns
(two blocks at two columns per lane, the second one ragged), with clades whose
columns are drawn from a pool of 20 tuples while four other taxa spell the
pattern's index in base 4 -- so the clade's parent has one class per pattern
and the clade is exactly the maximal one.  Every case runs 40 and 2 draws
through phy_eval_device with two columns per lane and one workgroup per draw.

The cap on compressed against uncompressed rows, 1e-13 of each array's largest
entry, bounds a reordering of exact sums of at most 200 terms per entry: the
forward values are the same bits (log-likelihoods must be equal), each dL/dP
entry is the same multiset of products summed in another order, which moves it
by a few units of 2^-53 times the sum of magnitudes -- about 1e-15 to 1e-14 of
the array's largest entry.  The oracle comparison is made for the compressed
and the uncompressed rows separately, so the cap hides nothing."""
import functools

import numpy as np
import pytest

from phylostan_amd import models
from tests import cases
from tests.test_gpu_00_configs import RTOL_G, RTOL_LL, check, errors

pytestmark = pytest.mark.gpu

KIND = {"JC69": 0, "HKY": 1, "GTR": 2}
DRAWS = 40
X, Y, FLAGS = 0, 1, 6
F_NOSTORE = 8


class _Tree:
    def __init__(self, S):
        self.S, self.nxt, self.rows = S, S, []

    def join(self, a, b):
        v = self.nxt
        self.nxt += 1
        self.rows.append([a, b, v])
        return v

    def bal4(self, t):
        return self.join(self.join(t[0], t[1]), self.join(t[2], t[3]))

    def cat4(self, t):
        return self.join(self.join(self.join(t[0], t[1]), t[2]), t[3])

    def cat5(self, t):  # a rebuilt cherry, then one-tip nodes rebuilt at depths 2 and 3 above it
        return self.join(self.join(self.join(self.join(t[0], t[1]), t[2]), t[3]), t[4])

    def peel(self):
        assert self.nxt == 2 * self.S - 1
        return np.array(self.rows, dtype=np.int32)


# name -> (clade shapes, where the first clade hangs, P, model, C, rooted, data variant)
SPECS = {
    "basic_hky4": (["bal4"], "inner", 200, "HKY", 4, True, None),
    "basic_gtr2": (["bal4"], "inner", 130, "GTR", 2, True, None),
    "two_clades": (["bal4", "cat4"], "inner", 170, "HKY", 4, True, None),
    "root_child": (["bal4"], "root", 150, "GTR", 2, True, None),
    "chain": (["cat5"], "inner", 160, "HKY", 4, True, None),
    "gap": (["bal4"], "inner", 140, "HKY", 4, True, "gap"),
    "unrooted": (["bal4"], "inner", 180, "GTR", 2, False, None),
    "skewed": (["bal4"], "inner", 200, "HKY", 4, True, "skewed"),
    "p129": (["bal4"], "inner", 129, "HKY", 4, True, None),
}
NTIPS = {"bal4": 4, "cat4": 4, "cat5": 5}


def _build(name):
    shapes, hang, P, model, C, rooted, variant = SPECS[name]
    rng = np.random.default_rng(sorted(SPECS).index(name) + 11)
    k = [NTIPS[s] for s in shapes]
    S = sum(k) + 4 + (2 if len(shapes) == 1 else 0)
    t = _Tree(S)
    tips = list(range(S))
    ctips = [tips[sum(k[:i]):sum(k[:i + 1])] for i in range(len(k))]
    dt = tips[sum(k):sum(k) + 4]
    rest = tips[sum(k) + 4:]
    roots = [getattr(t, s)(ct) for s, ct in zip(shapes, ctips)]
    D = t.bal4(dt)
    if len(shapes) == 2:  # the second clade is a child of the root
        t.join(roots[1], t.join(roots[0], D))
    elif hang == "root":
        t.join(roots[0], t.join(D, t.join(rest[0], rest[1])))
    else:  # (rest, (clade, D)): the last internal node before the root is (clade, D), as an unrooted peel needs
        r = t.join(rest[0], rest[1])
        t.join(r, t.join(roots[0], D))
    peel = t.peel()
    if not rooted:
        peel = cases.make_unrooted(peel)
    codes = rng.choice([1, 2, 4, 8], size=(S, P)).astype(np.uint8)
    perm = rng.permutation(256)[:P]  # distinct base-4 words: one class per pattern above the clade
    for j, d in enumerate(dt):
        codes[d] = 1 << ((perm >> (2 * j)) & 3)
    for ct in ctips:
        pool = rng.choice([1, 2, 4, 8], size=(20, len(ct))).astype(np.uint8)
        pool = np.unique(pool, axis=0)
        if variant == "gap":
            pool[::3, 1] = 15
            pool = np.unique(pool, axis=0)
        which = rng.integers(0, len(pool), P)
        if variant == "skewed":  # one class with most patterns, three with a single one
            which = np.concatenate([np.zeros(P - 40, dtype=int), [1, 2, 3], rng.integers(4, len(pool), 37)])
            which = which[rng.permutation(P)]
        codes[ct] = pool[which].T
    if variant == "gap":
        codes[rest[0], ::7] = 5
    B = 2 * S - 2 if rooted else 2 * S - 3
    freqs = rng.dirichlet(np.full(4, 5.0))
    rates = rng.uniform(0.5, 3.0, 6) if model == "GTR" else models.hky_exchangeabilities(rng.uniform(1.0, 8.0))
    rs, ps = models.weibull_site_rates(rng.uniform(0.3, 2.0), C)
    w = rng.integers(1, 5, P).astype(np.float64)
    case = cases.Case(name, codes, w, peel, rooted, model, C, rng.uniform(0.01, 0.3, B), freqs, rates, rs, ps)
    return case, roots


@functools.lru_cache(maxsize=None)
def _problem(name):
    """The case, its clade roots, DRAWS parameter points and their C-port results."""
    from oracle import cpu
    from phylostan_amd.engine import EvalResult
    case, roots = _build(name)
    rng = np.random.default_rng(3)
    B = len(case.blens)
    blens = np.vstack([case.blens] + [rng.uniform(0.01, 0.3, B) for _ in range(DRAWS - 1)])
    mv = np.tile(case.model_vec(), (DRAWS, 1))
    refs = []
    for d in range(DRAWS):
        out, sl = cpu.evaluate(case.tipcodes, case.weights, case.peel0, case.rooted, KIND[case.model], mv[d], blens[d],
                               case.C, site_ll=True)
        refs.append(EvalResult(out, B, case.C, sl).as_dict())
    return case, tuple(roots), blens, mv, refs


def _engine(case, max_draws=DRAWS):
    from phylostan_amd.engine import TreeLikelihood
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C, max_draws=max_draws)
    eng.set_engine("pattern")
    eng.set_tuning(wg_budget=1, cols=2)  # two columns per lane, one workgroup per draw
    assert eng.lds_plan()["cols"] == 2
    return eng


def _device_rows(eng, blens, mv, site=True):
    import torch
    n = blens.shape[0]
    d_bl = torch.tensor(blens, device="cuda:0")
    d_mv = torch.tensor(mv, device="cuda:0")
    d_out = torch.zeros((n, eng.outlen), dtype=torch.float64, device="cuda:0")
    d_site = torch.zeros((n, eng.P), dtype=torch.float64, device="cuda:0")
    eng.evaluate_device(d_bl.data_ptr(), d_mv.data_ptr(), d_out.data_ptr(), d_site.data_ptr() if site else 0,
                        n_draws=n, stream=torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_out.cpu().numpy(), d_site.cpu().numpy()


def _rel(a, b):
    return float(np.max(np.abs(np.asarray(a) - np.asarray(b))) / max(np.max(np.abs(b)), 1e-300))


def _check_rows(case, eng, rows, site, refs):
    from phylostan_amd.engine import EvalResult
    worst = {}
    for d in range(rows.shape[0]):
        res = EvalResult(rows[d], eng.B, eng.C, site[d])
        e = errors(res, refs[d], case.model)
        e["q"] = max(_rel(res.grad_rates, refs[d]["grad_rates"]), _rel(res.grad_freqs, refs[d]["grad_freqs"]))
        worst = {k: max(v, worst.get(k, 0.0)) for k, v in e.items()}
        check(e, e["q"])
    return worst


def _fields(eng, row):
    from phylostan_amd.engine import EvalResult
    r = EvalResult(row, eng.B, eng.C, None)
    return {k: getattr(r, k) for k in ("grad_blens", "grad_rs", "grad_ps", "grad_freq_root", "grad_rates",
                                       "grad_freqs", "dLdP")}


@pytest.mark.parametrize("name", sorted(SPECS))
def test_compressed_rows_vs_cport_and_uncompressed(name):
    from phylostan_amd.engine import clade_plan
    case, roots, blens, mv, refs = _problem(name)
    eng = _engine(case)
    try:
        eng.set_clade_compression("on")
        cc = eng.clade_compression()
        assert cc["clades"] == len(roots) and sorted(c["node"] for c in cc["clade_list"]) == sorted(roots), cc
        assert cc["blocks"] == 2 and all(c["classes"] <= 20 for c in cc["clade_list"])
        info = eng.program_info()
        assert info["clades"] == len(roots) and info["l_steps"] + info["u_steps"] == info["nsteps"]
        plan = clade_plan(case.tipcodes, case.peel0, case.rooted, case.C, 5, 64, True, 1)
        prog, nL = plan["program"], plan["l_steps"]
        if name == "chain":  # a rebuilt cherry and the one-tip node above it, inside the clade
            assert int(((prog[:nL, FLAGS] & F_NOSTORE) != 0).sum()) >= 2 and int((prog[:nL, 15] == 2).sum()) >= 1
        if name == "skewed":
            sizes = (plan["members"][0] >= 0).sum(axis=0)
            assert sizes.max() >= case.P - 40 and (sizes == 1).sum() >= 1
        if name == "root_child":
            assert any(r in roots for r in case.peel0[-1][:2])
        if name == "unrooted":  # the merged root branch is a U step with a gathered child
            merged = prog[prog[:, 14] == 2 * case.S - 3][0]
            assert not (merged[FLAGS] & 1) and min(merged[X], merged[Y]) <= -2
        on, on_site = _device_rows(eng, blens, mv)
        on2, _ = _device_rows(eng, blens, mv)
        on_few, on_few_site = _device_rows(eng, blens[:2], mv[:2])
        eng.set_clade_compression("off")
        assert eng.clade_compression()["clades"] == 0
        off, off_site = _device_rows(eng, blens, mv)
    finally:
        eng.close()
    assert np.array_equal(on, on2)  # bitwise reproducible
    assert np.array_equal(on_few, on[:2]) and np.array_equal(on_few_site, on_site[:2])
    w_on = _check_rows(case, eng, on, on_site, refs)
    w_off = _check_rows(case, eng, off, off_site, refs)
    print(name, "compressed", w_on, "uncompressed", w_off)
    # the forward is the same bits; the gradients a reordering of exact sums
    assert np.array_equal(on[:, 0], off[:, 0]) and np.array_equal(on_site, off_site)
    worst = 0.0
    for d in range(DRAWS):
        a, b = _fields(eng, on[d]), _fields(eng, off[d])
        worst = max(worst, max(_rel(a[k], b[k]) for k in a))
    print(name, "compressed vs uncompressed", worst)
    assert worst <= 1e-13, worst
    assert RTOL_G == 1e-9 and RTOL_LL == 1e-10


def test_mode_off_is_bitwise_a_context_created_off(monkeypatch):
    case, _, blens, mv, _ = _problem("basic_hky4")
    monkeypatch.setenv("PHY_CLADE_COMPRESSION", "0")
    ref_eng = _engine(case)
    try:
        assert ref_eng.clade_compression()["mode"] == 0
        ref, ref_site = _device_rows(ref_eng, blens, mv)
    finally:
        ref_eng.close()
    monkeypatch.delenv("PHY_CLADE_COMPRESSION")
    eng = _engine(case)
    try:
        eng.set_clade_compression("on")
        on, _ = _device_rows(eng, blens, mv)
        eng.set_clade_compression("off")
        off, off_site = _device_rows(eng, blens, mv)
    finally:
        eng.close()
    assert np.array_equal(off, ref) and np.array_equal(off_site, ref_site)
    assert not np.array_equal(on, ref)  # the compressed plan did run


def test_compact_rows_are_the_full_rows_head():
    case, _, blens, mv, _ = _problem("two_clades")
    eng = _engine(case)
    try:
        eng.set_clade_compression("on")
        assert eng.clade_compression()["clades"] == 2
        full, _ = _device_rows(eng, blens, mv, site=False)
        eng.set_output(compact=True)
        compact, _ = _device_rows(eng, blens, mv, site=False)
    finally:
        eng.close()
    assert compact.shape[1] == 1 + eng.B + 2 * eng.C + 14
    assert np.array_equal(compact, full[:, :compact.shape[1]])


def test_rescaling_switches_compression_off_and_back():
    case, _, blens, mv, refs = _problem("basic_hky4")
    eng = _engine(case)
    try:
        eng.set_clade_compression("on")
        on, on_site = _device_rows(eng, blens, mv)
        eng.set_clade_compression("off")
        eng.set_rescaling(True)
        rs_off, _ = _device_rows(eng, blens, mv)
        eng.set_clade_compression("on")
        rs_on, rs_site = _device_rows(eng, blens, mv)  # rescaled sweep: the compressed plan is not taken
        eng.set_rescaling(False)
        back, back_site = _device_rows(eng, blens, mv)
    finally:
        eng.close()
    assert np.array_equal(rs_on, rs_off)
    _check_rows(case, eng, rs_on, rs_site, refs)
    assert np.array_equal(back, on) and np.array_equal(back_site, on_site)


def test_deep_stack_in_global_memory():
    case, roots, blens, mv, refs = _problem("two_clades")
    eng = _engine(case)
    try:
        eng.set_deep_stack(2)
        eng.set_tuning(wg_budget=1, cols=2)
        assert eng.lds_plan()["deep_lds_entries"] == 0 and eng.program_info()["depth"] >= 1
        eng.set_clade_compression("on")
        assert eng.clade_compression()["clades"] == len(roots)
        on, on_site = _device_rows(eng, blens[:3], mv[:3])
    finally:
        eng.close()
    _check_rows(case, eng, on, on_site, refs[:3])


def test_fluA_automatic_plan_vs_cport():
    from oracle import cpu
    from phylostan_amd.engine import EvalResult, TreeLikelihood
    case = cases.fluA_case()
    n = 64
    rng = np.random.default_rng(9)
    blens = case.blens[None, :] * rng.uniform(0.7, 1.3, (n, len(case.blens)))
    mv = np.tile(case.model_vec(), (n, 1))
    eng = TreeLikelihood(case.tipcodes, case.weights, case.peel0, case.rooted, case.model, case.C, max_draws=n)
    try:
        eng.set_tuning(wg_budget=1, cols=2)
        cc = eng.clade_compression()
        if cc["mode"] == 0:  # the shipped default may be off: the automatic selection is what is tested
            eng.set_clade_compression("auto")
            cc = eng.clade_compression()
        assert 114 in {c["node"] for c in cc["clade_list"]}, cc
        rows, site = _device_rows(eng, blens, mv)
    finally:
        eng.close()
    refs = []
    for d in range(n):
        out, sl = cpu.evaluate(case.tipcodes, case.weights, case.peel0, case.rooted, KIND[case.model], mv[d], blens[d],
                               case.C, site_ll=True)
        refs.append(EvalResult(out, eng.B, case.C, sl).as_dict())
    print("fluA automatic", _check_rows(case, eng, rows, site, refs))
