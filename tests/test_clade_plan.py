"""CPU: the compressed-clade plan (phy_clade_plan, no device) on the fluA and
HCV fixtures -- the clades taken, the class and member tables, the L and U
programs and their records -- and, with compression off, the uncompressed
plan's program and records byte for byte (tests/golden/plan_records_uncompressed.npz:
phy_plan_records of the commit before clade compression)."""
import functools
import os

import numpy as np
import pytest

from tests import cases

X, Y, MX, MY, MV, VSLOT, FLAGS, XSLOT, YSLOT, XDPOS, VDPOS, CHUNK, M0, MN, NODE, RD = range(16)
BR_X, BR_Y, BR_VSO, BR_XSO, BR_YSO, BR_GX, BR_GY = 0, 1, 5, 7, 8, 11, 14
F_MV, F_XDEEP, F_VDEEP, F_NOSTORE, F_PREVREC = 1, 2, 4, 8, 16
OOB = 0x40000000
CAP, R = 69, 5

FIXTURES = {"fluA": cases.fluA_case, "HCV": cases.hcv_case}
# (root node, internal nodes, classes, largest class) of every maximal clade of at most 128 classes and at least
# three internal nodes, and the block-steps before / after (steps x blocks)
EXPECT = {
    "fluA": ([(76, 3, 15, 62), (114, 36, 123, 28), (121, 6, 34, 58)], 136, 91),
    "HCV": (6, 124, 73),
}


def _lib_built():
    from phylostan_amd import _lib
    return os.path.exists(_lib.LIB_PATH)


pytestmark = pytest.mark.skipif(not _lib_built(), reason="HIP library not built (run __graft_entry__.build())")


@functools.lru_cache(maxsize=None)
def _plan(name, mode):
    from phylostan_amd.engine import clade_plan
    case = FIXTURES[name]()
    return case, clade_plan(case.tipcodes, case.peel0, case.rooted, case.C, R, CAP, True, mode)


def _subtree_tips(case, node):
    kids = {int(v): (int(a), int(b)) for a, b, v in case.peel0}
    out, st = [], [node]
    while st:
        n = st.pop()
        if n < case.S:
            out.append(n)
        else:
            st.extend(kids[n])
    return sorted(out)


def _model_keeps(node, plan):
    """The cost model of sweep_plan.h (plan_clades), restated: cycles of one
    category wave per draw, calibrated on an MI355X from the fluA A/B runs.
    With the uncalibrated constants it started from (boundary 2 k per block,
    200 per round) it kept fluA's node 121 too; measured, that clade's boundary
    (two blocks, 58 rounds: about 53 k cycles) costs more than the 28 k its
    six steps save -- fluA at 8,192 draws ran 1.42 M evals/s with nodes 76,
    114 and 121, 1.49 M with 114 and 121, against 1.33 M uncompressed -- so
    the automatic plan keeps 114 alone and mode 1 takes all three."""
    c = [c for c in plan["clade_list"] if c["node"] == node][0]
    save = (plan["blocks"] - 1) * c["internal_nodes"] * 4700
    cost = plan["blocks"] * 13000 + -(-c["maxmult"] // 8) * 2500 + 7000
    return 4 * save > 5 * cost


def test_fluA_takes_the_issue_s_clades():
    case, on = _plan("fluA", 1)
    got = sorted((c["node"], c["internal_nodes"], c["classes"], c["maxmult"]) for c in on["clade_list"])
    want, before, after = EXPECT["fluA"]
    assert got == want
    assert (case.S - 1) * on["blocks"] == before
    assert on["l_steps"] + on["blocks"] * on["u_steps"] == after
    # the automatic plan keeps what the calibrated cost model says pays
    _, auto = _plan("fluA", -1)
    assert sorted(c["node"] for c in auto["clade_list"]) == [n for n, *_ in want if _model_keeps(n, on)]
    assert 114 in [c["node"] for c in auto["clade_list"]]
    assert auto["u_matrices"] == 136 - sum(2 * c["internal_nodes"] + 1 for c in auto["clade_list"])


def test_hcv_takes_six_clades():
    case, on = _plan("HCV", 1)
    n, before, after = EXPECT["HCV"]
    assert on["clades"] == n
    assert (case.S - 1) * on["blocks"] == before
    assert on["l_steps"] + on["blocks"] * on["u_steps"] == after
    assert all(c["classes"] <= 128 and c["internal_nodes"] >= 3 for c in on["clade_list"])


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("mode", [-1, 1])
def test_class_and_member_tables(name, mode):
    case, plan = _plan(name, mode)
    P = case.P
    for ci, c in enumerate(plan["clade_list"]):
        tips = _subtree_tips(case, c["node"])
        cls, rep, mem = plan["cls_of"][ci], plan["rep"][ci], plan["members"][ci]
        assert np.all(cls[P:] == -1) and cls[:P].min() == 0 and cls[:P].max() == c["classes"] - 1
        assert np.all(rep[:c["classes"]] >= 0) and np.all(rep[c["classes"]:] == -1)
        # every pattern's column holds exactly its tuple of the clade's tip states
        assert np.array_equal(case.tipcodes[tips][:, rep[cls[:P]]], case.tipcodes[tips])
        # distinct classes hold distinct tuples
        assert len(np.unique(case.tipcodes[tips][:, rep[:c["classes"]]], axis=1).T) == c["classes"]
        # every pattern exactly once, ascending within its class, no holes
        listed = mem[mem >= 0]
        assert sorted(listed.tolist()) == list(range(P))
        for j in range(128):
            col = mem[:, j]
            k = int((col >= 0).sum())
            assert np.all(col[:k] >= 0) and np.all(col[k:] == -1) and np.all(np.diff(col[:k]) > 0)
            assert np.all(cls[col[:k]] == j)
        assert max(int((mem[:, j] >= 0).sum()) for j in range(128)) == c["maxmult"]
        assert plan["rounds"] % 4 == 0 and plan["rounds"] >= c["maxmult"]


@pytest.mark.parametrize("name", sorted(FIXTURES))
def test_programs_cover_the_tree_and_store_the_clade_roots(name):
    case, plan = _plan(name, 1)
    prog, recs, nL = plan["program"], plan["records"], plan["l_steps"]
    S = case.S
    assert sorted(prog[:, NODE].tolist()) == list(range(S, 2 * S - 1))  # L u U: every internal node once
    assert sorted(plan["mat_branch"].tolist()) == list(range(2 * S - 2))
    estr = 2 * 2 * case.C * 64 * 16
    step_of = {int(prog[s, NODE]): s for s in range(len(prog))}
    roots = {c["node"]: ci for ci, c in enumerate(plan["clade_list"])}
    for ci, c in enumerate(plan["clade_list"]):
        lo, hi = c["first_step"], c["last_step"]
        assert hi - lo + 1 == c["internal_nodes"] and hi < nL
        assert prog[lo, X] >= 0 and prog[lo, Y] >= 0  # a clade starts at a cherry: nothing popped across clades
        root = prog[hi]
        assert root[NODE] == c["node"] and root[VSLOT] == hi and not (root[FLAGS] & (F_NOSTORE | F_VDEEP))
        assert recs[hi, BR_VSO] == hi * estr
        nodes = set(prog[lo:hi + 1, NODE].tolist())
        tips = set(_subtree_tips(case, c["node"]))
        for s in range(lo, hi + 1):  # the clade's steps touch its own nodes only, none gathered
            for ch in (X, Y):
                assert prog[s, ch] >= -1 and (prog[s, ch] < 0 or prog[s, ch] in tips)
        assert len(nodes) == c["internal_nodes"]
    # no chunk straddles the L / U boundary
    assert prog[nL - 1, CHUNK] != prog[nL, CHUNK] and prog[nL, M0] == plan["l_matrices"]
    # U: every clade root is a gathered child exactly once, with its slot and r plane in the record
    seen = []
    for s in range(nL, len(prog)):
        for ch, so, g in ((X, BR_XSO, BR_GX), (Y, BR_YSO, BR_GY)):
            if prog[s, ch] <= -2:
                ci = -2 - int(prog[s, ch])
                seen.append(ci)
                node = plan["clade_list"][ci]["node"]
                assert recs[s, ch] == prog[s, ch]
                assert recs[s, so] == step_of[node] * estr
                assert recs[s, g] == (S - 1 + ci * plan["blocks"]) * estr
                assert not (prog[s, FLAGS] & F_PREVREC)
            elif prog[s, ch] == -1:
                assert recs[s, ch] == -1
    assert sorted(seen) == list(range(plan["clades"]))
    assert plan["scratch_entries"] == S - 1 + plan["clades"] * plan["blocks"]
    assert (plan["scratch_entries"] * estr) < OOB
    del roots


@pytest.mark.parametrize("name", sorted(FIXTURES))
@pytest.mark.parametrize("cap", [69, 24])
def test_uncompressed_plan_is_byte_identical(name, cap):
    from phylostan_amd.engine import clade_plan, plan_records
    case = FIXTURES[name]()
    gold = np.load(os.path.join(cases.GOLDEN, "plan_records_uncompressed.npz"))
    prog, recs, nmat, _ = plan_records(case.peel0, case.rooted, case.C, R, 2, cap, True)
    assert nmat == 2 * case.S - 2
    assert prog.tobytes() == gold["%s_cap%d_program" % (name, cap)].tobytes()
    assert recs.tobytes() == gold["%s_cap%d_records" % (name, cap)].tobytes()
    assert clade_plan(case.tipcodes, case.peel0, case.rooted, case.C, R, cap, True, 0)["clades"] == 0
