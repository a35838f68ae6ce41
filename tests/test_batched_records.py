"""The batched sweep's step records (phy_plan_records, no device).

The two-column kernel loads one 16-int record per step in which every index
is already the byte offset it adds.  Here every offset is recomputed from the
raw program and the plan -- entry stride, chunk base, the "operand not loaded"
rule -- for three trees, one and two columns per lane, and two chunk plans
(what a set_tuning that shrinks the LDS budget changes)."""
import numpy as np
import pytest

from phylostan_amd.engine import plan_records
from tests import cases

# raw program fields / record fields (include/phylo_hip_diag.h)
X, Y, MX, MY, MV, VSLOT, FLAGS, XSLOT, YSLOT, XDPOS, VDPOS, CHUNK, M0, MN, NODE, RD = range(16)
(BR_X, BR_Y, BR_MXO, BR_MYO, BR_MVO, BR_VSO, BR_FLRD, BR_XSO, BR_YSO, BR_XDPOS, BR_VDPOS, BR_GX, BR_M0, BR_MN,
 BR_GY, BR_GV) = range(16)
F_MV, F_XDEEP, F_VDEEP, F_NOSTORE, F_PREVREC = 1, 2, 4, 8, 16
OOB = 0x40000000


def _trees():
    flu = cases.load_layout("fluA")
    ds1 = cases.ds1_case()
    cat = cases.random_peel(12, np.random.default_rng(0), caterpillar=True)
    return {"fluA": (flu["peel"] - 1, True), "DS1_unrooted": (ds1.peel0, False), "caterpillar12": (cat, True)}


TREES = _trees()


def _check(prog, recs, nmat, nch, K, C, R, cap):
    estr = K * 2 * C * 64 * 16  # bytes per scratch entry
    rec8 = R * 32  # bytes per matrix record
    n = prog.shape[0]
    chunks = set()
    for s in range(n):
        p, q = prog[s], recs[s]
        fl, rd = int(p[FLAGS]), int(p[RD])
        rec = bool(fl & F_PREVREC)
        for child, row, m, mo, g in ((X, BR_X, MX, BR_MXO, BR_GX), (Y, BR_Y, MY, BR_MYO, BR_GY)):
            if p[child] >= 0:  # a tip: nibble row offset, its matrix inside the chunk, its slot
                assert q[row] == p[child] * K * 32
                assert 0 <= p[m] - p[M0] < p[MN] <= cap
                assert q[mo] == (p[m] - p[M0]) * rec8
                assert q[g] == p[m] * 128
            else:
                assert q[row] == -1 and p[m] == -1
        if fl & F_MV:
            assert 0 <= p[MV] - p[M0] < p[MN]
            assert q[BR_MVO] == (p[MV] - p[M0]) * rec8 and q[BR_GV] == p[MV] * 128
        else:
            assert p[MV] == -1
        assert q[BR_VSO] == (p[VSLOT] * estr if p[VSLOT] >= 0 else -1)
        assert (p[VSLOT] < 0) == (s == n - 1)
        assert q[BR_FLRD] == fl | (rd << 8) and (rd > 0) == rec
        # operands the reverse loads: an internal child, unless it is the
        # rebuilt previous-step child (y when y is internal, else x)
        load_x = p[X] < 0 and not (rec and p[Y] >= 0)
        load_y = p[Y] < 0 and not rec
        assert q[BR_XSO] == (p[XSLOT] * estr if load_x else OOB)
        assert q[BR_YSO] == (p[YSLOT] * estr if load_y else OOB)
        for load, slot in ((load_x, XSLOT), (load_y, YSLOT)):
            if load:  # what is loaded was stored (a slot is its step's index)
                assert not prog[p[slot]][FLAGS] & F_NOSTORE
                assert p[slot] * estr + estr <= OOB
        if rec:  # the operand not loaded is the step before, rebuilt inside one chunk
            skipped = YSLOT if p[Y] < 0 else XSLOT
            assert p[skipped] == s - 1 and prog[s - 1][FLAGS] & F_NOSTORE
            assert all(prog[s - j][M0] == p[M0] for j in range(1, rd + 1))
        assert q[BR_XDPOS] == p[XDPOS] and q[BR_VDPOS] == p[VDPOS]
        assert q[BR_M0] == p[M0] and q[BR_MN] == p[MN]
        chunks.add((int(p[CHUNK]), int(p[M0]), int(p[MN])))
    assert len(chunks) == nch and len({c[1] for c in chunks}) == nch  # m0 names the chunk
    assert sum(c[2] for c in chunks) == nmat


@pytest.mark.parametrize("K", [1, 2])
@pytest.mark.parametrize("name", sorted(TREES))
def test_record_offsets_follow_the_plan(name, K):
    peel0, rooted = TREES[name]
    S = peel0.shape[0] + 1
    nch_seen = []
    for C, R, cap in ((4, 4, 3 * S), (4, 6, 9), (1, 5, 3)):  # one chunk; the plan of a small LDS budget; the smallest
        prog, recs, nmat, nch = plan_records(peel0, rooted, C, R, K, cap)
        assert nmat == (2 * S - 2 if rooted else 2 * S - 3)
        _check(prog, recs, nmat, nch, K, C, R, cap)
        nch_seen.append(nch)
    assert nch_seen[0] == 1 and nch_seen[1] >= 3 and nch_seen[2] > nch_seen[1]


def test_trees_reach_the_paths():
    """The three trees cover what the records encode: rebuilt chains up to
    depth 4 (caterpillar), the merged root branch (unrooted: two steps
    without a matrix), deep-stack operands (fluA)."""
    prog, _, _, _ = plan_records(TREES["caterpillar12"][0], True, 4, 4, 2, 64)
    assert prog[:, RD].max() == 4
    prog, _, _, _ = plan_records(TREES["DS1_unrooted"][0], False, 1, 4, 2, 64)
    assert int(np.sum((prog[:, FLAGS] & F_MV) == 0)) == 2
    prog, _, _, _ = plan_records(TREES["fluA"][0], True, 4, 4, 2, 64)
    assert np.any(prog[:, FLAGS] & F_XDEEP) and np.any(prog[:, FLAGS] & F_VDEEP)
    off, _, _, _ = plan_records(TREES["fluA"][0], True, 4, 4, 2, 64, recompute=False)
    assert not np.any(off[:, FLAGS] & (F_PREVREC | F_NOSTORE)) and np.any(prog[:, FLAGS] & F_PREVREC)
