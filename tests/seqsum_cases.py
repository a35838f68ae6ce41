"""The cases of the sequence-summary tests (CPU and GPU) and their truth rows,
computed once per process (tests/seqsum_truth.py)."""
import functools

import numpy as np

from tests import cases, seqsum_truth

# (S, P, C, model, rooted): one column, a block less one, a full block, a block
# and one, two blocks and one, and 16 categories past two blocks
SHAPES = [(3, 1, 1, "JC69", True), (4, 63, 1, "JC69", False), (5, 64, 4, "HKY", False), (5, 65, 4, "HKY", True),
          (9, 129, 3, "GTR", True), (8, 130, 16, "GTR", False)]
TREES = ["caterpillar", "balanced"]


def balanced_peel(S):
    """Pairs of the current nodes level by level (S a power of two: a
    perfectly balanced tree)."""
    nodes, nxt, peel = list(range(S)), S, []
    while len(nodes) > 1:
        up = []
        for k in range(0, len(nodes) - 1, 2):
            peel.append([nodes[k], nodes[k + 1], nxt])
            up.append(nxt)
            nxt += 1
        if len(nodes) % 2:
            up.append(nodes[-1])
        nodes = up
    return np.array(peel, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def shape_case(k):
    S, P, C, model, rooted = SHAPES[k]
    return cases.random_case(300 + k, S=S, P=P, C=C, model=model, rooted=rooted)


@functools.lru_cache(maxsize=None)
def tree_case(kind):
    c = cases.random_case(77, S=16, P=40, C=4, model="HKY", rooted=True, caterpillar=(kind == "caterpillar"))
    if kind == "balanced":
        c.peel0 = balanced_peel(16)
    return c


@functools.lru_cache(maxsize=None)
def missing_case():
    """SHAPES[3] with its last pattern (the lone column of the second block)
    missing at every tip."""
    c = cases.random_case(303, S=5, P=65, C=4, model="HKY", rooted=True)
    c.tipcodes = c.tipcodes.copy()
    c.tipcodes[:, 64] = 15
    return c


@functools.lru_cache(maxsize=None)
def draws_case():
    """The case whose parameter points the bitwise / running-sum tests vary."""
    return cases.random_case(41, S=7, P=70, C=3, model="GTR", rooted=True)


def draws(case, n, seed=5):
    """n parameter points around the case's own: (blens [n, B], model [n, 10 + 2C])."""
    rng = np.random.default_rng(seed)
    bl = case.blens[None, :] * rng.uniform(0.5, 1.5, (n, case.blens.size))
    mv = np.repeat(case.model_vec()[None, :], n, axis=0)
    if case.model != "JC69":
        f = rng.dirichlet(np.full(4, 20.0), n)
        mv[:, :4] = f
    return np.ascontiguousarray(bl), np.ascontiguousarray(mv)


@functools.lru_cache(maxsize=None)
def truth(key):
    """The truth row of shape_case(k) (key = k), tree_case(kind) (key = kind)
    or missing_case() (key = "missing"); shared, never modified."""
    case = missing_case() if key == "missing" else tree_case(key) if key in TREES else shape_case(key)
    row = seqsum_truth.truth_row(case)
    row.setflags(write=False)
    return row


def check_row(row, case, want, what=""):
    """The issue's bars: 1e-10 absolute on anc and cat, 1e-10 relative on rate;
    every (node, pattern) sums to one."""
    from phylostan_amd.seqsum import split_row
    S, P, C = case.S, case.P, case.C
    _, anc, cat, rate = split_row(np.asarray(row), S, P, C)
    _, tanc, tcat, trate = split_row(np.asarray(want), S, P, C)
    errs = (float(np.abs(anc - tanc).max()), float(np.abs(cat - tcat).max()),
            float(np.max(np.abs(rate - trate) / np.abs(trate))), float(np.abs(anc.sum(axis=1) - 1.0).max()),
            float(np.abs(cat.sum(axis=0) - 1.0).max()))
    print("%s anc %.2e cat %.2e rate(rel) %.2e anc-sum %.2e cat-sum %.2e" % ((what,) + errs))
    assert errs[0] < 1e-10 and errs[1] < 1e-10 and errs[2] < 1e-10
    assert errs[3] < 1e-10 and errs[4] < 1e-10
    assert np.all(anc >= 0.0) and np.all(anc <= 1.0 + 1e-12)
