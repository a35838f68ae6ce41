"""The exact reference of the K-state sequence engine, and the cases its tests
share.  numpy only; shares no algebra and no code with ``phylostan_amd.kseq``: the tip
masks are decoded here, bit by bit.

Q is built directly (``geo_oracle.build_q``), P_{b,c} = expm(Q t_b r_c) by
scaling and squaring of a Taylor series on complex arrays (``geo_oracle.expm``),
the pruning is a plain loop over categories and peel rows, and each derivative
is Im f(theta + 1e-30 i) / 1e-30.  ``extended=True`` normalises every internal
partial by its largest real part, pattern by pattern, and carries the logs: for
trees whose likelihood leaves the fp64 range.
"""
import os

import numpy as np

from tests.geo_oracle import STEP, build_q, caterpillar_peel, expm, random_peel


# The truth's own reading of the data: nothing here comes from phylostan_amd.kseq.
def rate_count(K):
    return K * (K - 1) // 2


def num_branches(S, rooted):
    return 2 * S - 2 if rooted else 2 * S - 3


def onehot_masks(states):
    return np.asarray([[1 << int(s) for s in row] for row in np.asarray(states)], np.uint64)


def full_mask(K):
    return np.uint64(2 ** K - 1)


def decode_masks(masks, K):
    """[S][P][K] 0 / 1: entry j of a tip's vector is bit j of its mask, read with Python integers."""
    masks = np.asarray(masks, np.uint64)
    out = np.zeros(masks.shape + (K,))
    for t in range(masks.shape[0]):
        for p in range(masks.shape[1]):
            m = int(masks[t, p])
            for j in range(K):
                if m & (1 << j):
                    out[t, p, j] = 1.0
    return out


def unknown_columns(masks, K):
    """[P] bool: the columns whose tips are all unknown, where L_i = 1 and log L_i = 0 exactly."""
    return np.all(np.asarray(masks, np.uint64) == full_mask(K), axis=0)


GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kseq")
NAMES = ("blens", "rates", "freqs", "rs", "ps")


def truth(masks, weights, peel, rooted, blens, rates, freqs, rs, ps, extended=False):
    """(complex log L, complex site log L [P]) at possibly complex parameters."""
    masks = np.asarray(masks, np.uint64)
    S, P = masks.shape
    K = np.asarray(freqs).size
    tips = decode_masks(masks, K).astype(complex)  # [S][P][K]
    t = np.asarray(blens, complex)
    f = np.asarray(freqs, complex)
    Q = build_q(f, rates)
    last = len(peel) - 1
    site_terms = []
    for c in range(len(rs)):
        pm = expm(Q[None] * (t * rs[c])[:, None, None])
        part = {n: tips[n] for n in range(S)}
        logs = np.zeros(P, complex)
        for r, (a, b, p) in enumerate(peel):
            a, b, p = int(a), int(b), int(p)
            va = part[a] @ pm[a].T
            vb = part[b] if (r == last and not rooted) else part[b] @ pm[b].T
            v = va * vb
            if extended:
                m = v[np.arange(P), np.argmax(v.real, axis=1)]
                m = np.where(m == 0, 1.0, m)  # an all-zero column (r_c = 0 at a variable site) stays as it is
                v = v / m[:, None]
                logs = logs + np.log(m)
            part[p] = v
        with np.errstate(divide="ignore"):  # a category without likelihood (r_c = 0 at a variable site): log 0
            site_terms.append((np.log(part[int(peel[-1][2])] @ f) + logs, ps[c]))
    # log sum_c ps_c exp(term_c) about the largest real part
    terms = np.stack([x for x, _ in site_terms])
    pw = np.asarray([w for _, w in site_terms], complex)
    live = np.asarray([abs(w) > 0 for _, w in site_terms])
    with np.errstate(invalid="ignore"):
        top = np.where(live[:, None], terms.real, -np.inf).max(axis=0)
        site = np.log(np.sum(np.where(live[:, None], pw[:, None] * np.exp(terms - top[None, :]), 0.0), axis=0)) + top
    return np.sum(np.asarray(weights) * site), site


class Case:
    """One alignment, tree and parameter point."""

    def __init__(self, name, masks, weights, peel, rooted, blens, rates, freqs, rs, ps, extended=False, through=None):
        self.name = name
        self.masks = np.ascontiguousarray(masks, np.uint64)
        self.weights = np.asarray(weights, float)
        self.peel = np.asarray(peel, np.int32)
        self.rooted = bool(rooted)
        self.args = {"blens": np.asarray(blens, float), "rates": np.asarray(rates, float),
                     "freqs": np.asarray(freqs, float), "rs": np.asarray(rs, float), "ps": np.asarray(ps, float)}
        self.extended = extended
        # codon cases: name -> (value, function value -> rates): the derivative through codon_rates is checked too
        self.through = through or {}
        self.S, self.P = self.masks.shape
        self.K = self.args["freqs"].size
        self.C = self.args["rs"].size
        self.B = num_branches(self.S, rooted)
        self.R = rate_count(self.K)

    @property
    def blens(self):
        return self.args["blens"]

    @property
    def params(self):
        a = self.args
        return np.concatenate([a["rates"], a["freqs"], a["rs"], a["ps"]])

    def split_row(self, row):
        B, C, R, K = self.B, self.C, self.R, self.K
        at = np.cumsum([1, B, C, C, R, K])
        return {"loglik": row[0], "blens": row[1:at[1]], "rs": row[at[1]:at[2]], "ps": row[at[2]:at[3]],
                "rates": row[at[3]:at[4]], "freqs": row[at[4]:at[5]]}

    def f(self, **over):
        a = dict(self.args)
        a.update(over)
        return truth(self.masks, self.weights, self.peel, self.rooted, a["blens"], a["rates"], a["freqs"], a["rs"],
                     a["ps"], extended=self.extended)

    def truth_row(self, only=None):
        """{"loglik", "site", and per array either "name": every entry's
        derivative, or (K >= 20, rates and freqs) "name_dirs": [6, len]
        directions with "name_dd": the directional derivatives}."""
        ll, site = self.f()
        out = {"loglik": float(ll.real), "site": site.real.copy()}
        rng = np.random.default_rng(12345)
        for name in NAMES:
            if only is not None and name not in only:
                continue
            x = self.args[name]
            if self.K >= 20 and name in ("rates", "freqs"):
                dirs = rng.standard_normal((6, x.size))
                if name == "rates":
                    dirs = dirs * (x > 0)  # zero rates stay the structure's zeros
                out[name + "_dirs"] = dirs
                out[name + "_dd"] = np.asarray([self.f(**{name: x + 1j * STEP * d})[0].imag / STEP for d in dirs])
                continue
            g = np.empty(x.size)
            for k in range(x.size):
                z = x.astype(complex)
                z[k] += 1j * STEP
                g[k] = self.f(**{name: z})[0].imag / STEP
            out[name] = g
        for name, (value, fn) in self.through.items():
            out["through_" + name] = self.f(rates=fn(value + 1j * STEP))[0].imag / STEP
        return out


def compare(case, row, site, ref, check_site=True):
    """{quantity: error} of a row against ``truth_row``: log L and site log L
    relative, each gradient array relative to its largest entry (the K = 2
    rate, whose gradient is exactly zero, absolute).  A column whose tips are
    all unknown has log L_i = 0 exactly, where a relative error says nothing:
    those columns alone are compared absolutely, against 0 ("site_unknown")."""
    got = case.split_row(np.asarray(row))
    err = {"loglik": abs(got["loglik"] - ref["loglik"]) / abs(ref["loglik"])}
    if check_site and site is not None:
        unk = unknown_columns(case.masks, case.K)
        if unk.any():
            err["site_unknown"] = float(np.max(np.abs(np.asarray(site)[unk])))
        if not unk.all():
            err["site"] = float(np.max(np.abs(site[~unk] - ref["site"][~unk]) / np.abs(ref["site"][~unk])))
    for name in NAMES:
        if name in ref:
            if name == "rates" and case.K == 2:
                err["rates_abs"] = float(np.max(np.abs(got[name] - ref[name])))
                continue
            err[name] = float(np.max(np.abs(got[name] - ref[name])) / max(np.max(np.abs(ref[name])), 1e-300))
        elif name + "_dd" in ref:
            dd = ref[name + "_dirs"] @ got[name]
            err[name] = float(np.max(np.abs(dd - ref[name + "_dd"])) / max(np.max(np.abs(ref[name + "_dd"])), 1e-300))
    return err


def bars(err):
    """The project's bars: log L and site log L 1e-10 relative, gradients 1e-9
    of the largest entry (1e-12 absolute for the K = 2 rate, as geo's test)."""
    bad = {}
    for k, v in err.items():
        bar = 1e-10 if k in ("loglik", "site", "site_unknown") else 1e-12 if k == "rates_abs" else 1e-9
        if not v <= bar:
            bad[k] = v
    return bad


# ------------------------------------------------------------------ generators
def rooted_peel(S, rng):
    """A random rooted tree's peel: any two live nodes join, root 2S-2."""
    nodes = list(range(S))
    peel = []
    nxt = S
    while len(nodes) > 1:
        i, j = rng.choice(len(nodes), 2, replace=False)
        a, b = nodes[i], nodes[j]
        nodes = [n for k, n in enumerate(nodes) if k not in (i, j)] + [nxt]
        peel.append((int(a), int(b), nxt))
        nxt += 1
    return np.asarray(peel, np.int32)


def random_masks(S, P, K, rng, unknown_column=True):
    """One-hot tips with partial masks, all-unknown tips and (P > 1) one column
    whose tips are all unknown."""
    masks = onehot_masks(rng.integers(0, K, (S, P)))
    extra = onehot_masks(rng.integers(0, K, (S, P)))
    partial = rng.random((S, P)) < 0.15
    masks = np.where(partial, masks | extra, masks)
    masks = np.where(rng.random((S, P)) < 0.1, full_mask(K), masks)
    if unknown_column and P > 1:
        masks[:, P - 1] = full_mask(K)
    return masks.astype(np.uint64)


def random_case(name, S, K, P, C, rooted, seed, caterpillar=False, sparse=False, invariant=False, mean_blen=0.2,
                zero_and_long=False):
    rng = np.random.default_rng(seed)
    if caterpillar:
        peel = caterpillar_peel(S)  # also a valid rooted peel
    else:
        peel = rooted_peel(S, rng) if rooted else random_peel(S, rng)
    B = num_branches(S, rooted)
    masks = random_masks(S, P, K, rng)
    weights = rng.integers(1, 5, P).astype(float)
    blens = rng.exponential(mean_blen, B)
    if zero_and_long:
        blens[0] = 0.0
        blens[B - 1] = 20.0
    rates = 0.1 + rng.exponential(1.0, rate_count(K))
    if sparse:  # the codon pattern: most pairs cannot exchange; a ring keeps the chain connected
        keep = rng.random(rate_count(K)) < 0.15
        for k, (row, col) in enumerate([(r, c) for c in range(K - 1) for r in range(c + 1, K)]):
            if row == col + 1 or (row == K - 1 and col == 0):
                keep[k] = True
        rates = rates * keep
    freqs = rng.dirichlet(np.ones(K) * 3.0)
    rs = np.sort(rng.exponential(1.0, C))
    if invariant:
        rs[0] = 0.0
    ps = rng.dirichlet(np.ones(C) * 4.0)
    return Case(name, masks, weights, peel, rooted, blens, rates, freqs, rs, ps)


def codon_case(name, S, P, C, rooted, seed, kappa, omega, uniform=False, mean_blen=0.2, single_changes=False):
    """K = 61 with the GY94 structure of zeros (``phylostan_amd.codon``)."""
    from phylostan_amd import codon
    rng = np.random.default_rng(seed)
    K = 61
    base = random_case(name, S, K, P, C, rooted, seed, mean_blen=mean_blen)
    x6 = lambda k: np.asarray([1.0, k, 1.0, 1.0, k, 1.0], dtype=np.result_type(k, float))  # noqa: E731
    rates = codon.codon_rates(x6(kappa), omega)
    freqs = np.full(K, 1.0 / K) if uniform else rng.dirichlet(np.ones(K) * 3.0)
    through = {"kappa": (kappa, lambda k: codon.codon_rates(x6(k), omega)),
               "omega": (omega, lambda w: codon.codon_rates(x6(kappa), w))}
    a = base.args
    masks = single_change_masks(base.peel, S, P, K, rates, rng) if single_changes else base.masks
    return Case(name, masks, base.weights, base.peel, rooted, a["blens"], rates, freqs, a["rs"], a["ps"],
                through=through)


def single_change_masks(peel, S, P, K, rates, rng):
    """One-hot tips drawn down the tree from a random root state, a branch in three changing the state once, to
    a state it exchanges with at a positive rate: the data of a tree whose branches are short."""
    ex = np.zeros((K, K), bool)
    pairs = [(r, c) for c in range(K - 1) for r in range(c + 1, K)]
    for k, (r, c) in enumerate(pairs):
        ex[r, c] = ex[c, r] = rates[k] > 0
    states = np.zeros((2 * S - 1, P), np.int64)
    states[2 * S - 2] = rng.integers(0, K, P)
    for a, b, p in np.asarray(peel)[::-1]:
        for ch in (int(a), int(b)):
            for i in range(P):
                s = states[p, i]
                states[ch, i] = rng.choice(np.flatnonzero(ex[s])) if rng.random() < 1.0 / 3.0 else s
    return onehot_masks(states[:S])


def small_cases():
    """The shape list of the engine's tests: K across a full tile, a tile plus
    one, padding of 3 and none; P across the 16-column unit and the 64-pattern
    tile; S in {3, 7}, random and caterpillar, rooted and unrooted; C in {1, 4}
    with and without the +I category; dense and sparse rates; a zero-length and
    a length-20 branch."""
    out = [
        random_case("K2_S3_P1_C1_unrooted", 3, 2, 1, 1, False, 1),
        random_case("K4_S7_P15_C4_rooted_inv", 7, 4, 15, 4, True, 2, invariant=True),
        random_case("K5_S7_P17_C1_cat_unrooted", 7, 5, 17, 1, False, 3, caterpillar=True, zero_and_long=True),
        random_case("K16_S3_P65_C1_rooted", 3, 16, 65, 1, True, 4),
        random_case("K17_S7_P17_C4_unrooted", 7, 17, 17, 4, False, 5),
        random_case("K20_S7_P65_C4_unrooted_sparse_inv", 7, 20, 65, 4, False, 6, sparse=True, invariant=True),
        random_case("K20_S7_P15_C1_cat_rooted", 7, 20, 15, 1, True, 7, caterpillar=True, zero_and_long=True),
        random_case("K64_S3_P17_C4_rooted", 3, 64, 17, 4, True, 8),
        random_case("K64_S7_P1_C1_unrooted_sparse", 7, 64, 1, 1, False, 9, sparse=True),
        codon_case("K61_S7_P17_C4_rooted_codon", 7, 17, 4, True, 10, 5.58, 0.2),
        codon_case("K61_S7_P15_C1_unrooted_ties", 7, 15, 1, False, 11, 1.0, 1.0, uniform=True),
        codon_case("K61_S3_P65_C1_rooted_nearties", 3, 65, 1, True, 12, 1.0 + 1e-9, 1.0, uniform=True),
    ]
    return out


def caterpillar400():
    """A 400-tip caterpillar at K = 20, P = 3: the likelihood leaves the fp64
    range; log L and d/dblens against the extended-range truth."""
    c = random_case("K20_S400_P3_C1_caterpillar", 400, 20, 3, 1, False, 20, caterpillar=True, mean_blen=0.1)
    c.extended = True
    c.masks = random_masks(400, 3, 20, np.random.default_rng(21), unknown_column=False)
    return c


def deep_invariant():
    """A 300-tip caterpillar at K = 20, P = 3, C = 2 with rs[0] = 0: column 0 is constant, the other two vary.  At a
    varying column the +I category's likelihood is exactly 0 with no shift while the live category's shift passes
    the 1023 bits of fp64's exponent: 2^-(shift - shmin) of the dead one is not a number of fp64.  Every array
    against the extended-range truth."""
    c = random_case("K20_S300_P3_C2_caterpillar_deep_inv", 300, 20, 3, 2, False, 50, caterpillar=True, invariant=True,
                    mean_blen=1.0)
    c.extended = True
    masks = random_masks(300, 3, 20, np.random.default_rng(51), unknown_column=False)
    masks[:, 0] = np.uint64(1) << np.uint64(7)
    c.masks = np.ascontiguousarray(masks, np.uint64)
    return c


def edge_cases():
    """Beside ``small_cases`` (whose indices other tests use): branches of length 0 and near 1e-8, where a
    transition probability q t lies beneath the 1e-16 of V V^T - I; short codon branches; the +I category far
    below a deep tree's shift; K of 32 (two full blocks), 33, 40 and 48 (three blocks: KT = 48), 49 (15 padded
    states); C = 16."""
    return [
        random_case("K40_S7_P33_C1_cat_rooted_zero_long", 7, 40, 33, 1, True, 33, caterpillar=True, zero_and_long=True),
        random_case("K20_S7_P17_C4_unrooted_tiny", 7, 20, 17, 4, False, 41, mean_blen=1e-8),
        random_case("K5_S7_P17_C1_rooted_tiny", 7, 5, 17, 1, True, 42, mean_blen=1e-8),
        codon_case("K61_S7_P17_C1_rooted_codon_short", 7, 17, 1, True, 43, 2.5, 0.4, mean_blen=1e-4,
                   single_changes=True),
        deep_invariant(),
        random_case("K32_S7_P17_C1_rooted", 7, 32, 17, 1, True, 44),
        random_case("K33_S7_P17_C4_unrooted_inv", 7, 33, 17, 4, False, 45, invariant=True),
        random_case("K48_S3_P65_C4_unrooted_sparse", 3, 48, 65, 4, False, 46, sparse=True),
        random_case("K49_S3_P17_C1_rooted", 3, 49, 17, 1, True, 47),
        random_case("K4_S3_P17_C16_rooted", 3, 4, 17, 16, True, 48),
    ]


_TRUTHS = {}


def shared_truth(case):
    """One truth per case for every test of a session that needs it; callers leave it unchanged."""
    if case.name not in _TRUTHS:
        _TRUTHS[case.name] = load_truth(case)
    return _TRUTHS[case.name]


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load_truth(case, only=None):
    """The recorded truth of a case (tests/kseq_record_truth.py), or computed."""
    path = golden_path(case.name)
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] if z[k].ndim else float(z[k]) for k in z.files}
    return case.truth_row(only=only)
