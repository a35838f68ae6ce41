"""The exact reference of the K-state mixture engine (M models over sites, C
rate categories each), and the cases its tests share.  numpy only; shares no
algebra with ``phylostan_amd.kseq.kseq_mix_host``: Q_m is built directly
(``geo_oracle.build_q``, normalised by its own s_m), P = expm(Q_m t rs[m][c]) by
scaling and squaring on complex arrays, the pruning is a plain loop over
components, categories and peel rows, the classes are mixed as a log-sum-exp
about the largest term, and each derivative is Im f(theta + 1e-30 i) / 1e-30.
``extended=True`` normalises every internal partial by its largest real part,
pattern by pattern, and carries the logs.

It takes the engine's params ``[rates_0 R][freqs_0 K] .. [rs M C][ps M C]`` and
returns log L, the site log L, every gradient block and the per-class site
log-likelihoods l_im = log sum_c ps[m][c] L_imc, whose exp(l_im - l_i) is the
posterior probability of component m at pattern i.
"""
import os

import numpy as np

from tests.geo_oracle import STEP, build_q, caterpillar_peel, expm
from tests.kseq_truth import (decode_masks, num_branches, random_case, random_masks, rate_count, rooted_peel,
                              unknown_columns)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kseq")


def _category_terms(tips, peel, rooted, t, Q, f, rs, extended):
    """[C][P] complex log L_ic of one component."""
    S, P = tips.shape[0], tips.shape[1]
    last = len(peel) - 1
    out = []
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
                m = np.where(m == 0, 1.0, m)  # an all-zero column stays as it is
                v = v / m[:, None]
                logs = logs + np.log(m)
            part[p] = v
        with np.errstate(divide="ignore"):
            out.append(np.log(part[int(peel[-1][2])] @ f) + logs)
    return np.stack(out)


def _lse(terms, w):
    """log sum_k w_k exp(terms_k) over axis 0, about the largest real part of the live terms; -inf where none is."""
    live = (np.abs(w) > 0)[:, None] & np.isfinite(terms.real)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        top = np.where(live, terms.real, -np.inf).max(axis=0)
        safe = np.where(np.isfinite(top), top, 0.0)
        tot = np.sum(np.where(live, w[:, None] * np.exp(np.where(live, terms, 0.0) - safe[None, :]), 0.0), axis=0)
        return np.where(np.isfinite(top), np.log(np.where(np.isfinite(top), tot, 1.0)) + safe, -np.inf)


def mix_truth(masks, weights, peel, rooted, blens, params, K, M, C, extended=False):
    """(complex log L, complex site log L [P], complex class log L [M][P]) at possibly complex blens / params."""
    masks = np.asarray(masks, np.uint64)
    R = rate_count(K)
    tips = decode_masks(masks, K).astype(complex)
    t = np.asarray(blens, complex)
    p = np.asarray(params, complex)
    rs = p[M * (R + K):M * (R + K) + M * C].reshape(M, C)
    ps = p[M * (R + K) + M * C:].reshape(M, C)
    terms = []
    for m in range(M):
        rates, f = p[m * (R + K):m * (R + K) + R], p[m * (R + K) + R:(m + 1) * (R + K)]
        terms.append(_category_terms(tips, peel, rooted, t, build_q(f, rates), f, rs[m], extended))
    cls = np.stack([_lse(terms[m], ps[m]) for m in range(M)])
    site = _lse(np.concatenate(terms), ps.reshape(-1))
    return np.sum(np.asarray(weights) * site), site, cls


class MixCase:
    """One alignment, tree and parameter point of a mixture."""

    def __init__(self, name, masks, weights, peel, rooted, blens, comps, rs, ps, extended=False):
        self.name = name
        self.masks = np.ascontiguousarray(masks, np.uint64)
        self.weights = np.asarray(weights, float)
        self.peel = np.asarray(peel, np.int32)
        self.rooted = bool(rooted)
        self.blens = np.asarray(blens, float)
        self.rs, self.ps = np.atleast_2d(np.asarray(rs, float)), np.atleast_2d(np.asarray(ps, float))
        self.M, self.C = self.rs.shape
        self.K = np.asarray(comps[0][1]).size
        self.R = rate_count(self.K)
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, rooted)
        self.extended = extended
        self.params = np.concatenate([np.concatenate([np.asarray(r, float), np.asarray(f, float)]) for r, f in comps]
                                     + [self.rs.reshape(-1), self.ps.reshape(-1)])

    def blocks(self):
        """name -> slice of the params; the same names slice the row's gradient after ``row_slices``."""
        R, K, M, G = self.R, self.K, self.M, self.M * self.C
        out = {}
        for m in range(M):
            out["rates%d" % m] = slice(m * (R + K), m * (R + K) + R)
            out["freqs%d" % m] = slice(m * (R + K) + R, (m + 1) * (R + K))
        out["rs"] = slice(M * (R + K), M * (R + K) + G)
        out["ps"] = slice(M * (R + K) + G, M * (R + K) + 2 * G)
        return out

    def split_row(self, row):
        R, K, M, G, B = self.R, self.K, self.M, self.M * self.C, self.B
        out = {"loglik": row[0], "blens": row[1:1 + B], "rs": row[1 + B:1 + B + G], "ps": row[1 + B + G:1 + B + 2 * G]}
        at = 1 + B + 2 * G
        for m in range(M):
            out["rates%d" % m] = row[at + m * (R + K):at + m * (R + K) + R]
            out["freqs%d" % m] = row[at + m * (R + K) + R:at + (m + 1) * (R + K)]
        assert at + M * (R + K) == len(row)
        return out

    def f(self, blens=None, params=None):
        return mix_truth(self.masks, self.weights, self.peel, self.rooted, self.blens if blens is None else blens,
                         self.params if params is None else params, self.K, self.M, self.C, extended=self.extended)

    def truth_row(self, only=None):
        """{"loglik", "site", "class" [M][P] and per array either "name": every entry's derivative, or (K >= 20,
        rates and freqs) "name_dirs": [4, len] directions with "name_dd": the directional derivatives}."""
        ll, site, cls = self.f()
        out = {"loglik": float(ll.real), "site": site.real.copy(), "class": cls.real.copy()}
        rng = np.random.default_rng(54321)
        if only is None or "blens" in only:
            g = np.empty(self.B)
            for k in range(self.B):
                z = self.blens.astype(complex)
                z[k] += 1j * STEP
                g[k] = self.f(blens=z)[0].imag / STEP
            out["blens"] = g
        for name, sl in self.blocks().items():
            if only is not None and name not in only:
                continue
            x = self.params[sl]
            if self.K >= 20 and name[:5] in ("rates", "freqs"):
                dirs = rng.standard_normal((4, x.size))
                if name.startswith("rates"):
                    dirs = dirs * (x > 0)  # zero rates stay the structure's zeros
                dd = []
                for d in dirs:
                    z = self.params.astype(complex)
                    z[sl] += 1j * STEP * d
                    dd.append(self.f(params=z)[0].imag / STEP)
                out[name + "_dirs"], out[name + "_dd"] = dirs, np.asarray(dd)
                continue
            g = np.empty(x.size)
            for k in range(x.size):
                z = self.params.astype(complex)
                z[sl.start + k] += 1j * STEP
                g[k] = self.f(params=z)[0].imag / STEP
            out[name] = g
        return out


def compare(case, row, site, post, ref):
    """{quantity: error} of a row, site log L and class posteriors against ``truth_row``: log L and site log L
    relative (all-unknown columns, where log L_i = log sum ps is 0 or near it, absolutely: "site_unknown"), each gradient array relative
    to its largest entry (an array whose truth is all zero, and the K = 2 rate, absolutely: "*_abs"), the
    posteriors absolutely against exp(l_im - l_i), and their sum over m against 1."""
    got = case.split_row(np.asarray(row))
    err = {"loglik": abs(got["loglik"] - ref["loglik"]) / abs(ref["loglik"])}
    if site is not None:
        unk = unknown_columns(case.masks, case.K)
        if unk.any():
            err["site_unknown"] = float(np.max(np.abs(np.asarray(site)[unk] - ref["site"][unk])))
        if not unk.all():
            err["site"] = float(np.max(np.abs(site[~unk] - ref["site"][~unk]) / np.abs(ref["site"][~unk])))
    if post is not None:
        with np.errstate(invalid="ignore"):
            want = np.where(np.isfinite(ref["class"]), np.exp(ref["class"] - ref["site"][None, :]), 0.0)
        err["class_post"] = float(np.max(np.abs(post - want)))
        err["class_sum"] = float(np.max(np.abs(post.sum(axis=0) - 1.0)))
    for name in ["blens"] + list(case.blocks()):
        if name in ref:
            top = float(np.max(np.abs(ref[name])))
            if top == 0.0 or (name.startswith("rates") and case.K == 2):
                err[name + "_abs"] = float(np.max(np.abs(got[name] - ref[name])))
            else:
                err[name] = float(np.max(np.abs(got[name] - ref[name])) / top)
        elif name + "_dd" in ref:
            dd = ref[name + "_dirs"] @ got[name]
            top = float(np.max(np.abs(ref[name + "_dd"])))
            if top == 0.0:
                err[name + "_abs"] = float(np.max(np.abs(dd)))
            else:
                err[name] = float(np.max(np.abs(dd - ref[name + "_dd"])) / top)
    return err


def bars(err):
    """The project's bars: log L and site log L 1e-10 relative, gradients 1e-9 of the largest entry (1e-12
    absolute where the truth is exactly zero), class posteriors 1e-9 absolute, their sum 1 to 1e-12."""
    bad = {}
    for k, v in err.items():
        bar = (1e-10 if k in ("loglik", "site", "site_unknown") else 1e-12 if k.endswith("_abs") or k == "class_sum"
               else 1e-9)
        if not v <= bar:
            bad[k] = v
    return bad


# ------------------------------------------------------------------ generators
def _component(K, rng, sparse=False):
    c = random_case("x", 3, K, 1, 1, False, int(rng.integers(1 << 30)), sparse=sparse)
    return c.args["rates"], c.args["freqs"]


def random_mix(name, S, K, P, M, C, rooted, seed, caterpillar=False, invariant=False, dead=None, comps=None,
               mean_blen=0.2):
    """Random tree, tips (partial and all-unknown masks, one all-unknown column at P > 1) and M components."""
    rng = np.random.default_rng(seed)
    base = random_case(name, S, K, P, 1, rooted, seed, caterpillar=caterpillar, mean_blen=mean_blen)
    if comps is None:
        comps = [_component(K, rng) for _ in range(M)]
    rs = np.sort(rng.exponential(1.0, (M, C)), axis=1)
    if invariant:
        rs[0, 0] = 0.0
    ps = rng.dirichlet(np.ones(M * C) * 4.0).reshape(M, C)
    if dead is not None:
        ps[dead] = 0.0
    return MixCase(name, base.masks, base.weights, base.peel, rooted, base.blens, comps, rs, ps)


def codon_comps(specs, seed):
    """K = 61 components (kappa, omega, uniform pi?) with the GY94 structure of zeros."""
    from phylostan_amd import codon
    rng = np.random.default_rng(seed)
    out = []
    for kappa, omega, uniform in specs:
        rates = codon.codon_rates(np.asarray([1.0, kappa, 1.0, 1.0, kappa, 1.0]), omega)
        out.append((rates, np.full(61, 1.0 / 61) if uniform else rng.dirichlet(np.ones(61) * 3.0)))
    return out


def small_cases():
    """K in {2, 5, 17, 61} (across a 16-state tile), M in {1, 2, 3}, C in {1, 2} with one rs = 0, P in {1, 15,
    17} (across a 16-pattern tile), S in {3, 7}, rooted and unrooted, partial and all-unknown tips; a component
    whose weights are all 0; the tied codon model (kappa = omega = 1, uniform pi) beside an untied one."""
    return [
        random_mix("K2_S3_P1_M1_C1_unrooted", 3, 2, 1, 1, 1, False, 1),
        random_mix("K5_S7_P15_M2_C2_rooted_inv", 7, 5, 15, 2, 2, True, 2, invariant=True),
        random_mix("K17_S7_P17_M3_C1_unrooted", 7, 17, 17, 3, 1, False, 3),
        random_mix("K5_S3_P17_M3_C2_rooted_dead1", 3, 5, 17, 3, 2, True, 4, dead=1),
        random_mix("K17_S7_P1_M2_C1_cat_rooted", 7, 17, 1, 2, 1, True, 5, caterpillar=True),
        random_mix("K61_S3_P17_M2_C2_unrooted_codon_tied", 3, 61, 17, 2, 2, False, 6,
                   comps=codon_comps([(1.0, 1.0, True), (5.58, 0.2, False)], 6)),
        random_mix("K61_S7_P15_M3_C1_rooted_codon", 7, 61, 15, 3, 1, True, 7,
                   comps=codon_comps([(3.0, 0.1, False), (3.0, 1.0, False), (3.0, 2.5, False)], 7)),
    ]


def edge_cases():
    """Beside ``small_cases``: the limits M = 8 and G = M C = 16 at once."""
    return [random_mix("K5_S3_P17_M8_C2_rooted", 3, 5, 17, 8, 2, True, 8)]


def shifted_caterpillar(S=None):
    """K = 5, P = 3, two components whose rates are a factor 10 apart on a caterpillar deep enough that their
    root shifts differ (``shift_counts``; S = 24 is the smallest multiple of 4 at which every pattern's do: the
    slow component is rescaled once, by 2^67 to 2^71, the fast one never).  The weights are set so that the two
    posteriors are of the same order.  Log L, d/dblens, d/drs, d/dps and the posteriors against the
    extended-range truth recorded by tests/kseq_mix_record_truth.py."""
    S = 24 if S is None else S
    rng = np.random.default_rng(31)
    base = random_case("x", S, 5, 3, 1, False, 30, caterpillar=True, mean_blen=0.15)
    masks = random_masks(S, 3, 5, np.random.default_rng(32), unknown_column=False)
    rates, freqs = _component(5, rng)
    case = MixCase("K5_S%d_P3_M2_C1_shifted_caterpillar" % S, masks, base.weights, caterpillar_peel(S), False,
                   base.blens, [(rates, freqs), (rates, freqs)], [[0.3], [3.0]], [[1.0 - 1e-7], [1e-7]], extended=True)
    return case


def shift_counts(case):
    """[G][P] total power-of-two shifts of the engine's rescaling rule (a column below 2^-64 is brought to [1, 2)),
    by plain real pruning: what the test asserts differs between the components."""
    K, M, C, R = case.K, case.M, case.C, case.R
    tips = decode_masks(case.masks, K)
    out = np.zeros((M * C, case.P))
    last = len(case.peel) - 1
    for m in range(M):
        p = case.params[m * (R + K):(m + 1) * (R + K)]
        Q = build_q(p[R:], p[:R])
        for c in range(C):
            pm = expm(Q[None] * (case.blens * case.rs[m, c]).astype(complex)[:, None, None]).real
            part = {n: tips[n] for n in range(case.S)}
            for r, (a, b, pa) in enumerate(case.peel):
                a, b, pa = int(a), int(b), int(pa)
                v = (part[a] @ pm[a].T) * (part[b] if (r == last and not case.rooted) else part[b] @ pm[b].T)
                mx = v.max(axis=1)
                sh = np.where((mx > 0) & (mx < 2.0 ** -64), -np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 0.0)
                part[pa] = v * np.exp2(sh)[:, None]
                out[m * C + c] += sh
    return out


def golden_path(name):
    return os.path.join(GOLDEN, name + ".npz")


def load_truth(case, only=None):
    """The recorded truth of a case (tests/kseq_mix_record_truth.py), or computed."""
    path = golden_path(case.name)
    if os.path.exists(path):
        with np.load(path) as z:
            return {k: z[k] if z[k].ndim else float(z[k]) for k in z.files}
    return case.truth_row(only=only)


_TRUTHS = {}


def shared_truth(case):
    """One truth per case for every test of a session that needs it; callers leave it unchanged."""
    if case.name not in _TRUTHS:
        _TRUTHS[case.name] = load_truth(case)
    return _TRUTHS[case.name]
