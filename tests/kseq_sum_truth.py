"""The exact reference of the K-state engine's posterior summaries, and the
cases their tests share.  numpy only, built on ``tests/kseq_mix_truth.py`` and
``tests/geo_oracle.py``; it shares no algebra with ``phylostan_amd.kseq``: there
is no eigensystem, no way down and no Phi here.

``node_post[v - S][j][i]``: the tree is pruned once per (node, state) with that
node's partial masked to the state; the value is L_i(masked) / L_i, taken on the
logs (``extended=True`` carries them through a deep tree).

``bcounts[l][b]``: the complex-step derivative Im f(1e-30 i) / 1e-30 of log L,
where branch b alone runs under expm((Q_m + eps offdiag(Q_m o lab_l)) t_b r_g),
the diagonal not compensated.  That derivative is sum_i w_i / L_i times the
column's int_0^t P(s) (Q o lab) P(t - s) ds between the branch's two ends: the
expected number of labelled substitutions on the branch.
"""
import numpy as np

from tests.geo_oracle import STEP, build_q, caterpillar_peel, expm
from tests.kseq_mix_truth import MixCase, _lse, codon_comps, random_mix
from tests.kseq_truth import decode_masks, random_masks, rate_count, single_change_masks

LN2 = np.log(2.0)


def label_matrix(K, lab):
    """[K][K] symmetric with zero diagonal: the pair k of the rates' order (the strict lower triangle column by
    column) at (row, col) and (col, row)."""
    out = np.zeros((K, K))
    k = 0
    for col in range(K - 1):
        for row in range(col + 1, K):
            out[row, col] = out[col, row] = lab[k]
            k += 1
    return out


def _prune(tips, peel, rooted, pm, f, extended, node=None, state=None):
    """Complex log L_i [P] of one (component, category) with the matrices ``pm [B]``; ``node``'s partial is
    masked to ``state`` when given."""
    S, P = tips.shape[0], tips.shape[1]
    last = len(peel) - 1
    part = {n: tips[n] for n in range(S)}
    logs = np.zeros(P, complex)
    for r, (a, b, p) in enumerate(peel):
        a, b, p = int(a), int(b), int(p)
        va = part[a] @ pm[a].T
        vb = part[b] if (r == last and not rooted) else part[b] @ pm[b].T
        v = va * vb
        if p == node:
            keep = np.zeros(v.shape[1])
            keep[state] = 1.0
            v = v * keep[None, :]
        if extended:
            m = v[np.arange(P), np.argmax(v.real, axis=1)]
            m = np.where(m == 0, 1.0, m)
            v = v / m[:, None]
            logs = logs + np.log(m)
        part[p] = v
    with np.errstate(divide="ignore"):
        return np.log(part[int(peel[-1][2])] @ f) + logs


class SumCase:
    """A ``MixCase`` with its labellings ``labels [NL][R]``."""

    def __init__(self, mix, labels):
        self.mix = mix
        self.name = mix.name + "_L%d" % len(labels)
        self.labels = np.ascontiguousarray(labels, float)
        self.NL = self.labels.shape[0]
        for k in ("masks", "weights", "peel", "rooted", "blens", "params", "K", "M", "C", "S", "P", "B", "R",
                  "extended"):
            setattr(self, k, getattr(mix, k))

    def _models(self):
        K, M, C, R = self.K, self.M, self.C, self.R
        p = self.params
        rs = p[M * (R + K):M * (R + K) + M * C].reshape(M, C)
        ps = p[M * (R + K) + M * C:].reshape(M, C)
        out = []
        for m in range(M):
            rates, f = p[m * (R + K):m * (R + K) + R], p[m * (R + K) + R:(m + 1) * (R + K)]
            out.append((build_q(f, rates), f.astype(complex)))
        return out, rs, ps

    def truth(self):
        """{"loglik", "site" [P], "node_post" [S-1][K][P], "bcounts" [NL][B]}."""
        K, M, C, S, P, B = self.K, self.M, self.C, self.S, self.P, self.B
        tips = decode_masks(self.masks, K).astype(complex)
        t = self.blens.astype(complex)
        models, rs, ps = self._models()
        psf = ps.reshape(-1)
        pms = [[expm(models[m][0][None] * (t * rs[m, c])[:, None, None]) for c in range(C)] for m in range(M)]

        def site_of(pm_of, node=None, state=None):
            terms = [_prune(tips, self.peel, self.rooted, pm_of(m, c), models[m][1], self.extended, node, state)
                     for m in range(M) for c in range(C)]
            return _lse(np.stack(terms), psf)

        site = site_of(lambda m, c: pms[m][c])
        w = self.weights
        with np.errstate(invalid="ignore"):
            ll = np.sum(np.where(w > 0, w * np.where(w > 0, site, 0.0), 0.0))
        out = {"loglik": float(ll.real), "site": site.real.copy()}
        npost = np.zeros((S - 1, K, P))
        for v in range(S, 2 * S - 1):
            for j in range(K):
                sm = site_of(lambda m, c: pms[m][c], v, j)
                with np.errstate(invalid="ignore", over="ignore"):
                    npost[v - S, j] = np.where(np.isfinite(sm.real) & np.isfinite(site.real),
                                               np.exp((sm - site).real), 0.0)
        out["node_post"] = npost
        bc = np.zeros((self.NL, B))
        for l in range(self.NL):
            LM = label_matrix(K, self.labels[l])
            for b in range(B):
                def pm_of(m, c):
                    Q = models[m][0]
                    Ql = Q * LM  # LM's diagonal is 0: the off-diagonal entries alone, the diagonal not compensated
                    one = expm(((Q + 1j * STEP * Ql) * (t[b] * rs[m, c]))[None])[0]
                    pm = pms[m][c].copy()
                    pm[b] = one
                    return pm
                sb = site_of(pm_of)
                with np.errstate(invalid="ignore"):
                    bc[l, b] = np.sum(np.where(w > 0, w * np.where(w > 0, sb, 0.0), 0.0)).imag / STEP
        out["bcounts"] = bc
        return out


def compare(case, ll, bc, npost, ref):
    """{quantity: error}: log L relative, node_post absolute and its sum over the states against 1 wherever the
    column has a likelihood, bcounts relative to the array's largest entry (absolute where the truth is all 0)."""
    err = {"loglik": abs(ll - ref["loglik"]) / abs(ref["loglik"]) if ref["loglik"] != 0 else abs(ll)}
    if npost is not None:
        err["node_post"] = float(np.max(np.abs(npost - ref["node_post"])))
        has = np.isfinite(ref["site"])
        err["node_sum"] = float(np.max(np.abs(npost.sum(axis=1)[:, has] - 1.0))) if has.any() else 0.0
    top = float(np.max(np.abs(ref["bcounts"])))
    if top == 0.0:
        err["bcounts_abs"] = float(np.max(np.abs(bc)))
    else:
        err["bcounts"] = float(np.max(np.abs(bc - ref["bcounts"])) / top)
    return err


def bars(err):
    """The project's bars against the truth: log L 1e-10 relative, node_post 1e-9 absolute (class_post's),
    bcounts 1e-9 of the array's largest entry (exactly 0 where the truth is all 0).  "node_sum" is an invariant
    of the engine, not a distance from the truth: the invariants' test holds it to ``SUM_BAR``."""
    bar = {"loglik": 1e-10, "node_post": 1e-9, "bcounts": 1e-9, "bcounts_abs": 0.0}
    return {k: v for k, v in err.items() if k in bar and not v <= bar[k]}


SUM_BAR = 1e-12  # every (node, pattern) of node_post sums to one over the states


# ------------------------------------------------------------------ cases
def dense_labels(K, NL, seed):
    return np.random.default_rng(seed).exponential(1.0, (NL, rate_count(K)))


def _codon_labels():
    from phylostan_amd import codon
    return codon.codon_labels()


def _short_tips(mix, seed):
    """One-hot tips drawn down the tree with single changes: the data of a tree whose branches are short."""
    rates = mix.params[:mix.R]
    masks = single_change_masks(mix.peel, mix.S, mix.P, mix.K, rates, np.random.default_rng(seed))
    return MixCase(mix.name, masks, mix.weights, mix.peel, mix.rooted, mix.blens,
                   [(mix.params[m * (mix.R + mix.K):m * (mix.R + mix.K) + mix.R],
                     mix.params[m * (mix.R + mix.K) + mix.R:(m + 1) * (mix.R + mix.K)]) for m in range(mix.M)],
                   mix.rs, mix.ps)


def small_cases():
    """K in {2, 5, 17, 33, 61, 64}; P in {1, 15, 17}; S in {3, 7}, random and caterpillar, rooted and unrooted;
    (M, C) in {(1, 1), (1, 4) with rs_0 = 0, (3, 1), (2, 4)}; 1, 2 and 4 labellings, dense except the codon
    pair; a zero-length branch beside one of length 20; every branch near 1e-8 at K = 5 on single-change tips; a
    column of unknowns (the last, at P > 1) and a column of weight zero."""
    out = []
    out.append(SumCase(random_mix("sum_K2_S3_P1_M1_C1_unrooted", 3, 2, 1, 1, 1, False, 101), dense_labels(2, 1, 1)))
    m = random_mix("sum_K5_S7_P15_M1_C4_rooted_inv_zero_long", 7, 5, 15, 1, 4, True, 102, invariant=True)
    m.blens[0], m.blens[m.B - 1] = 0.0, 20.0
    m.weights[3] = 0.0
    out.append(SumCase(m, dense_labels(5, 2, 2)))
    m = _short_tips(random_mix("sum_K5_S7_P17_M3_C1_cat_unrooted_tiny", 7, 5, 17, 3, 1, False, 103, caterpillar=True,
                               mean_blen=1e-8), 113)
    out.append(SumCase(m, dense_labels(5, 4, 3)))
    m = random_mix("sum_K17_S7_P17_M2_C4_unrooted", 7, 17, 17, 2, 4, False, 104)
    m.weights[0] = 0.0
    out.append(SumCase(m, dense_labels(17, 2, 4)))
    out.append(SumCase(random_mix("sum_K17_S7_P1_M3_C1_cat_rooted", 7, 17, 1, 3, 1, True, 105, caterpillar=True),
                       dense_labels(17, 1, 5)))
    m = random_mix("sum_K33_S3_P15_M1_C1_rooted_zero_long", 3, 33, 15, 1, 1, True, 106)
    m.blens[1], m.blens[m.B - 1] = 0.0, 20.0
    out.append(SumCase(m, dense_labels(33, 4, 6)))
    m = random_mix("sum_K61_S7_P17_M3_C1_rooted_codon", 7, 61, 17, 3, 1, True, 107,
                   comps=codon_comps([(3.0, 0.1, False), (3.0, 1.0, False), (3.0, 2.5, False)], 107))
    m.weights[5] = 0.0
    out.append(SumCase(m, _codon_labels()))
    out.append(SumCase(random_mix("sum_K64_S3_P17_M1_C4_unrooted_inv", 3, 64, 17, 1, 4, False, 108, invariant=True),
                       dense_labels(64, 1, 8)))
    return out


def tied_codon():
    """kappa = omega = 1 with uniform frequencies: eigenvalues of high multiplicity, Phi's tie arm throughout."""
    m = random_mix("sum_K61_S7_P17_M1_C1_unrooted_codon_tied", 7, 61, 17, 1, 1, False, 109,
                   comps=codon_comps([(1.0, 1.0, True)], 109))
    return SumCase(m, _codon_labels())


def deep_caterpillar(S=40):
    """A 40-tip caterpillar at K = 20, P = 3, C = 2 with rs_0 = 0 and long branches: the partials of the
    varying columns are rescaled more than once on the way up (``kseq_mix_truth.shift_counts``: 132 and 136
    bits); against the extended-range truth."""
    m = random_mix("sum_K20_S%d_P3_M1_C2_caterpillar_deep_inv" % S, S, 20, 3, 1, 2, False, 110, caterpillar=True,
                   invariant=True, mean_blen=1.0)
    masks = random_masks(S, 3, 20, np.random.default_rng(111), unknown_column=False)
    masks[:, 0] = np.uint64(1) << np.uint64(7)  # a constant column: the +I category is alive there
    m = MixCase(m.name, masks, m.weights, caterpillar_peel(S), False, m.blens,
                [(m.params[:m.R], m.params[m.R:m.R + m.K])], m.rs, m.ps, extended=True)
    return SumCase(m, dense_labels(20, 2, 10))


_TRUTHS = {}


def shared_truth(case):
    """One truth per case for every test of a session that needs it; callers leave it unchanged."""
    if case.name not in _TRUTHS:
        _TRUTHS[case.name] = case.truth()
    return _TRUTHS[case.name]
