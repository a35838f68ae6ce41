"""Codon models (GY94 / MG94 style) on the K-state sequence engine.

The alignment is read as triplets of the universal genetic code: K = 61 sense
codons in TCAG order.  Q_ij = 0 for codons differing at more than one
position, otherwise the nucleotide exchangeability of the differing pair, times
omega (dN / dS) if the amino acids differ, times pi_j; normalised to ONE
EXPECTED SUBSTITUTION PER CODON per unit of branch length (the engine's s), so
branch lengths are three times those of a nucleotide model on the same data in
substitutions per nucleotide site.

``-m HKY`` gives the exchangeabilities (1, kappa, 1, 1, kappa, 1) -- GY94 --,
``-m GTR`` the six ``rates``, ``-m JC69`` all ones.  Codon frequencies
(``--codon_freqs``): ``F3x4`` (three position-specific nucleotide simplexes),
``F1x4`` (one), ``F61`` (fixed at the observed counts plus one each); pi_j is
the product of its positions' nucleotide frequencies over one minus the stop
mass.

Site models (``--codon_sites``, ``CodonSitesPosterior``): omega varies over
sites as a mixture of M classes with proportions ``pclass``, ``M1a`` (omega0 <
1, omega1 = 1), ``M2a`` (M1a and omega2 > 1) and ``M3:k`` (k free, ordered
omegas), on the K-state mixture engine (``kseq.kseq_mix_host``); Q is
normalised so that the MEAN rate over the classes is one substitution per
codon.
"""
import math

import numpy as np

from .geo import rate_count, rate_pairs
from .posterior import Posterior, _Param
from .transforms import Lower, Simplex, Unit

BASES = "TCAG"
_AMINO = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
CODONS64 = [a + b + c for a in BASES for b in BASES for c in BASES]
SENSE = [i for i in range(64) if _AMINO[i] != "*"]          # index into CODONS64 of every sense codon
STOPS = [i for i in range(64) if _AMINO[i] == "*"]
CODONS = [CODONS64[i] for i in SENSE]
AMINO = [_AMINO[i] for i in SENSE]
K = len(SENSE)  # 61
FREQ_MODELS = ("F3x4", "F1x4", "F61")

_IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "U": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT",
          "M": "AC", "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT", "-": "ACGT", "?": "ACGT",
          ".": "ACGT", "X": "ACGT"}
# 4-bit sets over TCAG of every byte (0: not a nucleotide symbol)
_SETS = np.zeros(256, np.uint8)
for _sym, _bases in _IUPAC.items():
    _bits = sum(1 << BASES.index(b) for b in _bases)
    _SETS[ord(_sym)] = _bits
    _SETS[ord(_sym.lower())] = _bits
_SENSE_OF64 = np.full(64, -1, np.int64)
_SENSE_OF64[SENSE] = np.arange(K)

# x6 entry (AC AG AT CG CT GT) of a pair of different bases
_X6 = {frozenset("AC"): 0, frozenset("AG"): 1, frozenset("AT"): 2, frozenset("CG"): 3, frozenset("CT"): 4,
       frozenset("GT"): 5}


def _pair_tables():
    pairs = rate_pairs(K)
    which = np.full(len(pairs), -1, np.int64)
    nonsyn = np.zeros(len(pairs), bool)
    for k, (row, col) in enumerate(pairs):
        a, b = CODONS[row], CODONS[col]
        diff = [p for p in range(3) if a[p] != b[p]]
        if len(diff) == 1:
            which[k] = _X6[frozenset((a[diff[0]], b[diff[0]]))]
            nonsyn[k] = AMINO[row] != AMINO[col]
    return which, nonsyn


_WHICH, _NONSYN = _pair_tables()
_LIVE = _WHICH >= 0
_ACGT_OF_TCAG = np.asarray([3, 1, 0, 2])  # index into (A, C, G, T) of T, C, A, G


def codon_rates(x6, omega):
    """``rates[R]`` (or ``[n, R]`` for ``x6 [n, 6]``, ``omega [n]``) of the
    K-state engine, R = 61 * 60 / 2 in ``geo.rate_pairs`` order."""
    x6 = np.asarray(x6)
    om = np.asarray(omega)
    base = x6[..., np.where(_LIVE, _WHICH, 0)]
    scale = np.where(_NONSYN, om[..., None], np.ones_like(om)[..., None])
    return np.where(_LIVE, base * scale, 0.0)


def codon_labels():
    """``[2, R]`` 0 / 1 labellings of the codon pairs in ``geo.rate_pairs`` order, for the K-state summaries
    (``kseq.kseq_sum_host``): row 0 synonymous (one nucleotide differs, the same amino acid), row 1
    nonsynonymous (one nucleotide differs, another amino acid).  Together the 263 live pairs, each once."""
    return np.stack([_LIVE & ~_NONSYN, _LIVE & _NONSYN]).astype(float)


def neutral_rates(x6, pi):
    """``(rho_S, rho_N)``: the synonymous and the nonsynonymous flux sum_i pi_i sum_j Q_ij lab_ij of the
    unnormalised Q at omega = 1 (``[n]`` each for ``x6 [n, 6]``, ``pi [n, 61]``).  Their ratio is what dN / dS
    divides the observed N / S by; Q's normalisation cancels in it."""
    x6, pi = np.asarray(x6, float), np.asarray(pi, float)
    rates = codon_rates(x6, np.ones(x6.shape[:-1]))
    flux = 2.0 * rates * pi[..., _PAIRS[:, 0]] * pi[..., _PAIRS[:, 1]]  # pi_i r_ij pi_j, both directions
    lab = codon_labels()
    return (flux * lab[0]).sum(axis=-1), (flux * lab[1]).sum(axis=-1)


def codon_rates_backward(x6, omega, g_rates):
    """The transpose of ``codon_rates``' Jacobian: g_rates -> (g_x6, g_omega)."""
    x6 = np.asarray(x6, float)
    om = np.asarray(omega, float)
    g = np.asarray(g_rates, float)
    scale = np.where(_NONSYN, om[..., None], 1.0)
    gs = np.where(_LIVE, g * scale, 0.0)
    g_x6 = np.stack([gs[..., _WHICH == k].sum(axis=-1) for k in range(6)], axis=-1)
    base = x6[..., np.where(_LIVE, _WHICH, 0)]
    g_om = np.where(_LIVE & _NONSYN, g * base, 0.0).sum(axis=-1)
    return g_x6, g_om


def position_frequencies(f1, f2, f3):
    """pi [n, 61] of nucleotide frequencies [n, 4] (A, C, G, T) per position."""
    t = [np.asarray(f)[..., _ACGT_OF_TCAG] for f in (f1, f2, f3)]
    u = (t[0][..., :, None, None] * t[1][..., None, :, None] * t[2][..., None, None, :])
    u = u.reshape(u.shape[:-3] + (64,))
    stop = u[..., STOPS].sum(axis=-1)
    return u[..., SENSE] / (1.0 - stop)[..., None]


def position_frequencies_backward(f1, f2, f3, g_pi):
    """g_pi [n, 61] -> (g_f1, g_f2, g_f3) [n, 4] each (A, C, G, T)."""
    t = [np.asarray(f, float)[..., _ACGT_OF_TCAG] for f in (f1, f2, f3)]
    u = (t[0][..., :, None, None] * t[1][..., None, :, None] * t[2][..., None, None, :])
    flat = u.reshape(u.shape[:-3] + (64,))
    live = 1.0 - flat[..., STOPS].sum(axis=-1)
    g_u = np.zeros(flat.shape)
    g_u[..., SENSE] = g_pi / live[..., None]
    g_u[..., STOPS] = ((g_pi * flat[..., SENSE]).sum(axis=-1) / live ** 2)[..., None]
    g_u = g_u.reshape(u.shape)
    g = [(g_u * t[1][..., None, :, None] * t[2][..., None, None, :]).sum(axis=(-1, -2)),
         (g_u * t[0][..., :, None, None] * t[2][..., None, None, :]).sum(axis=(-1, -3)),
         (g_u * t[0][..., :, None, None] * t[1][..., None, :, None]).sum(axis=(-2, -3))]
    out = []
    for gt in g:
        ga = np.zeros(gt.shape)
        ga[..., _ACGT_OF_TCAG] = gt
        out.append(ga)
    return tuple(out)


def triplet_mask(triplet):
    """The uint64 mask of the sense codons compatible with three IUPAC symbols;
    ValueError for a symbol that is no nucleotide code, 0 if only stop codons fit."""
    sets = []
    for ch in triplet:
        s = int(_SETS[ord(ch)]) if len(ch) == 1 and ord(ch) < 256 else 0
        if s == 0:
            raise ValueError("%r is not a nucleotide symbol" % ch)
        sets.append(s)
    return _mask_of_sets(*sets)


def _mask_of_sets(s1, s2, s3):
    m = 0
    for a in range(4):
        if not (s1 >> a) & 1:
            continue
        for b in range(4):
            if not (s2 >> b) & 1:
                continue
            for c in range(4):
                if (s3 >> c) & 1:
                    j = _SENSE_OF64[16 * a + 4 * b + c]
                    if j >= 0:
                        m |= 1 << int(j)
    return m


def codon_alignment(chars, taxa=None):
    """``chars uint8 [S, sites]`` (upper-case symbols) read as codons in frame
    0: ``(tipmasks uint64 [S, P], weights [P], codon_pattern int64 [codons])``.
    Codon columns are deduplicated on their raw symbols in first-seen order with
    weights = counts, as the nucleotide path does.  Gaps and ``N`` mean all four
    nucleotides.  ValueError, naming taxon and site (1-based nucleotide
    position), for a length that is no multiple of 3, an in-frame stop codon, a
    triplet compatible only with stop codons, or a symbol that is no nucleotide
    code."""
    chars = np.ascontiguousarray(chars, np.uint8)
    S, L = chars.shape
    name = (lambda t: str(taxa[t])) if taxa is not None else (lambda t: "taxon %d" % (t + 1))
    if L % 3 != 0 or L == 0:
        raise ValueError("codon alignment: the length %d is not a multiple of 3" % L)
    n = L // 3
    cols = np.ascontiguousarray(chars.reshape(S, n, 3).transpose(1, 0, 2)).reshape(n, S * 3)
    view = cols.view(np.dtype((np.void, S * 3)))[:, 0]
    _, first, inverse, counts = np.unique(view, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(first, kind="stable")
    first_sorted = first[order]
    weights = counts[order].astype(np.float64)
    rank = np.empty(order.size, np.int64)
    rank[order] = np.arange(order.size)
    sets = _SETS[chars]
    if np.any(sets == 0):
        t, s = np.argwhere(sets == 0)[0]
        raise ValueError("codon alignment: %s site %d: %r is not a nucleotide symbol" % (name(t), s + 1, chr(chars[t, s])))
    trip = sets.reshape(S, n, 3)[:, first_sorted, :]
    keys = (trip[..., 0].astype(np.int64) << 8) | (trip[..., 1].astype(np.int64) << 4) | trip[..., 2].astype(np.int64)
    table = {}
    masks = np.empty(keys.shape, np.uint64)
    for t in range(S):
        for p in range(keys.shape[1]):
            k = int(keys[t, p])
            m = table.get(k)
            if m is None:
                m = table[k] = _mask_of_sets(k >> 8, (k >> 4) & 15, k & 15)
            if m == 0:
                site = int(first_sorted[p]) * 3 + 1
                tri = bytes(chars[t, site - 1:site + 2]).decode("ascii")
                what = "an in-frame stop codon" if all(bin(v).count("1") == 1 for v in (k >> 8, (k >> 4) & 15, k & 15)) \
                    else "compatible only with stop codons"
                raise ValueError("codon alignment: %s site %d: %s is %s" % (name(t), site, tri, what))
            masks[t, p] = m
    return masks, weights, rank[np.asarray(inverse).reshape(-1)]


def codon_counts(masks, weights):
    """Observed counts [61] of the unambiguous codons of an alignment."""
    m = np.asarray(masks, np.uint64)
    counts = np.zeros(K)
    for j in range(K):
        counts[j] = ((m == np.uint64(1 << j)) * np.asarray(weights)[None, :]).sum()
    return counts


class CodonPosterior(Posterior):
    """``Posterior`` with a codon substitution model: the tree, clock,
    coalescent, speciation and site-rate parts are ``Posterior``'s own.  Its
    likelihood is a K-state sequence likelihood (``kseq.HostKStateLikelihood``
    on ``kseq_host``): ``evaluate_rows(blens [n, B], params [n, R + 61 + 2C])``.

    Parameters: ``kappa`` (HKY, its nucleotide prior) or ``rates`` Simplex(6)
    (GTR), ``omega`` Lower(0) ~ lognormal(-1, 1.25), and the frequency
    simplexes ``freqs_pos1..3`` (F3x4) or ``freqs`` (F1x4), dirichlet(1); F61
    fixes pi at ``counts`` + 1.  The native strict-clock fast path is not used."""

    def __init__(self, spec, tree, likelihood, codon_freqs="F3x4", counts=None):
        if codon_freqs not in FREQ_MODELS:
            raise ValueError("codon_freqs must be one of %s" % ", ".join(FREQ_MODELS))
        self.codon_freqs = codon_freqs
        self.K = K
        self.R = rate_count(K)
        if codon_freqs == "F61":
            if counts is None:
                raise ValueError("F61 needs the observed codon counts")
            c = np.asarray(counts, float) + 1.0
            self.fixed_pi = c / c.sum()
        super().__init__(spec, tree, likelihood, compact_rows=False)

    def _native_strict(self):
        return None

    def _declare_subst(self, suffix=""):
        sp = self.spec
        P = []
        if sp.model == "GTR":
            P.append(_Param("rates", Simplex(6)))
        elif sp.model == "HKY":
            P.append(_Param("kappa", Lower(0.0)))
        P.append(_Param("omega", Lower(0.0)))
        if self.codon_freqs == "F3x4":
            P += [_Param("freqs_pos%d" % k, Simplex(4)) for k in (1, 2, 3)]
        elif self.codon_freqs == "F1x4":
            P.append(_Param("freqs", Simplex(4)))
        return P

    def _dropped_constants(self):
        c = Posterior._dropped_constants(self)
        if self.spec.model in ("GTR", "HKY"):
            c -= math.lgamma(4.0)  # the nucleotide model's one freqs ~ dirichlet(1, 1, 1, 1)
        c += {"F3x4": 3, "F1x4": 1, "F61": 0}[self.codon_freqs] * math.lgamma(4.0)
        return c - math.log(1.25) - 0.5 * math.log(2.0 * math.pi)  # omega ~ lognormal(-1, 1.25)

    # ------------------------------------------------------------ the pieces
    def _x6(self, vals, n):
        sp = self.spec
        if sp.model == "GTR":
            return vals["rates"]
        x = np.ones((n, 6))
        if sp.model == "HKY":
            x[:, 1] = vals["kappa"]
            x[:, 4] = vals["kappa"]
        return x

    def _position_freqs(self, vals):
        if self.codon_freqs == "F3x4":
            return vals["freqs_pos1"], vals["freqs_pos2"], vals["freqs_pos3"]
        return vals["freqs"], vals["freqs"], vals["freqs"]

    def codon_frequencies(self, vals, n):
        """pi [n, 61]."""
        if self.codon_freqs == "F61":
            return np.repeat(self.fixed_pi[None, :], n, axis=0)
        return position_frequencies(*self._position_freqs(vals))

    def _row_width(self):
        return 1 + self.B + 2 * self.C + self.R + self.K

    def _subst_forward(self, vals, n):
        x6 = self._x6(vals, n)
        rates = codon_rates(x6, vals["omega"])
        pi = self.codon_frequencies(vals, n)
        rs, ps = self._site_rates(vals, n)
        with np.errstate(invalid="ignore"):
            positive = np.all(pi > 0, axis=1)
        return np.concatenate([rates, pi, rs, ps], axis=1), positive, (rs, ps, x6)

    def _lik_rows(self, blens, mv, tags=None):
        if tags is not None:
            raise ValueError("tags: a codon likelihood has one tree")
        return self.lik.evaluate_rows(blens, mv)

    def _subst_prior(self, vals, lp, gx):
        lp = Posterior._subst_prior(self, vals, lp, gx)  # wshape, and kappa's with -m HKY
        w = vals["omega"]
        lw = np.log(w)
        lp = lp - lw - (lw + 1.0) ** 2 / (2.0 * 1.25 ** 2)
        gx["omega"] += -1.0 / w - (lw + 1.0) / (1.25 ** 2 * w)
        return lp

    def _subst_backward(self, vals, rows, bad, gx, sub):
        sp = self.spec
        C = self.C
        rs, ps, x6 = sub
        o = 1 + self.B + 2 * C
        g_rs = rows[:, 1 + self.B:1 + self.B + C]
        g_ps = rows[:, 1 + self.B + C:o]
        good = np.nonzero(~bad)[0]
        if len(good):
            g_x6, g_om = codon_rates_backward(x6[good], vals["omega"][good], rows[good, o:o + self.R])
            gx["omega"][good] += g_om
            if sp.model == "GTR":
                gx["rates"][good] += g_x6
            elif sp.model == "HKY":
                gx["kappa"][good] += g_x6[:, 1] + g_x6[:, 4]
            if self.codon_freqs != "F61":
                f = [v[good] for v in self._position_freqs(vals)]
                g1, g2, g3 = position_frequencies_backward(f[0], f[1], f[2], rows[good, o + self.R:o + self.R + self.K])
                if self.codon_freqs == "F3x4":
                    gx["freqs_pos1"][good] += g1
                    gx["freqs_pos2"][good] += g2
                    gx["freqs_pos3"][good] += g3
                else:
                    gx["freqs"][good] += g1 + g2 + g3
        self._site_rates_backward(vals, g_rs, g_ps, gx, rs, ps)

    # ------------------------------------------------------------------ output
    def model_vectors(self, U):
        """The engine's params [n, R + 61 + 2C] of draws U."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        vals, _, _ = self.constrain(U)
        return self._subst_forward(vals, U.shape[0])[0]

    def nucleotide_rates(self, U):
        """The six nucleotide exchangeabilities ``x6 [n, 6]`` (AC AG AT CG CT GT) of draws U."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        vals, _, _ = self.constrain(U)
        return np.asarray(self._x6(vals, U.shape[0]), float)

    def codon_summary(self, U):
        """{"omega": [n], "kappa": [n] or "rates": [n, 6] (as the model has them), "pi": [n, 61]} of draws U."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        vals, _, _ = self.constrain(U)
        out = {"omega": vals["omega"], "pi": self.codon_frequencies(vals, U.shape[0])}
        for name in ("kappa", "rates"):
            if name in vals:
                out[name] = vals[name]
        return out


def write_codon_tsv(path, summary):
    """OUT.codon.tsv: the mean and 95 % interval of omega (with a site model: of every class's omega and
    proportion), kappa or the six rates, and the 61 codon frequencies over the draws."""
    if "omegas" in summary:
        M = summary["omegas"].shape[1]
        rows = [("omega.%d" % (m + 1), summary["omegas"][:, m]) for m in range(M)]
        rows += [("pclass.%d" % (m + 1), summary["pclass"][:, m]) for m in range(M)]
    else:
        rows = [("omega", summary["omega"])]
    if "kappa" in summary:
        rows.append(("kappa", summary["kappa"]))
    if "rates" in summary:
        rows += [("rates.%s" % n, summary["rates"][:, k]) for k, n in enumerate(("AC", "AG", "AT", "CG", "CT", "GT"))]
    rows += [("pi.%s" % CODONS[j], summary["pi"][:, j]) for j in range(K)]
    with open(path, "w") as fp:
        fp.write("parameter\tmean\t2.5%\t97.5%\n")
        for name, col in rows:
            col = np.asarray(col, float)
            lo, hi = np.percentile(col, [2.5, 97.5])
            fp.write("%s\t%.6g\t%.6g\t%.6g\n" % (name, float(col.mean()), lo, hi))


# ---------------------------------------------------------------- site models
_PAIRS = np.asarray(rate_pairs(K), np.int64).reshape(-1, 2)


def parse_site_model(name):
    """``M1a`` | ``M2a`` | ``M3:k`` (k in 2..4) -> (kind, M); ValueError otherwise."""
    if name == "M1a":
        return "M1a", 2
    if name == "M2a":
        return "M2a", 3
    if isinstance(name, str) and name.startswith("M3:") and name[3:] in ("2", "3", "4"):
        return "M3", int(name[3:])
    raise ValueError("codon_sites must be M1a, M2a or M3:k with k in 2..4, got %r" % (name,))


def class_scale(rates, pi, p):
    """``s_m / sbar [n, M]`` of the classes' rates ``[n, M, R]``, the shared ``pi [n, 61]`` and the proportions
    ``p [n, M]``: s_m = 2 sum_{i<j} rates_m,ij pi_i pi_j is what the engine divides Q_m by, sbar = sum_m p_m s_m
    what the site models divide it by, so the engine's category rates of class m carry this factor.  Any dtype."""
    rates, pi, p = np.asarray(rates), np.asarray(pi), np.asarray(p)
    w = 2.0 * pi[..., _PAIRS[:, 0]] * pi[..., _PAIRS[:, 1]]  # [n, R]
    s = (rates * w[..., None, :]).sum(axis=-1)               # [n, M]
    return s / (p * s).sum(axis=-1, keepdims=True)


def class_scale_backward(rates, pi, p, g_ratio):
    """The transpose of ``class_scale``'s Jacobian: ``g_ratio [n, M]`` -> ``(g_rates [n, M, R], g_pi [n, 61],
    g_p [n, M])``."""
    rates, pi, p, g = (np.asarray(a, float) for a in (rates, pi, p, g_ratio))
    pr, pc = pi[:, _PAIRS[:, 0]], pi[:, _PAIRS[:, 1]]
    w = 2.0 * pr * pc
    s = (rates * w[:, None, :]).sum(axis=-1)
    sbar = (p * s).sum(axis=-1, keepdims=True)
    g_sbar = -(g * s).sum(axis=-1, keepdims=True) / sbar ** 2
    g_s = g / sbar + g_sbar * p
    g_p = g_sbar * s
    g_rates = g_s[:, :, None] * w[:, None, :]
    g_w = 2.0 * (g_s[:, :, None] * rates).sum(axis=1)  # d/d(pi_i pi_j) of every pair
    g_pi = np.zeros(pi.shape)
    np.add.at(g_pi.T, _PAIRS[:, 0], (g_w * pc).T)
    np.add.at(g_pi.T, _PAIRS[:, 1], (g_w * pr).T)
    return g_rates, g_pi, g_p


class CodonSitesPosterior(CodonPosterior):
    """``CodonPosterior`` with omega varying over sites: a mixture of M classes, each with its own omega_m and a
    proportion ``pclass`` Simplex(M) ~ dirichlet(1), sharing kappa or rates and pi.  As in PAML, Q_m =
    Qu(omega_m) / sbar with sbar = sum_m p_m s_m: the MEAN rate over classes is one substitution per codon.  The
    likelihood is a K-state mixture likelihood (``kseq.HostKStateMixLikelihood`` on ``kseq_mix_host``), which
    normalises each class by its own s_m, so it is handed rs[m][c] = (s_m / sbar) r_c and ps[m][c] = p_m ps_c.

    ``sites``: ``M1a`` (``omega0`` Unit ~ uniform(0, 1); omega1 = 1), ``M2a`` (M1a and ``omega2`` Lower(1) with
    omega2 - 1 ~ exponential(1)) or ``M3:k`` (``omega_first`` Lower(0) ~ lognormal(-1, 1.25) and ``omega_delta``
    Lower(0) [k - 1] ~ exponential(1): omega_m = omega_{m-1} + delta_m keeps the classes ordered)."""

    def __init__(self, spec, tree, likelihood, codon_freqs="F3x4", sites="M2a", counts=None):
        self.sites = sites
        self.kind, self.M = parse_site_model(sites)
        if self.M * spec.C > 16:
            raise ValueError("%s with %d rate categories: classes times categories must be <= 16" % (sites, spec.C))
        super().__init__(spec, tree, likelihood, codon_freqs, counts=counts)

    def _declare_subst(self, suffix=""):
        P = [p for p in CodonPosterior._declare_subst(self, suffix) if p.name != "omega"]
        head = [p for p in P if p.name in ("rates", "kappa")]
        if self.kind == "M3":
            om = [_Param("omega_first", Lower(0.0)), _Param("omega_delta", Lower(0.0, n=self.M - 1))]
        else:
            om = [_Param("omega0", Unit())] + ([_Param("omega2", Lower(1.0))] if self.kind == "M2a" else [])
        return head + om + [_Param("pclass", Simplex(self.M))] + [p for p in P if p not in head]

    def _dropped_constants(self):
        c = CodonPosterior._dropped_constants(self) + math.lgamma(float(self.M))  # pclass ~ dirichlet(1)
        if self.kind != "M3":  # no lognormal omega: uniform(0, 1) and exponential(1) have constant 0
            c += math.log(1.25) + 0.5 * math.log(2.0 * math.pi)
        return c

    # ------------------------------------------------------------ the pieces
    def omegas(self, vals):
        """omega of every class [n, M], ascending."""
        if self.kind == "M3":
            return np.cumsum(np.concatenate([vals["omega_first"][:, None], vals["omega_delta"]], axis=1), axis=1)
        cols = [vals["omega0"], np.ones_like(vals["omega0"])] + ([vals["omega2"]] if self.kind == "M2a" else [])
        return np.stack(cols, axis=1)

    def _omegas_backward(self, g_om, good, gx):
        if self.kind == "M3":
            tail = np.cumsum(g_om[:, ::-1], axis=1)[:, ::-1]  # d/d(first) and d/d(delta_m): every later class
            gx["omega_first"][good] += tail[:, 0]
            gx["omega_delta"][good] += tail[:, 1:]
            return
        gx["omega0"][good] += g_om[:, 0]
        if self.kind == "M2a":
            gx["omega2"][good] += g_om[:, 2]

    def _row_width(self):
        return 1 + self.B + 2 * self.M * self.C + self.M * (self.R + self.K)

    def _subst_forward(self, vals, n):
        M = self.M
        x6 = self._x6(vals, n)
        om = self.omegas(vals)
        rates = np.stack([codon_rates(x6, om[:, m]) for m in range(M)], axis=1)  # [n, M, R]
        pi = self.codon_frequencies(vals, n)
        r, q = self._site_rates(vals, n)
        p = vals["pclass"]
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = class_scale(rates, pi, p)
            positive = np.all(pi > 0, axis=1)
        rs = ratio[:, :, None] * r[:, None, :]
        ps = p[:, :, None] * q[:, None, :]
        comps = np.concatenate([rates, np.repeat(pi[:, None, :], M, axis=1)], axis=2).reshape(n, -1)
        return (np.concatenate([comps, rs.reshape(n, -1), ps.reshape(n, -1)], axis=1), positive,
                (r, q, x6, om, rates, pi, ratio))

    def _subst_prior(self, vals, lp, gx):
        lp = Posterior._subst_prior(self, vals, lp, gx)  # wshape, and kappa's with -m HKY
        if self.kind == "M3":
            w = vals["omega_first"]
            lw = np.log(w)
            lp = lp - lw - (lw + 1.0) ** 2 / (2.0 * 1.25 ** 2) - vals["omega_delta"].sum(axis=1)
            gx["omega_first"] += -1.0 / w - (lw + 1.0) / (1.25 ** 2 * w)
            gx["omega_delta"] -= 1.0
        elif self.kind == "M2a":
            lp = lp - (vals["omega2"] - 1.0)
            gx["omega2"] -= 1.0
        return lp

    def _subst_backward(self, vals, rows, bad, gx, sub):
        sp = self.spec
        M, C, R, B = self.M, self.C, self.R, self.B
        r, q, x6, om, rates, pi, ratio = sub
        n = rows.shape[0]
        o = 1 + B + 2 * M * C
        g_rs = rows[:, 1 + B:1 + B + M * C].reshape(n, M, C)
        g_ps = rows[:, 1 + B + M * C:o].reshape(n, M, C)
        blocks = rows[:, o:o + M * (R + self.K)].reshape(n, M, R + self.K)
        p = vals["pclass"]
        good = np.nonzero(~bad)[0]
        if len(good):
            g_ratio = (g_rs[good] * r[good][:, None, :]).sum(axis=2)
            g_rates, g_pi, g_p = class_scale_backward(rates[good], pi[good], p[good], g_ratio)
            g_rates = g_rates + blocks[good, :, :R]
            g_pi = g_pi + blocks[good, :, R:].sum(axis=1)
            gx["pclass"][good] += g_p + (g_ps[good] * q[good][:, None, :]).sum(axis=2)
            g_x6 = np.zeros((len(good), 6))
            g_om = np.zeros((len(good), M))
            for m in range(M):
                a, g_om[:, m] = codon_rates_backward(x6[good], om[good, m], g_rates[:, m])
                g_x6 += a
            self._omegas_backward(g_om, good, gx)
            if sp.model == "GTR":
                gx["rates"][good] += g_x6
            elif sp.model == "HKY":
                gx["kappa"][good] += g_x6[:, 1] + g_x6[:, 4]
            if self.codon_freqs != "F61":
                f = [v[good] for v in self._position_freqs(vals)]
                g1, g2, g3 = position_frequencies_backward(f[0], f[1], f[2], g_pi)
                if self.codon_freqs == "F3x4":
                    gx["freqs_pos1"][good] += g1
                    gx["freqs_pos2"][good] += g2
                    gx["freqs_pos3"][good] += g3
                else:
                    gx["freqs"][good] += g1 + g2 + g3
        # the site-rate model sees the classes summed out: rs[m][c] = ratio_m r_c, ps[m][c] = p_m q_c
        self._site_rates_backward(vals, (g_rs * ratio[:, :, None]).sum(axis=1), (g_ps * p[:, :, None]).sum(axis=1),
                                  gx, r, q)

    # ------------------------------------------------------------------ output
    def transformed(self, U):
        """``CodonPosterior``'s columns with the classes' free omegas as ``omega.m`` (m from 1; a fixed omega has no
        column) in place of their raw parameters, and ``pclass.1..M``."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        vals, _, _ = self.constrain(U)
        om = self.omegas(vals)
        free = [m for m in range(self.M) if not (self.kind != "M3" and m == 1)]
        out, done = [], False
        for name, arr in Posterior.transformed(self, U):
            if name in ("omega0", "omega2", "omega_first", "omega_delta"):
                if not done:
                    out += [("omega.%d" % (m + 1), om[:, m]) for m in free]
                    done = True
                continue
            out.append((name, arr))
        return out

    def codon_summary(self, U):
        """{"omegas": [n, M], "pclass": [n, M], "kappa" or "rates", "pi": [n, 61]} of draws U."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        vals, _, _ = self.constrain(U)
        out = {"omegas": self.omegas(vals), "pclass": vals["pclass"], "pi": self.codon_frequencies(vals, U.shape[0])}
        for name in ("kappa", "rates"):
            if name in vals:
                out[name] = vals[name]
        return out

    def class_posteriors(self, U):
        """The posterior probability of every class at every pattern ``[n, M, P]`` of draws U (zeros for a draw
        without a likelihood): one more evaluation of the likelihood with ``class_post``."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        _, post = self.lik.evaluate_rows(self.blens(U), self.model_vectors(U), class_post=True)
        return post


def site_summary(omegas, post, codon_pattern):
    """Per codon of the alignment, in alignment order: the posterior mean over the draws of each class's
    probability ``[codons, M]``, the posterior mean omega of the site and P(omega > 1).  ``omegas [n, M]``,
    ``post [n, M, P]``; draws without a likelihood (all-zero posteriors) are left out."""
    omegas, post = np.asarray(omegas, float), np.asarray(post, float)
    keep = post.sum(axis=(1, 2)) > 0
    if not keep.any():
        raise ValueError("no draw has a finite likelihood")
    omegas, post = omegas[keep], post[keep]
    cls = post.mean(axis=0).T                                      # [P, M]
    mean_om = (post * omegas[:, :, None]).sum(axis=1).mean(axis=0)  # [P]
    p_pos = (post * (omegas > 1.0)[:, :, None]).sum(axis=1).mean(axis=0)
    at = np.asarray(codon_pattern, np.int64)
    return cls[at], mean_om[at], p_pos[at]


def write_codon_sites_tsv(path, cls, mean_omega, p_positive):
    """OUT.codon_sites.tsv: one line per codon of the alignment."""
    M = cls.shape[1]
    with open(path, "w") as fp:
        fp.write("codon\t" + "\t".join("p.%d" % (m + 1) for m in range(M)) + "\tmean_omega\tP(omega>1)\n")
        for k in range(cls.shape[0]):
            fp.write("%d\t%s\t%.6g\t%.6g\n" % (k + 1, "\t".join("%.6g" % v for v in cls[k]), mean_omega[k],
                                                p_positive[k]))
