"""Phylogeography: the K-state discrete-trait model of the reference's
``--geo`` (``phylostan/generate_script.py:1058-1165``) around the device
engine of ``csrc/geo_engine.inc``.

* ``GeoLikelihood``        ctypes wrapper of ``phy_geo_*`` (``include/phylo_hip_geo.h``);
* ``read_metadata``        the metadata table -> tip partials (``phylostan.py:206-237``);
* ``geo_gradients_host``   the host restatement of the device's derivation
  (eigenbasis pruning, rank-one reverse pass, ``W`` with ``models.phi_rule``,
  the chain rule to ``rates_geo`` / ``freqs_geo``), for tests and as the
  yardstick of ``tools/geo_latency.py``;
* ``geo_summaries_host``   the same for ``phy_geo_eval_summaries``: node
  marginals, expected transitions and dwell times, transitions per branch;
* ``GeoSummary``           their posterior means over draws (``run --geo --ancestral``);
* ``jacobi_round_robin``   the device eigensolver's rotation order on the host;
* ``GeoPosterior``         the log density ADVI and NUTS consume:
  ``vector<lower=0.1>[R] rates_geo`` (no prior, as emitted, ``:1131``),
  ``simplex[K] freqs_geo ~ dirichlet(1)`` (``:1132-1134``);
* ``tree_sample``, ``GeoTreesLikelihood``, ``geo_trees_host``,
  ``geo_trees_summaries_host``, ``GeoTreesPosterior``: the same model
  integrated over a sample of trees (``phy_geo_trees_*``, ``csrc/geo_trees.inc``;
  ``run --geo --trees``), which the reference does not have;
* a trait clock rate mu (``clock=``, ``evaluate_rows_clock``, ``run --geo_clock
  / --geo_rate``): ``P_b = exp(Q mu t_b)`` for trees whose branch lengths are
  times, with d/dmu and a Gamma prior.

What the reference ships cannot run (``phylostan.py:253`` stores the tip data
under the key ``'geodata]'``, ``:246`` adds the second root child's length to
the slot after the intended one, and ``convert_samples_to_nexus`` finds no
``heights.1`` / ``blens.1`` column in a geo sample file); this module builds
what those lines evidently mean ("Phylogeography").
"""
import ctypes
import math
import types

import numpy as np

from . import _lib
from .models import phi_rule
from .transforms import Lower, Simplex

K_MAX = 64
RATE_LOWER = 0.1  # generate_script.py:1131


def rate_count(K):
    return K * (K - 1) // 2


def rate_pairs(K):
    """(row, col) of each ``rates_geo`` entry: the strict lower triangle column
    by column (generate_script.py:913-920)."""
    return [(row, col) for col in range(K - 1) for row in range(col + 1, K)]


def rate_matrix(freqs, rates):
    """(normalised Q, symmetric R, unnormalised Q, s) of generate_script.py:911-928."""
    f = np.asarray(freqs)
    r = np.asarray(rates)
    K = f.shape[0]
    R = np.zeros((K, K), dtype=np.result_type(f, r))
    for k, (row, col) in enumerate(rate_pairs(K)):
        R[row, col] = R[col, row] = r[k]
    Qu = R * f[None, :]
    idx = np.arange(K)
    Qu[idx, idx] = 0.0
    Qu[idx, idx] = -Qu.sum(1)
    s = -np.dot(np.diag(Qu), f)
    return Qu / s, R, Qu, s


def jacobi_round_robin(A, tol=1e-32, sweep_cap=60):
    """Cyclic Jacobi of a symmetric matrix in the device's ordering
    (csrc/geo_engine.inc): n - 1 rounds of n / 2 disjoint pairs per sweep (n =
    K, or K + 1 with a bye), until off(A)^2 <= tol |A|^2.  Returns (lam, V,
    sweeps); sweeps is -1 past the cap."""
    A = np.array(A, np.float64)
    K = A.shape[0]
    V = np.eye(K)
    n = K + (K & 1)
    nr = n - 1
    for sweep in range(sweep_cap + 1):
        tot = float((A * A).sum())
        off = float((A * A)[~np.eye(K, dtype=bool)].sum())
        if off <= tol * tot or off == 0.0:
            return np.diag(A).copy(), V, sweep
        if sweep == sweep_cap:
            break
        for r in range(nr):
            pairs = []
            for i in range(n // 2):
                x, y = (r, n - 1) if i == 0 else ((r + i) % nr, (r - i + nr) % nr)
                p, q = min(x, y), max(x, y)
                if q < K:
                    pairs.append((p, q))
            J = np.eye(K)
            for p, q in pairs:
                apq = A[p, q]
                if apq == 0.0:
                    continue
                d, e = A[q, q] - A[p, p], 2.0 * apq
                den = abs(d) + math.sqrt(d * d + e * e)
                inv = 1.0 / math.sqrt(den * den + e * e)
                c = den * inv
                s = (abs(e) if (d == 0.0 or (d > 0.0) == (e > 0.0)) else -abs(e)) * inv
                J[p, p] = c
                J[q, q] = c
                J[q, p] = -s
                J[p, q] = s
            A = J.T @ A @ J
            for p, q in pairs:
                A[p, q] = A[q, p] = 0.0
            V = V @ J
    return np.diag(A).copy(), V, -1


SCALE_BELOW = 2.0 ** -64  # the device's rescaling threshold (GEO_SCALE_BELOW)


def clock_ok(mu):
    """A usable trait clock rate: finite and > 0."""
    with np.errstate(invalid="ignore"):
        return bool(np.isfinite(mu) and mu > 0.0)


EXPM2_TERMS = 16  # the series of expm1(x) - x runs to x^16 / 16!: below 2e-17 of x^2 / 2 at |x| = 1/2


def expm1_less_x(x):
    """``expm1(x) - x = x^2/2 + x^3/6 + ...``: the series where |x| < 1/2 (the
    difference keeps 1e-16 / |x| of it), the difference beyond (the device's
    ``geo_expm1_less_x``)."""
    x = np.asarray(x, np.float64)
    h = np.zeros_like(x)
    for n in range(EXPM2_TERMS, 2, -1):
        h = (x / n) * (1.0 + h)
    return np.where(np.abs(x) < 0.5, 0.5 * x * x * (1.0 + h), np.expm1(x) - x)


def psi_rule(emk, eml, fk, fl, d, lk, t):
    """``Psi_kl = Phi_kl - t`` by ``models.phi_rule``'s three arms, each less t
    in closed form: ``t expm1(lam_k t)`` at a tie; ``t (expm1(lam_l t) p + (p -
    1))``, p the series' polynomial, in the near window; else the quotient of
    ``f = expm1(lam t) - lam t``.  Phi is t to first order, and the dwell times
    are what is left of ``diag(V W V^T)`` when that order is taken exactly."""
    from .models import NEAR_WINDOW, SERIES_WINDOW, TIE_WINDOW
    scale = np.maximum(1.0, np.abs(lk))
    tie = np.abs(d) < TIE_WINDOW * scale
    x = d * t
    series = ~tie & (np.abs(d) < NEAR_WINDOW * scale) & (np.abs(x) < SERIES_WINDOW)
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (fk - fl) / np.where(tie, 1.0, d)
    pm1 = x * (0.5 + x * (1.0 / 6.0 + x * (1.0 / 24.0 + x * (1.0 / 120.0))))
    return np.where(tie, t * emk, np.where(series, t * (eml * (1.0 + pm1) + pm1), quot))


def _geo_passes(tips, peel, blens, rates, freqs, eigensolver, bjumps=False):
    """The forward (pruning) and reverse pass of one draw, which ``geo_gradients_host``
    and ``geo_summaries_host`` share: the eigensystem of ``A = D^1/2 Q D^-1/2``,
    the rescaled lower partials, and per branch, in the device's accumulation
    order, ``dlogL/dt_b``, ``W_b = (a_b c_b^T) o Phi``, the downward messages and
    the direct ``D^{+-1/2}`` terms.  With ``bjumps``, ``bj[b] = sum(W_b o M)`` is
    formed from each ``W_b`` before it is added to ``W``.  It validates nothing:
    what a caller refuses it refuses itself.  Returns ``None`` when the root sum
    is not > 0.

    A message is ``P(t) x = x + (P(t) - I) x``, the second term through ``em =
    expm1(lam t)``, and so is the way down, ``P^T u = u + (P^T - I) u``: ``V V^T``
    is the identity to 1e-16 only, which on a short branch is 1e-16 / (q t) of a
    transition probability q t, and at t = 0 lets a parent take a state its tip
    forbids.  Phi's quotient is taken of ``em`` and the direct term ``colt -
    rowt`` from the two differences, for the same reason ("Short
    branches" of the geo engines).  A zero-length branch passes its operand
    through exactly."""
    tips = np.asarray(tips, np.float64)
    S, K = tips.shape
    peel = np.asarray(peel, np.int64)
    blens = np.asarray(blens, np.float64)
    freqs = np.asarray(freqs, np.float64)
    rates = np.asarray(rates, np.float64)
    N, B = 2 * S - 1, 2 * S - 3
    _, Rm, Qu, s = rate_matrix(freqs, rates)
    sq = np.sqrt(freqs)
    A = (sq[:, None] * sq[None, :]) * Rm / s
    A[np.arange(K), np.arange(K)] = np.diag(Qu) / s
    lam, V = np.linalg.eigh(A) if eigensolver is None else eigensolver(A)
    m1 = V / sq[:, None]
    m2 = V.T * sq[None, :]
    low = np.zeros((N, K))
    c = np.zeros((N, K))
    msg = np.zeros((N, K))
    E = np.zeros((N, K))
    EM = np.zeros((N, K))
    fac = np.ones(N)
    shift = 0
    low[:S] = tips
    nrow = len(peel)
    for r, (a, b, p) in enumerate(peel):
        last = r == nrow - 1
        for ch in ((a,) if last else (a, b)):
            c[ch] = m2 @ low[ch]
            E[ch] = np.exp(lam * blens[ch])
            EM[ch] = np.expm1(lam * blens[ch])
            msg[ch] = low[ch] + m1 @ (EM[ch] * c[ch])  # x + (P - I) x
        x = msg[a] * (low[b] if last else msg[b])
        mx = x.max()
        if 0.0 < mx < SCALE_BELOW:
            sh = min(-(math.frexp(mx)[1] - 1), 1000)
            fac[p] = math.ldexp(1.0, sh)
            shift += sh
        low[p] = x * fac[p]
    root = peel[-1][2]
    Ls = low[root].sum()
    if not Ls > 0.0:
        return None
    up = np.zeros((N, K))
    up[root] = 1.0 / Ls
    # M = V^T A_off V = diag(lam) - V^T diag(A) V: one product, since V^T A V = diag(lam)
    M = np.diag(lam) - (V.T * np.diag(A)[None, :]) @ V if bjumps else None
    gb = np.zeros(B)
    bj = np.zeros(B)
    W = np.zeros((K, K))
    dvec = np.zeros(K)  # colt - rowt: sum_b (P^T u~) o v - u~ o (P v)
    dwell0 = np.zeros(K)
    W2 = np.zeros((K, K))
    lk = lam[:, None]
    d = lk - lam[None, :]
    for r in range(nrow - 1, -1, -1):
        a, b, p = peel[r]
        last = r == nrow - 1
        upv = up[p] * fac[p]
        if last:
            ut = {a: upv * low[b]}
            up[b] = upv * msg[a]
        else:
            ut = {a: upv * msg[b], b: upv * msg[a]}
        for ch, u in ut.items():  # u = dlogL / dmessage[ch], message = P low
            aa = m1.T @ u
            e, em = E[ch], EM[ch]
            gb[ch] = (aa * lam * e * c[ch]).sum()
            Wb = np.outer(aa, c[ch]) * phi_rule(e[:, None], e[None, :], d, lk, blens[ch], em=(em[:, None], em[None, :]))
            if bjumps:
                bj[ch] = (Wb * M).sum()
                # the dwell times, diag(V W V^T), with Phi = t + Psi: the t part is t u~ o v exactly (V a = u~ /
                # sqrt(pi), V c = sqrt(pi) v), the rest is of second order in t
                dwell0 += blens[ch] * u * low[ch]
                f = expm1_less_x(lam * blens[ch])
                W2 += np.outer(aa, c[ch]) * psi_rule(em[:, None], em[None, :], f[:, None], f[None, :], d, lk, blens[ch])
            W += Wb
            du = m2.T @ (em * aa)  # (P^T - I) u
            up[ch] = u + du
            dvec += du * low[ch] - u * (msg[ch] - low[ch])
    dwell = dwell0 + np.einsum("ik,kl,il->i", V, W2, V) if bjumps else None
    return types.SimpleNamespace(Ls=Ls, logL=math.log(Ls) - shift * math.log(2.0), gb=gb, bj=bj, W=W, dvec=dvec,
                                 dwell=dwell, low=low, up=up, root=root, V=V, A=A, Rm=Rm, Qu=Qu, s=s, sq=sq)


def geo_gradients_host(tips, peel, blens, rates, freqs, eigensolver=None, clock=None):
    """log L and its gradient as the device computes them: returns ``(logL,
    grad_blens[B], grad_rates[R], grad_freqs[K])``, the ``freqs`` entries taken
    as independent.  ``eigensolver(A) -> (lam, V)`` defaults to
    ``numpy.linalg.eigh``.

    With a trait clock rate ``clock`` (mu) the likelihood is taken at the
    effective lengths ``mu * blens`` and a fifth value follows, ``dlogL/dmu =
    sum_b t_b dlogL/dt_eff,b``; ``grad_blens`` is then with respect to the
    tree's own lengths (``mu dlogL/dt_eff``).  A mu that is not finite or not
    > 0 gives -inf and zeros."""
    if clock is not None:
        t = np.asarray(blens, np.float64)
        mu = float(clock)
        if not clock_ok(mu):
            return -np.inf, np.zeros(t.size), np.zeros(np.size(rates)), np.zeros(np.size(freqs)), 0.0
        ll, gb, gr, gf = geo_gradients_host(tips, peel, mu * t, rates, freqs, eigensolver)
        return ll, mu * gb, gr, gf, float(np.dot(t, gb))
    freqs = np.asarray(freqs, np.float64)
    K = freqs.size
    st = _geo_passes(tips, peel, blens, rates, freqs, eigensolver)
    if st is None:
        return -np.inf, np.zeros(2 * len(peel) - 1), np.zeros(len(rates)), np.zeros(K)
    V, Rm, Qu, s, sq = st.V, st.Rm, st.Qu, st.s, st.sq
    dA = V @ st.W @ V.T
    dA = 0.5 * (dA + dA.T)
    # P = D^-1/2 exp(A t) D^1/2: the direct pi dependence
    g_direct = 0.5 * st.dvec / freqs
    dQ = dA * sq[:, None] / sq[None, :]
    ds = -(dQ * (Qu / s)).sum() / s  # not / s^2: rates near 1e160 would square past the fp64 range
    dd = np.diag(dQ) / s - ds * freqs  # dlogL / dQu_ii, the path through s included
    off = dQ / s - dd[:, None]          # Qu_ii = -sum_{j != i} Qu_ij
    np.fill_diagonal(off, 0.0)
    gR = off * freqs[None, :]
    g_rates = np.array([gR[row, col] + gR[col, row] for row, col in rate_pairs(K)])
    g_freqs = g_direct - ds * np.diag(Qu) + (off * Rm).sum(0)
    return st.logL, st.gb, g_rates, g_freqs


def summary_len(S, K):
    """Doubles of one summary row: marg [2S-1, K], jumps [K, K], bjumps [2S-3]."""
    return (2 * S - 1) * K + K * K + (2 * S - 3)


def split_summaries(flat, S, K):
    """Summary rows ``[n, summary_len]`` -> ``(marg [n, N, K], jumps [n, K, K],
    bjumps [n, B])``."""
    flat = np.asarray(flat, np.float64)
    n = flat.shape[0]
    N, B = 2 * S - 1, 2 * S - 3
    return (flat[:, :N * K].reshape(n, N, K), flat[:, N * K:N * K + K * K].reshape(n, K, K),
            flat[:, N * K + K * K:].reshape(n, B))


def geo_summaries_host(tips, peel, blens, rates, freqs, eigensolver=None, clock=None):
    """The posterior summaries of one draw as the device computes them
    (``phy_geo_eval_summaries``): returns ``(marg [2S-1, K], jumps [K, K],
    bjumps [2S-3])``.

    * ``marg[n] = low(n) o up[n]``: the posterior state distribution of node n,
      ``up`` the derivative of log L with respect to the (scaled) lower partial;
      row 2S-3, the merged root child, repeats the root's row 2S-2;
    * ``jumps[i, j] = A_ij G_ij`` (i != j), the expected number of i -> j
      transitions over the tree, and ``jumps[i, i] = G_ii``, the expected time
      in i, with ``G = V W V^T`` before it is symmetrised (Minin & Suchard 2008);
      the diagonal is formed as ``sum_b t_b u~_b o v_b + diag(V W2 V^T)``, ``W2``
      being W with ``Psi = Phi - t`` (``psi_rule``) in Phi's place: the product
      keeps on its diagonal 1e-16 of G's largest entry, which on a tree of
      total length 1e-7 is 1e-7 of the dwell times ("Short branches
      of the geo engines");
    * ``bjumps[b] = sum_kl a_bk c_bl Phi_kl(t_b) M_kl``, ``M = V^T A_off V``: the
      expected number of transitions of any kind on branch b.
    A draw without a finite likelihood gives zeros.  With a trait clock rate
    ``clock`` (mu) the summaries are those at ``mu * blens``, the dwell times
    ``jumps[i, i]`` divided by mu: in the tree's own unit."""
    if clock is not None:
        mu = float(clock)
        if not clock_ok(mu):
            mu = np.nan
        marg, jumps, bj = geo_summaries_host(tips, peel, mu * np.asarray(blens, np.float64), rates, freqs, eigensolver)
        if clock_ok(mu):
            idx = np.arange(jumps.shape[0])
            jumps[idx, idx] = jumps[idx, idx] / mu
        return marg, jumps, bj
    S, K = np.shape(tips)
    zero = (np.zeros((2 * S - 1, K)), np.zeros((K, K)), np.zeros(2 * S - 3))
    freqs = np.asarray(freqs, np.float64)
    rates = np.asarray(rates, np.float64)
    with np.errstate(all="ignore"):
        bad = not (np.all(freqs > 0.0) and np.all(np.isfinite(freqs)) and np.all(rates >= 0.0)
                   and np.all(np.isfinite(rates)) and np.all(np.isfinite(blens)))
    if bad:
        return zero
    s = rate_matrix(freqs, rates)[3]
    if not (s > 0.0 and np.isfinite(s)):
        return zero
    st = _geo_passes(tips, peel, blens, rates, freqs, eigensolver, bjumps=True)
    if st is None or not np.isfinite(st.Ls):
        return zero
    marg = st.low * st.up
    marg[peel[-1][1]] = marg[st.root]  # the merged root child carries the root's distribution
    G = st.V @ st.W @ st.V.T
    jumps = st.A * G
    # G's diagonal is of order t beside off-diagonal entries of order 1 / q on a short tree: taken directly it keeps
    # 1e-16 of those
    jumps[np.arange(K), np.arange(K)] = st.dwell
    return marg, jumps, st.bj


class GeoSummary:
    """Posterior means of the three summary arrays, accumulated chunk by chunk
    over the draws of ``evaluate_summaries``.  Draws without a finite
    likelihood (``rows[:, 0]`` not finite: their summary is a zero row) are
    counted in ``skipped`` and left out of the means."""

    def __init__(self, S, K):
        self.S, self.K = int(S), int(K)
        self.count = 0
        self.skipped = 0
        self._marg = np.zeros((2 * self.S - 1, self.K))
        self._jumps = np.zeros((self.K, self.K))
        self._bjumps = np.zeros(2 * self.S - 3)

    def add(self, rows, marg, jumps, bjumps):
        ok = np.isfinite(np.asarray(rows)[:, 0])
        self.count += int(ok.sum())
        self.skipped += int((~ok).sum())
        self._marg += np.asarray(marg)[ok].sum(0)
        self._jumps += np.asarray(jumps)[ok].sum(0)
        self._bjumps += np.asarray(bjumps)[ok].sum(0)

    def _mean(self, x):
        if self.count == 0:
            raise ValueError("no draw with a finite likelihood to average")
        return x / self.count

    @property
    def marg(self):
        """[2S-1, K] posterior-mean state probabilities of every node, each row
        divided by its sum (1 to rounding: a known tip's 1 + 2^-52 becomes 1)."""
        m = self._mean(self._marg)
        return m / m.sum(1, keepdims=True)

    @property
    def jumps(self):
        """[K, K] off-diagonal: expected i -> j transitions; diagonal: expected time in i."""
        return self._mean(self._jumps)

    @property
    def bjumps(self):
        """[2S-3] expected transitions on each branch."""
        return self._mean(self._bjumps)

    @property
    def migrations(self):
        """K x K expected transitions, the diagonal zero."""
        m = self.jumps.copy()
        np.fill_diagonal(m, 0.0)
        return m

    @property
    def times(self):
        return np.diag(self.jumps).copy()


class GeoLikelihood:
    """One device context of the discrete-trait engine.  ``tips [S, K]`` tip
    partials, ``peel0 [S-1, 3]`` 0-based in the unrooted convention."""

    def __init__(self, tips, peel0, max_draws=128, device=0):
        self.lib = _lib.load()
        tips = np.ascontiguousarray(tips, np.float64)
        if tips.ndim != 2:
            raise ValueError("tips must be [S, K]")
        self.S, self.K = (int(v) for v in tips.shape)
        self.R = rate_count(self.K)
        peel0 = np.ascontiguousarray(peel0, np.int32)
        if peel0.shape != (self.S - 1, 3):
            raise ValueError("peel must be [S-1, 3]")
        self.max_draws = int(max_draws)
        ctx = ctypes.c_void_p()
        self.ctx = None
        _lib.check(self.lib.phy_geo_create(self.S, self.K, tips.ctypes.data, peel0.ctypes.data, self.max_draws,
                                           int(device), ctypes.byref(ctx)), "phy_geo_create")
        self.ctx = ctx
        self.B = self.lib.phy_geo_num_branches(self.ctx)
        self.outlen = self.lib.phy_geo_output_len(self.ctx)
        self.param_len = self.R + self.K

    def evaluate_rows(self, blens, params):
        """n draws -> rows [n, 1 + B + R + K]: log L, d/dblens, d/drates, d/dfreqs."""
        blens = np.ascontiguousarray(np.atleast_2d(np.asarray(blens, np.float64)))
        params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, np.float64)))
        n = blens.shape[0]
        if blens.shape != (n, self.B) or params.shape != (n, self.param_len):
            raise ValueError("bad shapes: blens %s params %s" % (blens.shape, params.shape))
        out = np.empty((n, self.outlen))
        _lib.check(self.lib.phy_geo_eval(self.ctx, n, blens.ctypes.data, params.ctypes.data, out.ctypes.data),
                   "phy_geo_eval")
        return out

    def evaluate_summaries(self, blens, params):
        """n draws -> ``(rows [n, 1 + B + R + K], marg [n, 2S-1, K], jumps [n, K,
        K], bjumps [n, B])``: the rows of ``evaluate_rows`` (bitwise) and each
        draw's posterior summaries (``geo_summaries_host`` states them; a draw
        whose row is -inf has a zero summary)."""
        blens = np.ascontiguousarray(np.atleast_2d(np.asarray(blens, np.float64)))
        params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, np.float64)))
        n = blens.shape[0]
        if blens.shape != (n, self.B) or params.shape != (n, self.param_len):
            raise ValueError("bad shapes: blens %s params %s" % (blens.shape, params.shape))
        slen = self.lib.phy_geo_summary_len(self.ctx)
        out = np.empty((n, self.outlen))
        flat = np.empty((n, slen))
        _lib.check(self.lib.phy_geo_eval_summaries(self.ctx, n, blens.ctypes.data, params.ctypes.data,
                                                   out.ctypes.data, flat.ctypes.data), "phy_geo_eval_summaries")
        return (out,) + split_summaries(flat, self.S, self.K)

    def evaluate_rows_clock(self, blens, params, clock):
        """n draws with a trait clock rate ``clock [n]`` (mu) -> rows [n, 2 + B +
        R + K]: log L at ``mu * blens``, d/dblens with respect to the tree's own
        lengths, d/drates, d/dfreqs, d/dmu.  ``phy_geo_eval`` takes the products;
        a draw whose mu is not finite or not > 0 is -inf and zeros."""
        return _single_tree_clock_rows(self.evaluate_rows, blens, params, clock, self.B)

    def evaluate_summaries_clock(self, blens, params, clock):
        """``evaluate_summaries`` with a trait clock rate: ``(rows [n, 2 + B + R +
        K] of evaluate_rows_clock, marg, jumps, bjumps)``, the dwell times
        ``jumps[n, i, i]`` in the tree's unit."""
        blens, mu, ok = _clock_products(blens, clock)
        out, marg, jumps, bjumps = self.evaluate_summaries(np.where(ok[:, None], mu[:, None] * blens, 0.0), params)
        rows = _clock_rows_from(out, blens, mu, ok, self.B)
        marg, jumps, bjumps = marg.copy(), jumps.copy(), bjumps.copy()
        idx = np.arange(self.K)
        jumps[:, idx, idx] /= np.where(ok, mu, 1.0)[:, None]
        marg[~ok], jumps[~ok], bjumps[~ok] = 0.0, 0.0, 0.0
        return rows, marg, jumps, bjumps

    def info(self):
        v = [ctypes.c_int() for _ in range(5)]
        _lib.check(self.lib.phy_geo_info(self.ctx, *[ctypes.byref(x) for x in v]), "phy_geo_info")
        return dict(zip(("levels", "widest_level", "lds_bytes", "threads", "workgroups"), (x.value for x in v)))

    def sweeps(self, n):
        """Jacobi sweeps of the first n draws of the last call."""
        out = np.empty(n, np.int32)
        _lib.check(self.lib.phy_geo_sweeps(self.ctx, n, out.ctypes.data), "phy_geo_sweeps")
        return out

    def close(self):
        if self.ctx is not None:
            self.lib.phy_geo_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _clock_products(blens, clock):
    blens = np.atleast_2d(np.asarray(blens, np.float64))
    mu = np.asarray(clock, np.float64).reshape(-1)
    if mu.size == 1 and blens.shape[0] != 1:
        mu = np.full(blens.shape[0], mu[0])
    if mu.shape != (blens.shape[0],):
        raise ValueError("bad shapes: blens %s clock %s" % (blens.shape, mu.shape))
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(mu) & (mu > 0.0)
    return blens, mu, ok


def _clock_rows_from(out, blens, mu, ok, B):
    """The rows of a single-tree call at ``mu * blens`` -> the clock rows: the
    d/dblens block times mu, d/dmu = sum_b t_b d/dt_eff,b appended."""
    rows = np.empty((out.shape[0], out.shape[1] + 1))
    rows[:, :-1] = out
    rows[:, -1] = (blens * out[:, 1:1 + B]).sum(1)
    rows[:, 1:1 + B] *= mu[:, None]
    rows[~ok, 0] = -np.inf
    rows[~ok, 1:] = 0.0
    return rows


def _single_tree_clock_rows(evaluate_rows, blens, params, clock, B):
    blens, mu, ok = _clock_products(blens, clock)
    out = evaluate_rows(np.where(ok[:, None], mu[:, None] * blens, 0.0), params)
    return _clock_rows_from(out, blens, mu, ok, B)


def mean_tree_length(blens, log_weights=None):
    """The default rate ``b`` of the clock's Gamma prior: the tree's length
    ``sum_b t_b`` for one tree, the ``w_t``-weighted mean total length for a
    sample ``blens [T, B]`` (``w_t = exp(log_weights[t])``, default equal)."""
    blens = np.asarray(blens, np.float64)
    if blens.ndim == 1:
        return float(blens.sum())
    lengths = blens.sum(1)
    if log_weights is None:
        return float(lengths.mean())
    lw = np.asarray(log_weights, np.float64)
    w = np.exp(lw - lw.max())
    return float(np.dot(w, lengths) / w.sum())


def read_metadata(path, key="Country", taxa=None):
    """The metadata table of ``run --geo -M`` (phylostan.py:206-237):
    tab-separated with a header, the first column the taxon, column ``key``
    its location.  States are numbered in the order the taxa of ``taxa`` (the
    tree's namespace order; default: the file's row order) first show them; a
    taxon without a row is an error.  Returns ``(tips [S, K] one-hot,
    states)``."""
    with open(path) as fp:
        header = next(fp).rstrip("\r\n").split("\t")
        if key not in header:
            raise ValueError("metadata file %s has no column %r (columns: %s)" % (path, key, ", ".join(header)))
        col = header.index(key)
        where = {}
        order = []
        for line in fp:
            row = line.rstrip("\r\n").split("\t")
            if len(row) <= col or not row[0]:
                continue
            if row[0] not in where:
                order.append(row[0])
            where[row[0]] = row[col]
    taxa = order if taxa is None else list(taxa)
    missing = [t for t in taxa if t not in where]
    if missing:
        raise ValueError("taxa without a row in the metadata file %s: %s" % (path, ", ".join(missing[:5])))
    states = []
    index = {}
    for t in taxa:
        if where[t] not in index:
            index[where[t]] = len(states)
            states.append(where[t])
    tips = np.zeros((len(taxa), len(states)))
    for i, t in enumerate(taxa):
        tips[i, index[where[t]]] = 1.0
    return tips, states


def tree_branch_lengths(tree, peel0):
    """The fixed ``blens[2S-3]`` of the geo model from the tree's edge lengths
    (phylostan.py:239-247): branch b is the edge above node b, the two root
    edges merged into the first root child's.  A negative or missing length
    raises ``ValueError``."""
    S = len(tree.taxon_namespace)
    bl = np.zeros(2 * S - 1)
    for node in tree.postorder_node_iter():
        if node.parent_node is None:
            continue
        if node.edge_length is None or node.edge_length < 0:
            raise ValueError("negative or missing branch length above node %d" % node.index)
        bl[node.index - 1] = node.edge_length
    a, b, _ = (int(v) for v in peel0[-1])
    bl[a] += bl[b]
    return bl[:2 * S - 3].copy()


def tree_sample(trees, taxa):
    """A tree sample (``treeio.read_trees``) in the engine's terms: returns
    ``(peels [T, S-1, 3], blens [T, 2S-3])``, every peel 0-based in the
    unrooted convention, tips numbered by their position in ``taxa`` whatever
    each tree's own leaf order is, branch lengths by ``tree_branch_lengths``
    (the merged root branch is the sum of the two root-child edges).  A tree
    whose labels are not exactly ``taxa``, or with a missing or negative
    length, raises ``ValueError`` naming the tree."""
    from . import data as dataio
    from .treeio import Taxon, Tree
    taxa = [str(t) for t in taxa]
    S = len(taxa)
    want = set(taxa)
    if len(want) != S:
        raise ValueError("taxa holds a label twice")
    peels = np.zeros((len(trees), S - 1, 3), np.int32)
    blens = np.zeros((len(trees), 2 * S - 3))
    for t, src in enumerate(trees):
        labels = [leaf.taxon.label for leaf in src.leaf_node_iter()]
        if len(labels) != S or set(labels) != want:
            odd = sorted(set(labels) ^ want)
            raise ValueError("tree %d: its %d leaves are not the %d taxa of the model%s"
                             % (t, len(labels), S, " (e.g. %s)" % ", ".join(odd[:3]) if odd else ""))
        tree = Tree(src.seed_node, [Taxon(lab) for lab in taxa])
        tree.resolve_polytomies(update_bipartitions=True)
        dataio.setup_indexes(tree)
        peel0 = np.asarray(dataio.unrooted_peel(dataio.get_peeling_order(tree)), dtype=np.int32) - 1
        try:
            blens[t] = tree_branch_lengths(tree, peel0)
        except ValueError as e:
            raise ValueError("tree %d: %s" % (t, e))
        peels[t] = peel0
    return peels, blens


def select_trees(n, burnin=0.0, max_trees=0):
    """The trees ``run --geo --trees`` keeps of a file of n: the leading
    ``floor(burnin n)`` are dropped, and of the m left, when ``0 < max_trees <
    m``, the ``max_trees`` at ``floor(i m / max_trees)``, i = 0 .. max_trees - 1
    (evenly spaced, the first kept tree always in).  Returns their indices."""
    if not 0.0 <= burnin < 1.0:
        raise ValueError("the burn-in fraction must lie in [0, 1)")
    idx = np.arange(int(math.floor(burnin * n)), n)
    if 0 < max_trees < idx.size:
        idx = idx[(np.arange(max_trees) * idx.size) // max_trees]
    return idx


def _mixture_weights(tree_ll, log_weights):
    """(log L_mix, p [T]) of per-tree log likelihoods: log-sum-exp against the
    largest term; a tree without a finite log L has weight 0."""
    with np.errstate(invalid="ignore"):
        x = np.where(np.isfinite(tree_ll), tree_ll + log_weights, -np.inf)
    mx = x.max()
    if not np.isfinite(mx):
        return -np.inf, np.zeros(x.size)
    w = np.exp(x - mx)
    return mx + math.log(w.sum()), w / w.sum()


def geo_trees_host(tips, peels, blens, rates, freqs, log_weights=None, eigensolver=None, clock=None):
    """The mixture over a tree sample as the device computes it
    (``phy_geo_trees_eval``), tree by tree on ``geo_gradients_host``: returns
    ``(log L_mix, grad_rates [R], grad_freqs [K], tree_ll [T])`` with ``L_mix
    = sum_t exp(log_weights[t]) L_t`` (default weights 1 / T) and ``grad log
    L_mix = sum_t p_t grad log L_t``, ``p_t`` the posterior tree weights.

    With a trait clock rate ``clock`` (mu) every tree is taken at ``mu *
    blens[t]`` and a fifth value follows: ``dlogL_mix/dmu = sum_t p_t sum_b
    t_tb dlogL_t/dt_eff,b``, summed branch by branch (the device forms it from
    the eigenvalues and the diagonal of W instead)."""
    peels = np.asarray(peels)
    blens = np.asarray(blens, np.float64)
    rates = np.asarray(rates, np.float64)
    freqs = np.asarray(freqs, np.float64)
    T = peels.shape[0]
    logw = np.full(T, -math.log(T)) if log_weights is None else np.asarray(log_weights, np.float64)
    tll = np.full(T, -np.inf)
    gr = np.zeros((T, rates.size))
    gf = np.zeros((T, freqs.size))
    gm = np.zeros(T)
    with np.errstate(all="ignore"):
        bad = not (np.all(freqs > 0.0) and np.all(np.isfinite(freqs)) and np.all(rates >= 0.0)
                   and np.all(np.isfinite(rates)) and (clock is None or clock_ok(float(clock))))
    if not bad:
        for t in range(T):
            res = geo_gradients_host(tips, peels[t], blens[t], rates, freqs, eigensolver, clock=clock)
            if np.isfinite(res[0]):
                tll[t], gr[t], gf[t] = res[0], res[2], res[3]
                if clock is not None:
                    gm[t] = res[4]
    lmix, p = _mixture_weights(tll, logw)
    out = (lmix, p @ gr, p @ gf, tll)
    return out if clock is None else out + (float(p @ gm),)


def geo_trees_summaries_host(tips, peels, blens, rates, freqs, log_weights=None, eigensolver=None, clock=None):
    """The summaries of ``phy_geo_trees_eval_summaries`` for one draw:
    ``(jumps [K, K], root [K])``, the posterior-tree-weighted means of
    ``geo_summaries_host``'s ``jumps`` and of its root row ``marg[2S-2]``.
    Zeros when no tree has a finite likelihood.  With a trait clock rate
    ``clock`` (mu): the summaries at ``mu * blens``, dwell times in the tree's
    unit."""
    peels = np.asarray(peels)
    blens = np.asarray(blens, np.float64)
    T = peels.shape[0]
    K = np.asarray(freqs).size
    if clock is not None:
        if not clock_ok(float(clock)):
            return np.zeros((K, K)), np.zeros(K)
        jumps, root = geo_trees_summaries_host(tips, peels, float(clock) * blens, rates, freqs, log_weights,
                                               eigensolver)
        idx = np.arange(K)
        jumps[idx, idx] = jumps[idx, idx] / float(clock)
        return jumps, root
    _, _, _, tll = geo_trees_host(tips, peels, blens, rates, freqs, log_weights, eigensolver)
    logw = np.full(T, -math.log(T)) if log_weights is None else np.asarray(log_weights, np.float64)
    _, p = _mixture_weights(tll, logw)
    jumps = np.zeros((K, K))
    root = np.zeros(K)
    for t in range(T):
        if p[t] > 0.0:
            marg, j, _ = geo_summaries_host(tips, peels[t], blens[t], rates, freqs, eigensolver)
            jumps += p[t] * j
            root += p[t] * marg[-1]
    return jumps, root


class GeoTreesLikelihood:
    """One device context of the tree-sample engine (``phy_geo_trees_*``):
    ``tips [S, K]``, ``peels [T, S-1, 3]`` 0-based in the unrooted convention,
    ``blens [T, 2S-3]``, ``log_weights [T]`` (default ``-log T`` each)."""

    def __init__(self, tips, peels, blens, log_weights=None, max_draws=128, device=0):
        self.lib = _lib.load()
        tips = np.ascontiguousarray(tips, np.float64)
        if tips.ndim != 2:
            raise ValueError("tips must be [S, K]")
        self.S, self.K = (int(v) for v in tips.shape)
        self.R = rate_count(self.K)
        self.B = 2 * self.S - 3
        peels = np.ascontiguousarray(peels, np.int32)
        blens = np.ascontiguousarray(blens, np.float64)
        if peels.ndim != 3 or peels.shape[1:] != (self.S - 1, 3):
            raise ValueError("peels must be [T, S-1, 3]")
        self.T = int(peels.shape[0])
        if blens.shape != (self.T, self.B):
            raise ValueError("blens must be [T, 2S-3]")
        if log_weights is None:
            self.log_weights = np.full(self.T, -math.log(max(self.T, 1)))
            lw = None
        else:
            self.log_weights = np.ascontiguousarray(log_weights, np.float64)
            if self.log_weights.shape != (self.T,):
                raise ValueError("log_weights must be [T]")
            lw = self.log_weights.ctypes.data
        self.max_draws = int(max_draws)
        self.param_len = self.R + self.K
        self.mean_length = mean_tree_length(blens, self.log_weights)  # the clock prior's default rate
        self.tree_loglik = None  # [n, T] log L_t of the last call's draws
        ctx = ctypes.c_void_p()
        self.ctx = None
        _lib.check(self.lib.phy_geo_trees_create(self.S, self.K, tips.ctypes.data, self.T, peels.ctypes.data,
                                                 blens.ctypes.data, lw, self.max_draws, int(device),
                                                 ctypes.byref(ctx)), "phy_geo_trees_create")
        self.ctx = ctx
        self.outlen = self.lib.phy_geo_trees_output_len(self.ctx)

    def _params(self, params):
        params = np.ascontiguousarray(np.atleast_2d(np.asarray(params, np.float64)))
        if params.ndim != 2 or params.shape[1] != self.param_len:
            raise ValueError("bad shape: params %s" % (params.shape,))
        return params

    def evaluate_rows(self, params):
        """n draws -> rows [n, 1 + R + K]: log L_mix, d/drates, d/dfreqs;
        ``tree_loglik`` [n, T] holds every tree's log L_t afterwards."""
        params = self._params(params)
        n = params.shape[0]
        out = np.empty((n, self.outlen))
        tll = np.empty((n, self.T))
        _lib.check(self.lib.phy_geo_trees_eval(self.ctx, n, params.ctypes.data, out.ctypes.data, tll.ctypes.data),
                   "phy_geo_trees_eval")
        self.tree_loglik = tll
        return out

    def evaluate_summaries(self, params):
        """n draws -> ``(rows [n, 1 + R + K], jumps [n, K, K], root [n, K])``:
        the rows of ``evaluate_rows`` (bitwise) and the posterior-tree-weighted
        summaries (``geo_trees_summaries_host`` states them)."""
        params = self._params(params)
        n = params.shape[0]
        K = self.K
        out = np.empty((n, self.outlen))
        tll = np.empty((n, self.T))
        flat = np.empty((n, self.lib.phy_geo_trees_summary_len(self.ctx)))
        _lib.check(self.lib.phy_geo_trees_eval_summaries(self.ctx, n, params.ctypes.data, out.ctypes.data,
                                                         tll.ctypes.data, flat.ctypes.data),
                   "phy_geo_trees_eval_summaries")
        self.tree_loglik = tll
        return out, flat[:, :K * K].reshape(n, K, K), flat[:, K * K:].copy()

    def _clock(self, clock, n):
        clock = np.ascontiguousarray(np.asarray(clock, np.float64).reshape(-1))
        if clock.size == 1 and n != 1:
            clock = np.full(n, clock[0])
        if clock.shape != (n,):
            raise ValueError("bad shape: clock %s for %d draws" % (clock.shape, n))
        return clock

    def evaluate_rows_clock(self, params, clock):
        """n draws with a trait clock rate ``clock [n]`` (mu; one value serves
        every draw) -> rows [n, 2 + R + K]: log L_mix at the lengths ``mu *
        blens``, d/drates, d/dfreqs, d/dmu (``phy_geo_trees_eval_clock``)."""
        params = self._params(params)
        n = params.shape[0]
        clock = self._clock(clock, n)
        out = np.empty((n, self.lib.phy_geo_trees_clock_output_len(self.ctx)))
        tll = np.empty((n, self.T))
        _lib.check(self.lib.phy_geo_trees_eval_clock(self.ctx, n, params.ctypes.data, clock.ctypes.data,
                                                     out.ctypes.data, tll.ctypes.data), "phy_geo_trees_eval_clock")
        self.tree_loglik = tll
        return out

    def evaluate_summaries_clock(self, params, clock):
        """``(rows [n, 2 + R + K], jumps [n, K, K], root [n, K])``: the rows of
        ``evaluate_rows_clock`` (bitwise) and the summaries, the dwell times
        ``jumps[n, i, i]`` in the tree's own unit."""
        params = self._params(params)
        n = params.shape[0]
        K = self.K
        clock = self._clock(clock, n)
        out = np.empty((n, self.lib.phy_geo_trees_clock_output_len(self.ctx)))
        tll = np.empty((n, self.T))
        flat = np.empty((n, self.lib.phy_geo_trees_summary_len(self.ctx)))
        _lib.check(self.lib.phy_geo_trees_eval_clock_summaries(self.ctx, n, params.ctypes.data, clock.ctypes.data,
                                                               out.ctypes.data, tll.ctypes.data, flat.ctypes.data),
                   "phy_geo_trees_eval_clock_summaries")
        self.tree_loglik = tll
        return out, flat[:, :K * K].reshape(n, K, K), flat[:, K * K:].copy()

    def tree_posterior(self, rows):
        """p_t [n, T] of the last call's draws from its rows: exp(tree_ll + log w - log L_mix); zeros where
        the mixture has no finite likelihood."""
        return tree_posterior(self.tree_loglik, self.log_weights, np.asarray(rows)[:, 0])

    def info(self):
        v = [ctypes.c_int() for _ in range(6)]
        _lib.check(self.lib.phy_geo_trees_info(self.ctx, *[ctypes.byref(x) for x in v]), "phy_geo_trees_info")
        return dict(zip(("widest_level", "max_levels", "groups", "threads", "lds_bytes", "workgroups"),
                        (x.value for x in v)))

    def close(self):
        if self.ctx is not None:
            self.lib.phy_geo_trees_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def tree_posterior(tree_ll, log_weights, log_mix):
    """p [n, T] = exp(tree_ll + log_weights - log_mix[:, None]), 0 where a term or the mixture is not finite."""
    tree_ll = np.atleast_2d(np.asarray(tree_ll, np.float64))
    log_mix = np.asarray(log_mix, np.float64).reshape(-1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        x = tree_ll + np.asarray(log_weights, np.float64)[None, :] - log_mix
        return np.where(np.isfinite(tree_ll) & np.isfinite(log_mix), np.exp(x), 0.0)


class GeoPosterior:
    """log p(rates_geo, freqs_geo | locations, tree) on Stan's unconstrained
    scale, Jacobian included: the interface ``advi.ADVI`` and
    ``nuts.run_chains`` consume.  ``likelihood`` offers ``evaluate_rows(blens
    [n, B], params [n, R + K])``; the branch lengths are data.

    ``clock``: the trait clock rate mu of ``P_b = exp(Q mu t_b)``.  ``None``:
    no clock, the class calls ``evaluate_rows`` as it always has.  A float: mu
    is fixed, no new coordinate; ``likelihood.evaluate_rows_clock(blens, params,
    clock [n])`` is called instead.  ``"estimate"``: one more coordinate, u =
    log mu, last, with ``mu ~ Gamma(a, b)``, ``clock_prior=(a, b)``; the
    default is a = 1/2 and b = the tree's length, the CTMC-rate reference prior
    of Ferreira & Suchard (2008) at a fixed tree length.  Its density on u,
    Jacobian included, is ``a u - b mu`` (+ ``a log b - lgamma(a)``)."""

    def __init__(self, K, blens, likelihood, clock=None, clock_prior=None, mean_length=None):
        self.K = int(K)
        self.R = rate_count(self.K)
        self.blens = np.asarray(blens, np.float64)
        self.B = self.blens.size
        self.lik = likelihood
        self.t_rates = Lower(RATE_LOWER, self.R)
        self.t_freqs = Simplex(self.K)
        self.dim = self.R + self.K - 1
        # freqs_geo ~ dirichlet(1): the density is its normaliser, log Gamma(K)
        self.const = math.lgamma(self.K)
        self.clock_estimated = isinstance(clock, str)
        self.clock_fixed = None
        self.clock_prior = None
        if self.clock_estimated:
            if clock != "estimate":
                raise ValueError("clock must be None, 'estimate' or a positive number")
            if clock_prior is None:
                clock_prior = (0.5, mean_tree_length(self.blens) if mean_length is None else float(mean_length))
            a, b = (float(v) for v in clock_prior)
            if not (clock_ok(a) and clock_ok(b)):
                raise ValueError("the clock prior's shape and rate must be positive and finite")
            self.clock_prior = (a, b)
            self.dim += 1
            self.const += a * math.log(b) - math.lgamma(a)
        elif clock is not None:
            if clock_prior is not None:
                raise ValueError("a clock prior needs an estimated clock")
            self.clock_fixed = float(clock)
            if not clock_ok(self.clock_fixed):
                raise ValueError("the clock rate must be positive and finite")
        elif clock_prior is not None:
            raise ValueError("a clock prior needs an estimated clock")
        self.has_clock = self.clock_estimated or self.clock_fixed is not None
        self.nfree = self.R + self.K - 1  # the coordinates of rates_geo and freqs_geo

    def constrain(self, U):
        """``(rates, freqs, log Jacobian, transform states)``; with an estimated
        clock the states carry mu = exp(u) as their third entry (its Jacobian
        is part of the prior's density on u)."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        rates, lj_r, st_r = self.t_rates.constrain(U[:, :self.R])
        freqs, lj_f, st_f = self.t_freqs.constrain(U[:, self.R:self.nfree])
        if self.clock_estimated:
            with np.errstate(over="ignore"):
                return rates, freqs, lj_r + lj_f, (st_r, st_f, np.exp(U[:, self.nfree]))
        return rates, freqs, lj_r + lj_f, (st_r, st_f)

    def clock_rates(self, U):
        """mu [n] of the points U: exp(u) when estimated, the fixed rate, or None without a clock."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        if self.clock_estimated:
            return np.exp(U[:, self.nfree])
        return None if self.clock_fixed is None else np.full(U.shape[0], self.clock_fixed)

    def log_prob_grad(self, U, propto=True, need_grad=True):
        U = np.atleast_2d(np.asarray(U, np.float64))
        n = U.shape[0]
        lp = np.full(n, -np.inf)
        G = np.zeros((n, self.dim)) if need_grad else None
        with np.errstate(all="ignore"):
            rates, freqs, logj, st = self.constrain(np.where(np.isfinite(U), U, 0.0))
            st_r, st_f = st[0], st[1]
            ok = (np.isfinite(U).all(axis=1) & np.isfinite(logj) & np.isfinite(rates).all(axis=1)
                  & (freqs > 0.0).all(axis=1))
            if self.clock_estimated:
                ok &= np.isfinite(st[2]) & (st[2] > 0.0)
        if not ok.any():
            return lp, G
        idx = np.flatnonzero(ok)
        params = np.concatenate([rates[idx], freqs[idx]], axis=1)
        tblens = np.broadcast_to(self.blens, (idx.size, self.B))
        if self.has_clock:
            mu = st[2][idx] if self.clock_estimated else np.full(idx.size, self.clock_fixed)
            rows = self.lik.evaluate_rows_clock(tblens, params, mu)
        else:
            rows = self.lik.evaluate_rows(tblens, params)
        val = rows[:, 0] + logj[idx]
        if self.clock_estimated:
            a, b = self.clock_prior
            val = val + a * U[idx, self.nfree] - b * mu
        if not propto:
            val = val + self.const
        if need_grad:
            g_rates = rows[:, 1 + self.B:1 + self.B + self.R]
            g_freqs = rows[:, 1 + self.B + self.R:1 + self.B + self.R + self.K]
            sub = (st_r[idx], tuple(s[idx] for s in st_f))
            blocks = [self.t_rates.backward(sub[0], g_rates, 1.0), self.t_freqs.backward(sub[1], g_freqs, 1.0)]
            if self.clock_estimated:
                blocks.append((mu * rows[:, -1] + a - b * mu)[:, None])
            g = np.concatenate(blocks, axis=1)
            fin = np.isfinite(val) & np.isfinite(g).all(axis=1)
            G[idx[fin]] = g[fin]
        else:
            fin = np.isfinite(val)
        lp[idx[fin]] = val[fin]
        return lp, G

    def log_prob(self, U, propto=True):
        return self.log_prob_grad(U, propto=propto, need_grad=False)[0]

    def initialize(self, rng, radius=2.0, max_tries=100):
        """Stan's random initialisation: uniform(-2, 2) until the density and its gradient are finite."""
        for _ in range(max_tries):
            q = rng.uniform(-radius, radius, self.dim)
            lp, G = self.log_prob_grad(q[None])
            if np.isfinite(lp[0]) and np.all(np.isfinite(G[0])):
                return q
        raise RuntimeError("Initialization failed after %d attempts" % max_tries)

    def column_names(self):
        return (["rates_geo.%d" % (k + 1) for k in range(self.R)] +
                ["freqs_geo.%d" % (k + 1) for k in range(self.K)] +
                (["rate_geo"] if self.clock_estimated else []))

    def flat_rows(self, U):
        rates, freqs, _, st = self.constrain(U)
        return np.concatenate([rates, freqs] + ([st[2][:, None]] if self.clock_estimated else []), axis=1)


class _RowsWithoutBlens:
    """What ``GeoPosterior`` calls, on a tree-sample likelihood: its branch
    lengths are the context's, so the (empty) ``blens`` argument is dropped."""

    def __init__(self, likelihood):
        self.lik = likelihood

    def evaluate_rows(self, blens, params):
        return self.lik.evaluate_rows(params)

    def evaluate_rows_clock(self, blens, params, clock):
        return self.lik.evaluate_rows_clock(params, clock)


class GeoTreesPosterior(GeoPosterior):
    """log p(rates_geo, freqs_geo | locations, tree sample): ``GeoPosterior``
    with the mixture likelihood over the sample in place of one tree's.
    ``likelihood`` offers ``evaluate_rows(params [n, R + K])`` with rows ``[log
    L_mix, d/drates, d/dfreqs]`` (``GeoTreesLikelihood``); the same parameters,
    transforms and priors, no branch-length block in the rows.  With a clock it
    offers ``evaluate_rows_clock(params, clock [n])`` (one more entry, d/dmu);
    the default prior's rate b is ``likelihood.mean_length``, the
    ``w_t``-weighted mean total length of the sample (the prior does not depend
    on the tree inside the mixture)."""

    def __init__(self, K, likelihood, clock=None, clock_prior=None):
        super().__init__(K, np.zeros(0), _RowsWithoutBlens(likelihood), clock=clock, clock_prior=clock_prior,
                         mean_length=getattr(likelihood, "mean_length", None) if clock == "estimate" else None)
        self.trees = likelihood
