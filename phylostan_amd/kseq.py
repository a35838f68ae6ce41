"""The K-state sequence likelihood on the host: an alignment of P patterns and
C rate categories under a reversible model of 2 <= K <= 64 states (codon models
are K = 61).

``kseq_host`` is the derivation a device engine for it has to follow, in numpy:
one symmetric eigendecomposition per draw (LAPACK ``eigh``), pruning in the
eigenbasis with power-of-two rescaling per node, pattern and category, the
reverse pass, W = sum (a c^T) o Phi with the three-arm rule of the K-state geo
engine (``csrc/geo_phases.inc``), sym(V W V^T) and the chain rule to rates and
freqs.  It returns log L, its full gradient and the site log-likelihoods, and is
what the CPU tests run on.  ``DeviceKStateLikelihood`` is the same likelihood on
the device engine (``csrc/kseq_engine.inc``), the one ``run
--codon`` takes from the command line; ``plan_kseq`` is its device-free planner.

Params per draw ``[rates R][freqs K][rs C][ps C]``, R = K(K-1)/2 in
``geo.rate_pairs`` order; row per draw ``[log L][d/dblens B][d/drs C][d/dps C]
[d/drates R][d/dfreqs K]``.

A mixture of M such models over sites (codon site models: one omega a
component) is ``kseq_mix_host``, ``HostKStateMixLikelihood`` and, on the same
device kernels (``phy_kseq_mix_*``), ``DeviceKStateMixLikelihood``: params
``[rates_0 R][freqs_0 K] .. [rs M C][ps M C]``, row ``[log L][d/dblens B]
[d/drs M C][d/dps M C][d/drates_0 R][d/dfreqs_0 K] ..``, and the posterior
probability of each component at each pattern.  M = 1 is the single model.

Its posterior summaries -- the internal nodes' state posteriors and the expected
number of labelled substitutions per branch (codon models: synonymous and
nonsynonymous) -- are ``kseq_sum_host``, ``HostKStateSummaries`` and, on the
device (``csrc/kseq_sum.inc``, ``phy_kseq_sum_*``), ``DeviceKStateSummaries``.
"""
import numpy as np

from .geo import rate_count, rate_pairs

KMIN, KMAX, CMAX = 2, 64, 16
MMAX = 8  # components of a mixture; M * C <= CMAX
PHI_TIE, PHI_NEAR, PHI_SERIES = 1e-12, 1e-5, 1e-3
DEAD_BELOW = 900.0  # bits a category that is not alive may lie below shmin and keep its rel (``_site_phase``)


def param_len(K, C):
    return rate_count(K) + K + 2 * C


def row_len(B, K, C):
    return 1 + B + 2 * C + rate_count(K) + K


def mix_param_len(K, M, C):
    """``[rates_0 R][freqs_0 K] .. [rates_{M-1}][freqs_{M-1}][rs M C][ps M C]``."""
    return M * (rate_count(K) + K) + 2 * M * C


def mix_row_len(B, K, M, C):
    """``[log L][d/dblens B][d/drs M C][d/dps M C][d/drates_0 R][d/dfreqs_0 K] ..``."""
    return 1 + B + 2 * M * C + M * (rate_count(K) + K)


def num_branches(S, rooted):
    return 2 * S - 2 if rooted else 2 * S - 3


def onehot_masks(states):
    """uint64 masks of integer states (any shape)."""
    return np.left_shift(np.uint64(1), np.asarray(states).astype(np.uint64))


def full_mask(K):
    return np.uint64((1 << K) - 1)


def mask_partials(masks, K):
    """[..., K] 0 / 1 partials of uint64 masks."""
    m = np.asarray(masks, np.uint64)
    return ((m[..., None] >> np.arange(K, dtype=np.uint64)) & np.uint64(1)).astype(float)


def phi_matrix(lam, t):
    """Phi_kl = (e^{lam_k t} - e^{lam_l t}) / (lam_k - lam_l), the three-arm
    rule of the device (``phi_rinv`` / ``phi_close``): the quotient outside the
    near window, the series of expm1(x) / x inside it, t e^{lam_k t} at a tie.
    The quotient is taken of expm1(lam t): on a short branch both exponentials
    are near 1 and their own difference keeps 1e-16 / (lam t) of it."""
    e = np.exp(lam * t)
    em = np.expm1(lam * t)
    d = lam[:, None] - lam[None, :]
    scale = np.maximum(1.0, np.abs(lam))[:, None]
    near = np.abs(d) < PHI_NEAR * scale
    tie = np.abs(d) < PHI_TIE * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        quot = (em[:, None] - em[None, :]) / d
    x = d * t
    series = t * e[None, :] * (1.0 + x * (0.5 + x * (1.0 / 6.0 + x * (1.0 / 24.0 + x / 120.0))))
    close = np.where(np.abs(x) < PHI_SERIES, series, quot)
    close = np.where(tie, t * e[:, None] * np.ones_like(d), close)
    return np.where(near, close, quot)


def _bad_row(B, K, C, P, M=1):
    row = np.zeros(mix_row_len(B, K, M, C))
    row[0] = -np.inf
    return row, np.full(P, -np.inf)


def _scalars_ok(blens, rs, ps):
    return bool(np.all(np.isfinite(rs)) and np.all(rs >= 0) and np.all(np.isfinite(ps)) and np.all(ps >= 0)
                and np.all(np.isfinite(blens)))


class _Eigen:
    """One model's A = D^1/2 (Qu / s) D^-1/2 = V diag(lam) V^T; ``ok`` False where it has none."""

    def __init__(self, rates, freqs):
        K = freqs.size
        self.ok = False
        self.rates, self.freqs = rates, freqs
        if not (np.all(np.isfinite(freqs)) and np.all(freqs > 0) and np.all(np.isfinite(rates)) and np.all(rates >= 0)):
            return
        self.pairs = pairs = np.asarray(rate_pairs(K), np.int64).reshape(-1, 2)
        self.Rm = Rm = np.zeros((K, K))
        Rm[pairs[:, 0], pairs[:, 1]] = rates
        Rm[pairs[:, 1], pairs[:, 0]] = rates
        self.qd = qd = -(Rm @ freqs)
        self.s = s = float(-np.dot(qd, freqs))
        if not (s > 0 and np.isfinite(s)):
            return
        self.sq = sq = np.sqrt(freqs)
        self.isq = 1.0 / sq
        A = (sq[:, None] * sq[None, :]) * Rm / s
        A[np.arange(K), np.arange(K)] = qd / s
        try:
            self.lam, self.V = np.linalg.eigh(A)
        except np.linalg.LinAlgError:
            return
        self.ok = True


class _Tree:
    def __init__(self, part0, peel, rooted):
        self.part0, self.peel, self.rooted = part0, peel, rooted
        self.S, self.P, self.K = part0.shape
        self.root = 2 * self.S - 2
        self.last = len(peel) - 1
        self.merged = None if rooted else int(peel[self.last][1])

    def low(self, store, n):
        return self.part0[n].T if n < self.S else store[n]


def _up_phase(tr, eg, blens, rs):
    """The way up of one model, per category: eigen coordinates, messages, scaled partials; the column shifts
    and L_c, ``[C, P]`` each.  A message is P(t) x = x + (P(t) - I) x, the second term through expm1(lam t): V V^T
    is the identity to 1e-16 only, which is 1e-16 / (q t) of a transition probability q t; at t = 0 it is x."""
    C = rs.size
    lam, V, sq, isq = eg.lam, eg.V, eg.sq, eg.isq
    LT = lam[None, None, :] * (blens[None, :, None] * rs[:, None, None])  # [C][B][K]
    E, EM = np.exp(LT), np.expm1(LT)
    LOW = [dict() for _ in range(C)]
    CC = [dict() for _ in range(C)]
    MSG = [dict() for _ in range(C)]
    SF = [dict() for _ in range(C)]
    shifts = np.zeros((C, tr.P))
    Lc = np.zeros((C, tr.P))
    for c in range(C):
        for r, (a, b, p) in enumerate(tr.peel):
            a, b, p = int(a), int(b), int(p)
            for ch in (a, b):
                if ch == tr.merged and r == tr.last:
                    continue
                CC[c][ch] = V.T @ (sq[:, None] * tr.low(LOW[c], ch))
                MSG[c][ch] = tr.low(LOW[c], ch) + isq[:, None] * (V @ (EM[c, ch][:, None] * CC[c][ch]))
            x = MSG[c][a] * (tr.low(LOW[c], b) if (b == tr.merged and r == tr.last) else MSG[c][b])
            mx = x.max(axis=0)
            with np.errstate(divide="ignore"):
                ex = np.where(mx > 0, -np.floor(np.log2(np.where(mx > 0, mx, 1.0))), 0.0)
            ex = np.where((mx > 0) & (mx < 2.0 ** -64), np.minimum(ex, 1000.0), 0.0)
            fac = np.exp2(ex)
            LOW[c][p] = x * fac[None, :]
            SF[c][p] = fac
            shifts[c] += ex
        Lc[c] = eg.freqs @ LOW[c][tr.root]
    return {"E": E, "EM": EM, "LOW": LOW, "CC": CC, "MSG": MSG, "SF": SF, "shifts": shifts, "Lc": Lc}


def _site_phase(weights, shifts, Lc, ps):
    """The patterns of one draw over all its categories (of every component, for a mixture): None for a draw
    without a likelihood, else log L, site log L, w_i / L_i, rel = 2^-(shift - shmin) and the live terms
    ps L rel, ``[G, P]``."""
    alive = (Lc > 0) & (ps[:, None] > 0)
    shmin = np.where(alive, shifts, np.inf).min(axis=0)
    shmin = np.where(np.isfinite(shmin), shmin, 0.0)
    # 2^-(shift_c - shmin).  A live category's shift is shmin or above.  One that is not alive (L_c = 0 exactly, the
    # +I category at a variable pattern, or ps_c = 0) can lie any distance below it, and 2^1024 is inf, which the way
    # down would multiply by its zeros: past DEAD_BELOW bits it takes no part (what it could add to the gradient
    # is L_c 2^900 times a live term: nothing, or not a number of fp64); the exponent stays within DEAD_BELOW.
    d = shifts - shmin[None, :]
    rel = np.where(~alive & (d < -DEAD_BELOW), 0.0, np.exp2(-np.clip(d, -DEAD_BELOW, DEAD_BELOW)))
    terms = np.where(alive, ps[:, None] * Lc * rel, 0.0)
    Ls = np.sum(terms, axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        site = np.where(Ls > 0, np.log(Ls) - shmin * np.log(2.0), -np.inf)
    if np.any((weights > 0) & ~((Ls > 0) & np.isfinite(Ls))):
        return None
    ll = float(np.sum(np.where(weights > 0, weights * np.where(weights > 0, site, 0.0), 0.0)))
    if not np.isfinite(ll):
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        down0 = np.where((weights > 0) & (Ls > 0), weights / Ls, 0.0)
    return {"ll": ll, "site": site, "down0": down0, "rel": rel, "terms": terms, "Ls": Ls}


def _down_phase(tr, eg, blens, rs, ps, up, down0, rel, gb):
    """The way down of one model: d/dblens added into ``gb``; d/drs, d/dps, W, dvec and the root term."""
    C, K = rs.size, tr.K
    lam, V, sq, isq = eg.lam, eg.V, eg.sq, eg.isq
    E, EM, LOW, CC, MSG, SF, Lc = up["E"], up["EM"], up["LOW"], up["CC"], up["MSG"], up["SF"], up["Lc"]
    grs = np.zeros(C)
    gps = np.zeros(C)
    W = np.zeros((K, K))
    dvec = np.zeros(K)
    rootpi = np.zeros(K)
    for c in range(C):
        down = down0 * rel[c]
        gps[c] = np.sum(down * Lc[c])
        UP = {tr.root: (down * ps[c])[None, :] * eg.freqs[:, None]}
        rootpi += (LOW[c][tr.root] * (down * ps[c])[None, :]).sum(axis=1)
        for r in range(tr.last, -1, -1):
            a, b, p = (int(v) for v in tr.peel[r])
            upp = UP[p] * SF[c][p][None, :]
            fold = (b == tr.merged and r == tr.last)
            mb = tr.low(LOW[c], b) if fold else MSG[c][b]
            todo = [(a, upp * mb)]
            if fold:
                UP[b] = upp * MSG[c][a]
            else:
                todo.append((b, upp * MSG[c][a]))
            for ch, ut in todo:
                aa = V.T @ (isq[:, None] * ut)
                e = E[c, ch]
                G = float(np.sum(aa * (lam * e)[:, None] * CC[c][ch]))
                gb[ch] += rs[c] * G
                grs[c] += blens[ch] * G
                du = sq[:, None] * (V @ (EM[c, ch][:, None] * aa))  # up - ut, as the message is low + (msg - low)
                UP[ch] = ut + du
                low = tr.low(LOW[c], ch)
                dvec += (du * low).sum(axis=1) - (ut * (MSG[c][ch] - low)).sum(axis=1)
                W += (aa @ CC[c][ch].T) * phi_matrix(lam, blens[ch] * rs[c])
    return grs, gps, W, dvec, rootpi


def _chain_phase(eg, W, dvec, rootpi):
    """dlogL/dA = sym(V W V^T), then the chain rule of A = D^1/2 Q D^-1/2, Q = Qu / s: d/drates, d/dfreqs."""
    K = eg.freqs.size
    V, sq, isq, Rm, qd, s, freqs, pairs = eg.V, eg.sq, eg.isq, eg.Rm, eg.qd, eg.s, eg.freqs, eg.pairs
    Gm = V @ W @ V.T
    Ws = 0.5 * (Gm + Gm.T)
    X = Ws * sq[:, None] * isq[None, :]
    Qu = Rm * freqs[None, :]
    Qu[np.arange(K), np.arange(K)] = qd
    ds = -float(np.sum(X * Qu)) / (s * s)
    dd = np.diag(X) / s - ds * freqs
    O = X / s - dd[:, None]
    g_rates = O[pairs[:, 0], pairs[:, 1]] * freqs[pairs[:, 1]] + O[pairs[:, 1], pairs[:, 0]] * freqs[pairs[:, 0]]
    offd = O * Rm  # Rm's diagonal is 0
    g_freqs = 0.5 * dvec / freqs - ds * qd + offd.sum(axis=0) + rootpi
    return g_rates, g_freqs


def _kseq_mix_draw(part0, weights, peel, rooted, blens, comps, rs, ps):
    """One draw of the mixture: ``comps`` a list of M (rates, freqs), ``rs`` and ``ps`` ``[M, C]``.  The row, the
    site log-likelihoods and the components' posteriors ``[M, P]``."""
    S, P, K = part0.shape
    M, C = rs.shape
    B = num_branches(S, rooted)
    bad = _bad_row(B, K, C, P, M) + (np.zeros((M, P)),)
    if not _scalars_ok(blens, rs, ps):
        return bad
    eigs = [_Eigen(rates, freqs) for rates, freqs in comps]
    if not all(e.ok for e in eigs):
        return bad
    tr = _Tree(part0, peel, rooted)
    ups = [_up_phase(tr, eigs[m], blens, rs[m]) for m in range(M)]
    st = _site_phase(weights, np.concatenate([u["shifts"] for u in ups]), np.concatenate([u["Lc"] for u in ups]),
                     ps.reshape(-1))
    if st is None:
        return bad
    gb = np.zeros(B)
    grs, gps, blocks = [], [], []
    for m in range(M):  # d/dblens folds in component, then category order
        x, y, W, dvec, rootpi = _down_phase(tr, eigs[m], blens, rs[m], ps[m], ups[m], st["down0"],
                                            st["rel"][m * C:(m + 1) * C], gb)
        grs.append(x)
        gps.append(y)
        blocks.extend(_chain_phase(eigs[m], W, dvec, rootpi))
    with np.errstate(divide="ignore", invalid="ignore"):
        post = np.where(st["Ls"] > 0, st["terms"].reshape(M, C, P).sum(axis=1) / st["Ls"], 0.0)
    return np.concatenate([[st["ll"]], gb] + grs + gps + blocks), st["site"], post


def _kseq_draw(part0, weights, peel, rooted, blens, rates, freqs, rs, ps):
    row, site, _ = _kseq_mix_draw(part0, weights, peel, rooted, blens, [(rates, freqs)], rs[None], ps[None])
    return row, site


def _host_data(who, tipmasks, weights, peel, blens, params, K, rooted):
    masks = np.asarray(tipmasks, np.uint64)
    S, P = masks.shape
    B = num_branches(S, rooted)
    if blens.shape[1] != B:
        raise ValueError("%s: blens has %d columns, the tree has %d branches" % (who, blens.shape[1], B))
    return mask_partials(masks, K), np.asarray(weights, float), np.asarray(peel), B, P


def kseq_host(tipmasks, weights, peel, rooted, blens, params, C):
    """Rows ``[n, row_len]`` and site log-likelihoods ``[n, P]`` of the draws
    ``blens [n, B]``, ``params [n, R + K + 2C]``; the number of states is read
    from the params' width."""
    blens, params = np.atleast_2d(np.asarray(blens, float)), np.atleast_2d(np.asarray(params, float))
    width = params.shape[1] - 2 * C
    K = int(round((np.sqrt(8.0 * width + 1.0) - 1.0) / 2.0))
    if rate_count(K) + K != width:
        raise ValueError("kseq_host: params of width %d fit no K at C = %d" % (params.shape[1], C))
    R = rate_count(K)
    part0, weights, peel, B, P = _host_data("kseq_host", tipmasks, weights, peel, blens, params, K, rooted)
    rows = np.empty((blens.shape[0], row_len(B, K, C)))
    site = np.empty((blens.shape[0], P))
    for n in range(blens.shape[0]):
        p = params[n]
        rows[n], site[n] = _kseq_draw(part0, weights, peel, bool(rooted), blens[n], p[:R], p[R:R + K],
                                      p[R + K:R + K + C], p[R + K + C:])
    return rows, site


def kseq_mix_host(tipmasks, weights, peel, rooted, blens, params, K, M, C):
    """The mixture of M models over sites, L_i = sum_m sum_c ps[m][c] L_i(Q_m, t rs[m][c], pi_m): rows
    ``[n, mix_row_len]``, site log-likelihoods ``[n, P]`` and the components' posterior probabilities
    ``[n, M, P]`` of the draws ``blens [n, B]``, ``params [n, M (R + K) + 2 M C]``.  The numpy restatement the
    device (``phy_kseq_mix_eval``) follows; at M = 1 it is ``kseq_host``."""
    blens, params = np.atleast_2d(np.asarray(blens, float)), np.atleast_2d(np.asarray(params, float))
    if not (1 <= M <= MMAX) or C < 1 or M * C > CMAX:
        raise ValueError("kseq_mix_host: M = %d, C = %d: supported M 1..%d, M * C <= %d" % (M, C, MMAX, CMAX))
    if params.shape[1] != mix_param_len(K, M, C):
        raise ValueError("kseq_mix_host: params must be [n, %d] at K = %d, M = %d, C = %d"
                         % (mix_param_len(K, M, C), K, M, C))
    R = rate_count(K)
    part0, weights, peel, B, P = _host_data("kseq_mix_host", tipmasks, weights, peel, blens, params, K, rooted)
    n = blens.shape[0]
    rows = np.empty((n, mix_row_len(B, K, M, C)))
    site = np.empty((n, P))
    post = np.empty((n, M, P))
    for k in range(n):
        p = params[k]
        comps = [(p[m * (R + K):m * (R + K) + R], p[m * (R + K) + R:(m + 1) * (R + K)]) for m in range(M)]
        tail = p[M * (R + K):]
        rows[k], site[k], post[k] = _kseq_mix_draw(part0, weights, peel, bool(rooted), blens[k], comps,
                                                   tail[:M * C].reshape(M, C), tail[M * C:].reshape(M, C))
    return rows, site, post


class HostKStateLikelihood:
    """``evaluate_rows(blens [n, B], params [n, R + K + 2C])`` on ``kseq_host``:
    the likelihood object ``codon.CodonPosterior`` and ``cli.run --codon`` take."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, C):
        self.masks = np.ascontiguousarray(tipmasks, np.uint64)
        self.weights = np.asarray(weights, float)
        self.peel = np.asarray(peel0, np.int32)
        self.rooted, self.K, self.C = bool(rooted), K, C
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, rooted)
        self.calls = 0

    def evaluate_rows(self, blens, params, site_ll=False):
        self.calls += 1
        if np.atleast_2d(params).shape[1] != param_len(self.K, self.C):
            raise ValueError("params must be [n, %d] at K = %d, C = %d" % (param_len(self.K, self.C), self.K, self.C))
        rows, site = kseq_host(self.masks, self.weights, self.peel, self.rooted, blens, params, self.C)
        return (rows, site) if site_ll else rows

    def close(self):
        pass


def _ptr(a):
    return a.ctypes.data


def _checked_data(tipmasks, weights, peel0, K, C):
    """The alignment and tree as the library takes them; ``ValueError`` for a wrong dtype or shape, before
    the library is touched."""
    masks = np.asarray(tipmasks)
    if masks.dtype.kind not in "ui":
        raise ValueError("tipmasks must be integer masks (uint64), got dtype %s" % masks.dtype)
    if masks.ndim != 2:
        raise ValueError("tipmasks must be [S, P], got shape %s" % (masks.shape,))
    if masks.dtype.kind == "i" and masks.size and masks.min() < 0:
        raise ValueError("tipmasks must not be negative")
    masks = np.ascontiguousarray(masks, np.uint64)
    S, P = masks.shape
    w = np.ascontiguousarray(weights, np.float64)
    if w.shape != (P,):
        raise ValueError("weights must be [%d], got shape %s" % (P, w.shape))
    peel = np.asarray(peel0)
    if peel.dtype.kind not in "ui" or peel.shape != (S - 1, 3):
        raise ValueError("peel must be integer [%d, 3], got %s of shape %s" % (S - 1, peel.dtype, peel.shape))
    peel = np.ascontiguousarray(peel, np.int32)
    if not (KMIN <= int(K) <= KMAX) or not (1 <= int(C) <= CMAX):
        raise ValueError("K = %s, C = %s: supported K %d..%d, C 1..%d" % (K, C, KMIN, KMAX, CMAX))
    return masks, w, peel


def check_draws(blens, params, B, K, C):
    """A call's draws as contiguous float64 ``blens [n, B]`` and ``params [n, R + K + 2C]``; ``ValueError`` for
    another shape, before the library is touched."""
    blens = np.atleast_2d(np.ascontiguousarray(blens, np.float64))
    params = np.atleast_2d(np.ascontiguousarray(params, np.float64))
    if params.ndim != 2 or params.shape[1] != param_len(K, C):
        raise ValueError("params must be [n, %d] at K = %d, C = %d" % (param_len(K, C), K, C))
    if blens.ndim != 2 or blens.shape[1] != B or blens.shape[0] != params.shape[0]:
        raise ValueError("blens must be [%d, %d], got %s" % (params.shape[0], B, blens.shape))
    return blens, params


PLAN_FACTS = ("KT", "tiles", "items_per_draw", "chunk_draws", "threads", "workgroups", "draw_workgroups", "lds_up",
              "lds_down", "lds_draw", "ws_doubles", "slot_doubles", "rec_doubles", "row_len", "B", "workspace_bytes")


def plan_kseq(tipmasks, weights, peel0, rooted, K, C, max_draws=1, cu_count=256):
    """The device-free planner's numbers (``csrc/kseq_plan.h`` through ``phy_kseq_plan``) for a device of
    ``cu_count`` compute units; its refusals raise ``PhyloHipError``."""
    from . import _lib
    masks, w, peel = _checked_data(tipmasks, weights, peel0, K, C)
    lib = _lib.load()
    facts = np.zeros(len(PLAN_FACTS), np.int64)
    _lib.check(lib.phy_kseq_plan(masks.shape[0], masks.shape[1], int(K), int(C), int(bool(rooted)), _ptr(masks),
                                 _ptr(w), _ptr(peel), int(max_draws), int(cu_count), _ptr(facts)), "phy_kseq_plan")
    return dict(zip(PLAN_FACTS, (int(v) for v in facts)))


class DeviceKStateLikelihood:
    """``HostKStateLikelihood``'s interface on the device engine (``phy_kseq_*``).  A call of more than
    ``max_draws`` draws is split into several; the arrays handed to the library are kept for the context's
    life."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, C, max_draws=64, device=0):
        self.ctx = None
        self.masks, self.weights, self.peel = _checked_data(tipmasks, weights, peel0, K, C)
        self.rooted, self.K, self.C = bool(rooted), int(K), int(C)
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, self.rooted)
        self.max_draws = int(max_draws)
        if self.max_draws < 1:
            raise ValueError("max_draws must be >= 1")
        self.calls = 0
        import ctypes

        from . import _lib
        self._lib = _lib
        self.lib = _lib.load()
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_kseq_create(self.S, self.P, self.K, self.C, int(self.rooted), _ptr(self.masks),
                                            _ptr(self.weights), _ptr(self.peel), self.max_draws, int(device),
                                            ctypes.byref(ctx)), "phy_kseq_create")
        self.ctx = ctx
        self.row_len = row_len(self.B, self.K, self.C)
        if self.lib.phy_kseq_row_len(self.ctx) != self.row_len or self.lib.phy_kseq_num_branches(self.ctx) != self.B:
            raise _lib.PhyloHipError("phy_kseq_create: the library's row does not match kseq.row_len")

    def evaluate_rows(self, blens, params, site_ll=False):
        blens, params = check_draws(blens, params, self.B, self.K, self.C)
        if self.ctx is None:
            raise self._lib.PhyloHipError("DeviceKStateLikelihood is closed")
        self.calls += 1
        n = blens.shape[0]
        rows = np.empty((n, self.row_len))
        site = np.empty((n, self.P)) if site_ll else None
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            bl, pr, out = blens[lo:hi], params[lo:hi], rows[lo:hi]  # contiguous row slices
            st = site[lo:hi] if site_ll else None
            self._lib.check(self.lib.phy_kseq_eval(self.ctx, hi - lo, _ptr(bl), _ptr(pr), _ptr(out),
                                                   _ptr(st) if site_ll else None), "phy_kseq_eval")
        return (rows, site) if site_ll else rows

    def info(self, n=0):
        """The live plan and the Jacobi sweeps of the last call's first n draws."""
        sweeps = np.zeros(max(n, 1), np.int32)
        facts = np.zeros(len(PLAN_FACTS), np.int64)
        self._lib.check(self.lib.phy_kseq_info(self.ctx, int(n), _ptr(sweeps), _ptr(facts)), "phy_kseq_info")
        out = dict(zip(PLAN_FACTS, (int(v) for v in facts)))
        out["sweeps"] = [int(v) for v in sweeps[:n]]
        return out

    def close(self):
        if self.ctx is not None:
            self.lib.phy_kseq_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def _check_mix(K, M, C):
    if not (KMIN <= int(K) <= KMAX) or not (1 <= int(M) <= MMAX) or int(C) < 1 or int(M) * int(C) > CMAX:
        raise ValueError("K = %s, M = %s, C = %s: supported K %d..%d, M 1..%d, M * C <= %d"
                         % (K, M, C, KMIN, KMAX, MMAX, CMAX))


def check_mix_draws(blens, params, B, K, M, C):
    """``check_draws`` for the mixture's params ``[n, M (R + K) + 2 M C]``."""
    blens = np.atleast_2d(np.ascontiguousarray(blens, np.float64))
    params = np.atleast_2d(np.ascontiguousarray(params, np.float64))
    if params.ndim != 2 or params.shape[1] != mix_param_len(K, M, C):
        raise ValueError("params must be [n, %d] at K = %d, M = %d, C = %d" % (mix_param_len(K, M, C), K, M, C))
    if blens.ndim != 2 or blens.shape[1] != B or blens.shape[0] != params.shape[0]:
        raise ValueError("blens must be [%d, %d], got %s" % (params.shape[0], B, blens.shape))
    return blens, params


def _mix_result(rows, site, post, site_ll, class_post):
    out = (rows,) + ((site,) if site_ll else ()) + ((post,) if class_post else ())
    return out if len(out) > 1 else rows


class HostKStateMixLikelihood:
    """``evaluate_rows(blens [n, B], params [n, M (R + K) + 2 M C], site_ll=False, class_post=False)`` on
    ``kseq_mix_host``: rows, then the site log-likelihoods ``[n, P]`` and the components' posteriors
    ``[n, M, P]`` where asked.  The likelihood object ``codon.CodonSitesPosterior`` takes."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, M, C):
        _check_mix(K, M, C)
        self.masks = np.ascontiguousarray(tipmasks, np.uint64)
        self.weights = np.asarray(weights, float)
        self.peel = np.asarray(peel0, np.int32)
        self.rooted, self.K, self.M, self.C = bool(rooted), int(K), int(M), int(C)
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, rooted)
        self.calls = 0

    def evaluate_rows(self, blens, params, site_ll=False, class_post=False):
        self.calls += 1
        blens, params = check_mix_draws(blens, params, self.B, self.K, self.M, self.C)
        rows, site, post = kseq_mix_host(self.masks, self.weights, self.peel, self.rooted, blens, params, self.K,
                                         self.M, self.C)
        return _mix_result(rows, site, post, site_ll, class_post)

    def close(self):
        pass


def plan_kseq_mix(tipmasks, weights, peel0, rooted, K, M, C, max_draws=1, cu_count=256):
    """``plan_kseq`` for the mixture (``phy_kseq_mix_plan``): ``items_per_draw`` is M C tiles."""
    from . import _lib
    masks, w, peel = _checked_data(tipmasks, weights, peel0, K, 1)
    lib = _lib.load()
    facts = np.zeros(len(PLAN_FACTS), np.int64)
    _lib.check(lib.phy_kseq_mix_plan(masks.shape[0], masks.shape[1], int(K), int(M), int(C), int(bool(rooted)),
                                     _ptr(masks), _ptr(w), _ptr(peel), int(max_draws), int(cu_count), _ptr(facts)),
               "phy_kseq_mix_plan")
    return dict(zip(PLAN_FACTS, (int(v) for v in facts)))


class DeviceKStateMixLikelihood:
    """``HostKStateMixLikelihood``'s interface on the device engine (``phy_kseq_mix_*``, the kernels of
    ``DeviceKStateLikelihood``).  A call of more than ``max_draws`` draws is split into several; the arrays
    handed to the library are kept for the context's life."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, M, C, max_draws=64, device=0):
        self.ctx = None
        self.masks, self.weights, self.peel = _checked_data(tipmasks, weights, peel0, K, 1)
        _check_mix(K, M, C)
        self.rooted, self.K, self.M, self.C = bool(rooted), int(K), int(M), int(C)
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, self.rooted)
        self.max_draws = int(max_draws)
        if self.max_draws < 1:
            raise ValueError("max_draws must be >= 1")
        self.calls = 0
        import ctypes

        from . import _lib
        self._lib = _lib
        self.lib = _lib.load()
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_kseq_mix_create(self.S, self.P, self.K, self.M, self.C, int(self.rooted),
                                                _ptr(self.masks), _ptr(self.weights), _ptr(self.peel),
                                                self.max_draws, int(device), ctypes.byref(ctx)),
                   "phy_kseq_mix_create")
        self.ctx = ctx
        self.row_len = mix_row_len(self.B, self.K, self.M, self.C)
        if (self.lib.phy_kseq_mix_row_len(self.ctx) != self.row_len
                or self.lib.phy_kseq_mix_num_branches(self.ctx) != self.B):
            raise _lib.PhyloHipError("phy_kseq_mix_create: the library's row does not match kseq.mix_row_len")

    def evaluate_rows(self, blens, params, site_ll=False, class_post=False):
        blens, params = check_mix_draws(blens, params, self.B, self.K, self.M, self.C)
        if self.ctx is None:
            raise self._lib.PhyloHipError("DeviceKStateMixLikelihood is closed")
        self.calls += 1
        n = blens.shape[0]
        rows = np.empty((n, self.row_len))
        site = np.empty((n, self.P)) if site_ll else None
        post = np.empty((n, self.M, self.P)) if class_post else None
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            bl, pr, out = blens[lo:hi], params[lo:hi], rows[lo:hi]  # contiguous row slices
            self._lib.check(self.lib.phy_kseq_mix_eval(self.ctx, hi - lo, _ptr(bl), _ptr(pr), _ptr(out),
                                                       _ptr(site[lo:hi]) if site_ll else None,
                                                       _ptr(post[lo:hi]) if class_post else None),
                            "phy_kseq_mix_eval")
        return _mix_result(rows, site, post, site_ll, class_post)

    def info(self, n=0):
        """The live plan and the Jacobi sweeps ``[n][M]`` of the last call's first n draws."""
        sweeps = np.zeros(max(n, 1) * self.M, np.int32)
        facts = np.zeros(len(PLAN_FACTS), np.int64)
        self._lib.check(self.lib.phy_kseq_mix_info(self.ctx, int(n), _ptr(sweeps), _ptr(facts)), "phy_kseq_mix_info")
        out = dict(zip(PLAN_FACTS, (int(v) for v in facts)))
        out["sweeps"] = [[int(v) for v in r] for r in sweeps[:n * self.M].reshape(n, self.M)]
        return out

    def close(self):
        if self.ctx is not None:
            self.lib.phy_kseq_mix_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


# ---------------------------------------------------------------- posterior summaries (phy_kseq_sum_*)
LMAX = 4  # labellings of one summary context


def label_matrix(K, lab):
    """``[K, K]`` symmetric, zero diagonal, of a labelling ``[R]`` of the unordered state pairs."""
    pairs = np.asarray(rate_pairs(K), np.int64).reshape(-1, 2)
    out = np.zeros((K, K))
    out[pairs[:, 0], pairs[:, 1]] = lab
    out[pairs[:, 1], pairs[:, 0]] = lab
    return out


def check_labels(labels, K):
    """Labels as contiguous float64 ``[NL, R]``; ``ValueError`` for what ``phy_kseq_sum_create`` refuses."""
    labels = np.ascontiguousarray(labels, np.float64)
    if labels.ndim != 2 or labels.shape[1] != rate_count(K) or not (1 <= labels.shape[0] <= LMAX):
        raise ValueError("labels must be [1..%d, %d] at K = %d, got shape %s" % (LMAX, rate_count(K), K, labels.shape))
    if not (np.all(np.isfinite(labels)) and np.all(labels >= 0)):
        raise ValueError("labels must be finite and non-negative")
    return labels


def _down_phase_sum(tr, eg, blens, rs, ps, up, seed, rel, weights, BL, bc, shares):
    """The summaries' form of ``_down_phase`` for one model: seeded with ps rel / L_i (the weight apart), each
    node's share up o low of its state posterior added into ``shares``, and per branch <(a (w c)^T) o Phi, B_l>
    added into ``bc [NL, B]``."""
    lam, V, sq, isq = eg.lam, eg.V, eg.sq, eg.isq
    EM, LOW, CC, MSG, SF = up["EM"], up["LOW"], up["CC"], up["MSG"], up["SF"]
    for c in range(rs.size):
        down = seed * rel[c] * ps[c]
        UP = {tr.root: down[None, :] * eg.freqs[:, None]}
        shares[tr.root] = shares[tr.root] + UP[tr.root] * LOW[c][tr.root]
        for r in range(tr.last, -1, -1):
            a, b, p = (int(v) for v in tr.peel[r])
            upp = UP[p] * SF[c][p][None, :]
            fold = (b == tr.merged and r == tr.last)
            mb = tr.low(LOW[c], b) if fold else MSG[c][b]
            todo = [(a, upp * mb)]
            if fold:
                UP[b] = upp * MSG[c][a]
                shares[b] = shares[b] + UP[b] * LOW[c][b]
            else:
                todo.append((b, upp * MSG[c][a]))
            for ch, ut in todo:
                aa = V.T @ (isq[:, None] * ut)
                UP[ch] = ut + sq[:, None] * (V @ (EM[c, ch][:, None] * aa))
                if ch >= tr.S:
                    shares[ch] = shares[ch] + UP[ch] * LOW[c][ch]
                MP = (aa @ (CC[c][ch] * weights[None, :]).T) * phi_matrix(lam, blens[ch] * rs[c])
                for l in range(BL.shape[0]):
                    bc[l, ch] += float(np.sum(MP * BL[l]))


def _kseq_sum_draw(part0, weights, peel, rooted, blens, comps, rs, ps, labmats):
    """One draw: log L, counts ``[NL, B]``, node posteriors ``[S-1, K, P]``; -inf and zeros for a refused draw."""
    S, P, K = part0.shape
    M, C = rs.shape
    B = num_branches(S, rooted)
    bc, npost = np.zeros((labmats.shape[0], B)), np.zeros((S - 1, K, P))
    bad = (-np.inf, bc, npost)
    if not _scalars_ok(blens, rs, ps):
        return bad
    eigs = [_Eigen(rates, freqs) for rates, freqs in comps]
    if not all(e.ok for e in eigs):
        return bad
    tr = _Tree(part0, peel, rooted)
    ups = [_up_phase(tr, eigs[m], blens, rs[m]) for m in range(M)]
    st = _site_phase(weights, np.concatenate([u["shifts"] for u in ups]), np.concatenate([u["Lc"] for u in ups]),
                     ps.reshape(-1))
    if st is None:
        return bad
    Ls = st["Ls"]
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        seed = np.where((Ls > 0) & np.isfinite(Ls), 1.0 / Ls, 0.0)
    shares = {v: np.zeros((K, P)) for v in range(S, 2 * S - 1)}
    for m in range(M):
        eg = eigs[m]
        A = (eg.sq[:, None] * eg.sq[None, :]) * eg.Rm / eg.s  # D^1/2 Q D^-1/2 off the diagonal
        BL = np.stack([eg.V.T @ (A * lm) @ eg.V for lm in labmats])
        _down_phase_sum(tr, eg, blens, rs[m], ps[m], ups[m], seed, st["rel"][m * C:(m + 1) * C], weights, BL, bc,
                        shares)
    for v in range(S, 2 * S - 1):
        npost[v - S] = shares[v]
    return st["ll"], bc, npost


def kseq_sum_host(tipmasks, weights, peel, rooted, blens, params, K, M, C, labels):
    """The summaries of the draws ``blens [n, B]``, ``params [n, M (R + K) + 2 M C]`` (``kseq_mix_host``'s) under
    the labellings ``labels [NL, R]``: log L ``[n]``, the expected labelled substitution counts per branch
    ``[n, NL, B]`` and the internal nodes' state posteriors ``[n, S-1, K, P]``.  The numpy restatement the device
    (``phy_kseq_sum_eval``) follows, on ``_up_phase`` and ``_site_phase``."""
    blens, params = np.atleast_2d(np.asarray(blens, float)), np.atleast_2d(np.asarray(params, float))
    _check_mix(K, M, C)
    labels = check_labels(labels, K)
    if params.shape[1] != mix_param_len(K, M, C):
        raise ValueError("kseq_sum_host: params must be [n, %d] at K = %d, M = %d, C = %d"
                         % (mix_param_len(K, M, C), K, M, C))
    R = rate_count(K)
    part0, weights, peel, B, P = _host_data("kseq_sum_host", tipmasks, weights, peel, blens, params, K, rooted)
    S = part0.shape[0]
    labmats = np.stack([label_matrix(K, lab) for lab in labels])
    n = blens.shape[0]
    loglik, bcounts, npost = np.empty(n), np.empty((n, labels.shape[0], B)), np.empty((n, S - 1, K, P))
    for k in range(n):
        p = params[k]
        comps = [(p[m * (R + K):m * (R + K) + R], p[m * (R + K) + R:(m + 1) * (R + K)]) for m in range(M)]
        tail = p[M * (R + K):]
        loglik[k], bcounts[k], npost[k] = _kseq_sum_draw(part0, weights, peel, bool(rooted), blens[k], comps,
                                                         tail[:M * C].reshape(M, C), tail[M * C:].reshape(M, C),
                                                         labmats)
    return loglik, bcounts, npost


class HostKStateSummaries:
    """``DeviceKStateSummaries``' interface on ``kseq_sum_host``: ``evaluate(blens, params)`` gives log L
    ``[n]``, counts ``[n, NL, B]`` and node posteriors ``[n, S-1, K, P]``; ``reset`` / ``add`` / ``read`` keep the
    running sum of the finite draws' node posteriors."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, M, C, labels, max_draws=64, device=0):
        _check_mix(K, M, C)
        self.masks = np.ascontiguousarray(tipmasks, np.uint64)
        self.weights = np.asarray(weights, float)
        self.peel = np.asarray(peel0, np.int32)
        self.rooted, self.K, self.M, self.C = bool(rooted), int(K), int(M), int(C)
        self.labels = check_labels(labels, self.K)
        self.NL = self.labels.shape[0]
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, rooted)
        self.calls = 0
        self.reset()

    def evaluate(self, blens, params, node_post=True):
        self.calls += 1
        blens, params = check_mix_draws(blens, params, self.B, self.K, self.M, self.C)
        ll, bc, npost = kseq_sum_host(self.masks, self.weights, self.peel, self.rooted, blens, params, self.K,
                                      self.M, self.C, self.labels)
        return (ll, bc, npost) if node_post else (ll, bc)

    def reset(self):
        self._sum = np.zeros((self.S - 1, self.K, self.P))
        self._n = 0

    def add(self, blens, params):
        ll, bc, npost = self.evaluate(blens, params)
        for k in range(ll.size):
            if np.isfinite(ll[k]):
                self._sum = self._sum + npost[k]
                self._n += 1
        return ll, bc

    def read(self):
        return self._sum.copy(), self._n

    def close(self):
        pass


class DeviceKStateSummaries:
    """The summaries on the device engine (``phy_kseq_sum_*``, ``csrc/kseq_sum.inc``): ``HostKStateSummaries``'
    interface.  A call of more than ``max_draws`` draws is split into several; the arrays handed to the library
    are kept for the context's life."""

    def __init__(self, tipmasks, weights, peel0, rooted, K, M, C, labels, max_draws=64, device=0):
        self.ctx = None
        self.masks, self.weights, self.peel = _checked_data(tipmasks, weights, peel0, K, 1)
        _check_mix(K, M, C)
        self.rooted, self.K, self.M, self.C = bool(rooted), int(K), int(M), int(C)
        self.labels = check_labels(labels, self.K)
        self.NL = self.labels.shape[0]
        self.S, self.P = self.masks.shape
        self.B = num_branches(self.S, self.rooted)
        self.max_draws = int(max_draws)
        if self.max_draws < 1:
            raise ValueError("max_draws must be >= 1")
        self.calls = 0
        import ctypes

        from . import _lib
        self._lib = _lib
        self.lib = _lib.load()
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_kseq_sum_create(self.S, self.P, self.K, self.M, self.C, int(self.rooted),
                                                _ptr(self.masks), _ptr(self.weights), _ptr(self.peel), self.NL,
                                                _ptr(self.labels), self.max_draws, int(device), ctypes.byref(ctx)),
                   "phy_kseq_sum_create")
        self.ctx = ctx
        if self.lib.phy_kseq_sum_num_branches(self.ctx) != self.B:
            raise _lib.PhyloHipError("phy_kseq_sum_create: the library's branch count does not match")

    def _open(self):
        if self.ctx is None:
            raise self._lib.PhyloHipError("DeviceKStateSummaries is closed")

    def evaluate(self, blens, params, node_post=True):
        blens, params = check_mix_draws(blens, params, self.B, self.K, self.M, self.C)
        self._open()
        self.calls += 1
        n = blens.shape[0]
        ll, bc = np.empty(n), np.empty((n, self.NL, self.B))
        npost = np.empty((n, self.S - 1, self.K, self.P)) if node_post else None
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            bl, pr = blens[lo:hi], params[lo:hi]  # contiguous row slices
            self._lib.check(self.lib.phy_kseq_sum_eval(self.ctx, hi - lo, _ptr(bl), _ptr(pr), _ptr(ll[lo:hi]),
                                                       _ptr(bc[lo:hi]), _ptr(npost[lo:hi]) if node_post else None),
                            "phy_kseq_sum_eval")
        return (ll, bc, npost) if node_post else (ll, bc)

    def reset(self):
        self._open()
        self._lib.check(self.lib.phy_kseq_sum_reset(self.ctx), "phy_kseq_sum_reset")

    def add(self, blens, params):
        blens, params = check_mix_draws(blens, params, self.B, self.K, self.M, self.C)
        self._open()
        self.calls += 1
        n = blens.shape[0]
        ll, bc = np.empty(n), np.empty((n, self.NL, self.B))
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            bl, pr = blens[lo:hi], params[lo:hi]
            self._lib.check(self.lib.phy_kseq_sum_add(self.ctx, hi - lo, _ptr(bl), _ptr(pr), _ptr(ll[lo:hi]),
                                                      _ptr(bc[lo:hi])), "phy_kseq_sum_add")
        return ll, bc

    def read(self):
        import ctypes
        self._open()
        out = np.empty((self.S - 1, self.K, self.P))
        nf = ctypes.c_int(0)
        self._lib.check(self.lib.phy_kseq_sum_read(self.ctx, _ptr(out), ctypes.byref(nf)), "phy_kseq_sum_read")
        return out, int(nf.value)

    def close(self):
        if self.ctx is not None:
            self.lib.phy_kseq_sum_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
