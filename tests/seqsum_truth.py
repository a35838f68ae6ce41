"""Truth for the sequence summaries, written independently of the product's
p o q / L form (TEST INFRASTRUCTURE ONLY).

* Node posterior by clamping: prune once more with part[v] multiplied by the
  unit vector e_s, and divide the site likelihood by the unclamped one.
* cat / rate from the per-category root sums.
* E[N_b] from the upper-right block of expm([[Q tau, Q_off tau], [0, Q tau]])
  (the integral int_0^tau e^{Qu} Q_off e^{Q(tau-u)} du), contracted with the
  oracle's dlogL/dP.
"""
import numpy as np

from oracle import numpy_pruner as npr


def _category_likelihoods(case, pm, clamp=None):
    """L_ci [C, P]; clamp = (node, state) keeps only that state at the node."""
    S, P = case.tipcodes.shape
    C = pm.shape[0]
    peel = np.asarray(case.peel0, np.int64)
    root = int(peel[-1, 2])
    merged = None if case.rooted else int(peel[-1, 1])
    part = {t: np.broadcast_to(npr.tip_vectors(case.tipcodes[t]), (C, P, 4)) for t in range(S)}
    for x, y, v in peel:
        ax = np.einsum("cjk,cpk->cpj", pm[:, x], part[x])
        ay = part[y] if y == merged else np.einsum("cjk,cpk->cpj", pm[:, y], part[y])
        pv = ax * ay
        if clamp is not None and clamp[0] == v:
            e = np.zeros(4)
            e[clamp[1]] = 1.0
            pv = pv * e
        part[v] = pv
    return np.asarray(case.ps)[:, None] * np.einsum("j,cpj->cp", np.asarray(case.freqs), part[root])


def matrices(case):
    return npr.model_matrices(npr.MODEL_IDS[case.model], case.freqs, case.rates, case.blens, case.rs)


def summaries(case):
    """dict(loglik, anc [S-1, 4, P], cat [C, P], rate [P]) of the case's point."""
    pm, _ = matrices(case)
    S, P = case.tipcodes.shape
    Lc = _category_likelihoods(case, pm)
    L = Lc.sum(axis=0)
    anc = np.zeros((S - 1, 4, P))
    for v in range(S, 2 * S - 1):
        for s in range(4):
            anc[v - S, s] = _category_likelihoods(case, pm, clamp=(v, s)).sum(axis=0) / L
    cat = Lc / L
    return dict(loglik=float(np.dot(case.weights, np.log(L))), anc=anc, cat=cat,
                rate=np.einsum("c,cp->p", np.asarray(case.rs), cat))


def truth_row(case):
    t = summaries(case)
    return np.concatenate([[t["loglik"]], t["anc"].ravel(), t["cat"].ravel(), t["rate"]])


def _expm(A):
    """exp of real square matrices A[..., n, n]: scaled to norm <= 1/2, a
    Taylor series to the rounding level, squared back."""
    A = np.asarray(A, np.float64)
    n = A.shape[-1]
    nrm = float(np.abs(A).sum(-1).max()) if A.size else 0.0
    s = max(0, int(np.ceil(np.log2(nrm))) + 1) if nrm > 0 else 0
    X = A / 2.0 ** s
    T = np.broadcast_to(np.eye(n), A.shape).copy()
    term = T.copy()
    for k in range(1, 25):
        term = term @ X / k
        T = T + term
    for _ in range(s):
        T = T @ T
    return T


def substitution_integrals(Q, blens, rs):
    """N[c, b] = int_0^tau e^{Qu} Q_off e^{Q(tau-u)} du, tau = rs_c blens_b,
    one block exponential per (c, b): each at its own scale."""
    Q = np.asarray(Q, np.float64)
    Qoff = Q - np.diag(np.diag(Q))
    rs, blens = np.asarray(rs, np.float64), np.asarray(blens, np.float64)
    N = np.zeros((rs.size, blens.size, 4, 4))
    for c in range(rs.size):
        for b in range(blens.size):
            tau = rs[c] * blens[b]
            M = np.zeros((8, 8))
            M[:4, :4] = M[4:, 4:] = Q * tau
            M[:4, 4:] = Qoff * tau
            N[c, b] = _expm(M)[:4, 4:]
    return N


def expected_substitutions(case, dLdP=None):
    """E[N_b] [B] from the oracle's dlogL/dP (or the one given)."""
    _, Q = matrices(case)
    if dLdP is None:
        dLdP = case.oracle()["dLdP"]
    return (np.asarray(dLdP) * substitution_integrals(Q, case.blens, case.rs)).sum(axis=(0, 2, 3))
