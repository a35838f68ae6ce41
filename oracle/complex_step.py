"""Exact-derivative reference: the pruning log-likelihood in complex
arithmetic, from the parameters up, differentiated by the complex step.

TEST INFRASTRUCTURE ONLY (see ``oracle/__init__.py``).  CPU, numpy only.

Every other gradient reference of the suite shares algebra with the code it
checks: the C port runs the device's Jacobi eigensolver operation for
operation, and ``models.q_param_gradients`` evaluates the device's divided
differences ``Phi_kl`` with the device's tie rule.  This module shares none
of it:

1. ``Q(freqs, rates)`` as ``models.rate_matrix`` states it (JC69:
   ``numpy_pruner.jc69_q()``, no normalisation);
2. ``P = expm(Q rs_c b)`` by scaling and squaring of a Taylor series,
   written out below -- no eigendecomposition anywhere (no
   ``models.eigen_system``, ``numpy_pruner.model_matrices`` or
   ``np.linalg.eig*``);
3. Felsenstein pruning, the mixture and the root, with the merged root edge
   of an unrooted tree as ``numpy_pruner._prune`` treats it;
4. all of it on complex arrays, so that
5. ``d f / d theta_k = Im f(theta + i h e_k) / h`` with ``h = 1e-30``: no
   subtraction, hence no step-size error -- the derivative carries the
   rounding error of one function evaluation.

``root_freqs`` defaults to ``freqs``.  Perturbing ``root_freqs`` alone gives
``grad_freq_root``; perturbing ``freqs`` with the root tied to it gives
``grad_freqs`` as the output rows define it (the path through Q plus the
root term).  For JC69 only log L, ``site_ll`` and the ``blens`` / ``rs`` /
``ps`` / ``freq_root`` gradients mean anything.

dL/dP (16 C B entries) has NO complex-step pin: one evaluation per entry is
too many.  It stays pinned to the numpy oracle, and through it to the
``grad_blens``, ``grad_rs`` and Q-parameter gradients pinned here, all of
which are contractions of it.
"""
import numpy as np

from phylostan_amd.models import GTR_PAIRS

from .numpy_pruner import jc69_q, tip_vectors

STEP = 1e-30
_TAYLOR_TERMS = 20  # |X| <= 1/2: the first dropped term is 2^-21 / 21! ~ 1e-26


def rate_matrix(freqs, rates):
    """Normalised Q of ``models.rate_matrix`` on complex arrays."""
    f = np.asarray(freqs, complex)
    r = np.asarray(rates, complex)
    R = np.zeros((4, 4), complex)
    for k, (i, j) in enumerate(GTR_PAIRS):
        R[i, j] = R[j, i] = r[k]
    Qt = R * f[None, :]
    idx = np.arange(4)
    Qt[idx, idx] = 0.0
    Qt[idx, idx] = -Qt.sum(1)
    s = -np.dot(np.diag(Qt), f)
    return Qt / s


def expm(A):
    """exp of complex matrices ``A[..., 4, 4]``: each matrix scaled by its own
    power of two to a row-sum norm <= 1/2, a Taylor series, then squared
    back (a short branch is not scaled by a long one's power; each squaring
    doubles the rounding error, so no more of them than the series needs)."""
    A = np.asarray(A, complex)
    nrm = np.abs(A).sum(-1).max(-1)
    s = np.where(nrm > 0, np.ceil(np.log2(np.maximum(nrm, 1e-300))) + 1, 0.0)
    s = np.maximum(s, 0.0).astype(np.int64)
    X = A / np.exp2(s)[..., None, None]
    T = np.broadcast_to(np.eye(4, dtype=complex), A.shape).copy()
    term = T.copy()
    for k in range(1, _TAYLOR_TERMS + 1):
        term = term @ X / k
        T = T + term
    for j in range(int(s.max()) if s.size else 0):
        T = np.where((s > j)[..., None, None], T @ T, T)
    return T


def loglik(case, blens, freqs, rates, rs, ps, root_freqs=None):
    """(complex log L, complex site_ll[P]) of ``case``'s data and tree at the
    given (possibly complex) parameters."""
    f = np.asarray(freqs, complex)
    rf = f if root_freqs is None else np.asarray(root_freqs, complex)
    Q = jc69_q().astype(complex) if case.model == "JC69" else rate_matrix(f, rates)
    t = np.asarray(rs, complex)[:, None] * np.asarray(blens, complex)[None, :]  # [C, B]
    pm = expm(Q[None, None] * t[..., None, None])
    S, P = case.tipcodes.shape
    C = t.shape[0]
    peel = np.asarray(case.peel0, dtype=np.int64)
    root = int(peel[-1, 2])
    merged = None if case.rooted else int(peel[-1, 1])  # root child with no branch of its own
    part = {}
    for tip in range(S):
        part[tip] = np.broadcast_to(tip_vectors(case.tipcodes[tip]), (C, P, 4)).astype(complex)
    for x, y, v in peel:
        ax = np.einsum("cjk,cpk->cpj", pm[:, x], part[x])
        ay = part[y] if y == merged else np.einsum("cjk,cpk->cpj", pm[:, y], part[y])
        part[v] = ax * ay
    L = (np.asarray(ps, complex)[:, None] * np.einsum("j,cpj->cp", rf, part[root])).sum(0)
    site_ll = np.log(L)
    return np.dot(np.asarray(case.weights, np.float64), site_ll), site_ll


_PARAMS = ("blens", "freqs", "rates", "rs", "ps")


def _point(case):
    return {k: np.asarray(getattr(case, k), complex).copy() for k in _PARAMS}


def value(case):
    """(log L, site_ll[P]) at the case's own point, real."""
    ll, site = loglik(case, **_point(case))
    return float(ll.real), site.real.copy()


def gradients(case, only=None, branches=None):
    """Complex-step gradients of log L at the case's own point: a dict with
    ``blens, rs, ps, rates, freqs, freq_root`` (``freqs`` with the root tied,
    ``freq_root`` the root term alone), one complex evaluation per entry.
    ``only`` restricts the arrays; ``branches`` the entries of ``blens``
    (the returned array then has one entry per listed branch)."""
    names = ("blens", "rs", "ps", "rates", "freqs", "freq_root") if only is None else tuple(only)
    out = {}
    for name in names:
        param = "freqs" if name == "freq_root" else name
        idx = range(getattr(case, param).size)
        if name == "blens" and branches is not None:
            idx = list(branches)
        g = np.zeros(len(idx))
        for n, k in enumerate(idx):
            a = _point(case)
            if name == "freq_root":
                a["root_freqs"] = a["freqs"].copy()
                a["root_freqs"][k] += 1j * STEP
            else:
                a[name][k] += 1j * STEP
            g[n] = loglik(case, **a)[0].imag / STEP
        out[name] = g
    return out
