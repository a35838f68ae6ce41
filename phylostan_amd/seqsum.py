"""Posterior summaries of the sequence likelihood (include/phylo_hip_seqsum.h):
the marginal state distribution of every internal node at every pattern, every
pattern's rate-category posterior and mean rate, per draw or summed over draws
on the device.

``SequenceSummaries`` binds the device context.  ``seqsum_host`` is a numpy
restatement of the device's derivation with the same interface (the CPU suite
passes it to the CLI; product code never imports ``oracle/``).  ``SeqSummary``
accumulates a run's summaries: the means over the finite draws of the node
posteriors, category posteriors, site rates, expected substitutions per branch
(``models.expected_substitutions``) and branch lengths.

A row is ``[loglik, anc[S-1, 4, P], cat[C, P], rate[P]]``; ``split_row`` gives
the four views.  anc's node index is ``node id - S``, its states A, C, G, T.
"""
import ctypes

import numpy as np

from . import _lib, models


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def row_length(S, P, C):
    return 1 + (4 * (S - 1) + C + 1) * P


def split_row(row, S, P, C):
    """(loglik, anc [S-1, 4, P], cat [C, P], rate [P]) views of one row, or
    with a leading axis on each of rows [n, row_len]."""
    row = np.asarray(row)
    lead = row.shape[:-1]
    if row.shape[-1] != row_length(S, P, C):
        raise ValueError("row length %d, expected %d" % (row.shape[-1], row_length(S, P, C)))
    a = 1 + 4 * (S - 1) * P
    return (row[..., 0], row[..., 1:a].reshape(lead + (S - 1, 4, P)),
            row[..., a:a + C * P].reshape(lead + (C, P)), row[..., a + C * P:])


class _SummariesBase:
    """Shapes and the chunked ``add`` shared by the device and the host form."""

    def _inputs(self, blens, model_vecs):
        blens = np.ascontiguousarray(np.atleast_2d(blens), dtype=np.float64)
        mv = np.ascontiguousarray(np.atleast_2d(model_vecs), dtype=np.float64)
        n = blens.shape[0]
        if blens.shape != (n, self.B) or mv.shape != (n, self.model_len):
            raise ValueError("bad shapes: blens %s model %s" % (blens.shape, mv.shape))
        return blens, mv, n

    def split(self, row):
        return split_row(row, self.S, self.P, self.C)


class SequenceSummaries(_SummariesBase):
    """One tree (``peel0`` [S-1, 3], 0-based) on one alignment.
    ``evaluate_rows(blens, model_vecs)`` returns the draws' rows [n, row_len];
    ``reset`` / ``add`` / ``read`` keep their running sum on the device: the
    sum is sequential in draw order, bit for bit the left-to-right sum of the
    finite draws' rows however they are split into calls."""

    def __init__(self, tipcodes, weights, peel0, rooted, model, C, max_draws=64, device=0):
        self.lib = _lib.load()
        tipcodes = np.ascontiguousarray(tipcodes, dtype=np.uint8)
        self.S, self.P = tipcodes.shape
        self.C = int(C)
        self.rooted = bool(rooted)
        self.model = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        peel = np.ascontiguousarray(peel0, dtype=np.int32)
        if w.shape != (self.P,):
            raise ValueError("weights must have shape (P,)")
        if peel.shape != (self.S - 1, 3):
            raise ValueError("peel0 must have shape (S-1, 3)")
        self.max_draws = int(max_draws)
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_seqsum_create(self.S, self.P, self.C, int(self.rooted), self.model, _ptr(tipcodes),
                                              _ptr(w), _ptr(peel), self.max_draws, int(device), ctypes.byref(ctx)),
                   "phy_seqsum_create")
        self.ctx = ctx
        self.B = self.lib.phy_seqsum_num_branches(ctx)
        self.row_len = self.lib.phy_seqsum_row_len(ctx)
        self.model_len = 10 + 2 * self.C

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.phy_seqsum_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def evaluate_rows(self, blens, model_vecs):
        """Rows [n, row_len]; calls above ``max_draws`` are chunked (a row's
        bits do not depend on the chunking).  A rejected draw: -inf, zeros."""
        blens, mv, n = self._inputs(blens, model_vecs)
        out = np.empty((n, self.row_len))
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            _lib.check(self.lib.phy_seqsum_eval(self.ctx, hi - lo, _ptr(blens[lo:hi]), _ptr(mv[lo:hi]),
                                                _ptr(out[lo:hi])), "phy_seqsum_eval")
        return out

    def reset(self):
        _lib.check(self.lib.phy_seqsum_reset(self.ctx), "phy_seqsum_reset")

    def add(self, blens, model_vecs):
        """Adds the finite draws to the device sum, in draw order; returns the
        draws' log-likelihoods [n] (-inf: rejected, left out)."""
        blens, mv, n = self._inputs(blens, model_vecs)
        ll = np.empty(n)
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            _lib.check(self.lib.phy_seqsum_add(self.ctx, hi - lo, _ptr(blens[lo:hi]), _ptr(mv[lo:hi]),
                                               _ptr(ll[lo:hi])), "phy_seqsum_add")
        return ll

    def read(self):
        """(sums [row_len], the number of finite draws added since reset)."""
        row = np.empty(self.row_len)
        n = ctypes.c_int()
        _lib.check(self.lib.phy_seqsum_read(self.ctx, _ptr(row), ctypes.byref(n)), "phy_seqsum_read")
        return row, n.value


def plan_seqsum(tipcodes, peel0, rooted, C, max_draws, model="JC69"):
    """The plan ``SequenceSummaries`` would take (no device, no context;
    ``phy_seqsum_plan``)."""
    lib = _lib.load()
    tipcodes = np.ascontiguousarray(tipcodes, dtype=np.uint8)
    S, P = tipcodes.shape
    peel = np.ascontiguousarray(peel0, dtype=np.int32)
    w = np.ones(P)
    facts, order = np.zeros(8, np.int64), np.zeros(S - 1, np.int32)
    kind = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
    _lib.check(lib.phy_seqsum_plan(S, P, int(C), int(bool(rooted)), kind, _ptr(tipcodes), _ptr(w), _ptr(peel),
                                   int(max_draws), _ptr(facts), _ptr(order)), "phy_seqsum_plan")
    out = dict(zip(("row_len", "Ppad", "workgroups_per_draw", "workspace_bytes", "draw_bytes", "draws_per_launch",
                    "lds_bytes", "record_vectors"), [int(v) for v in facts]))
    out["order"] = [int(v) for v in order]
    return out


def transition_matrices(kind, freqs, rates, blens, rs):
    """P [C, B, 4, 4] (P[c, b][i, j]: i at the top of branch b, j below) as the
    device forms them: JC69's closed form, else V diag(exp(lam t)) V^-1."""
    t = np.asarray(rs, np.float64)[:, None] * np.asarray(blens, np.float64)[None, :]
    if kind == models.JC69:
        e = np.exp(-t / 0.75)
        P = np.empty(t.shape + (4, 4))
        P[...] = (0.25 - 0.25 * e)[..., None, None]
        idx = np.arange(4)
        P[..., idx, idx] = (0.25 + 0.75 * e)[..., None]
        return P
    _, lam, V, Vinv, _, _, _ = models.eigen_system(freqs, rates)
    E = np.exp(lam[None, None, :] * t[..., None])  # [C, B, 4]
    return np.einsum("ik,cbk,kj->cbij", V, E, Vinv)


class _SeqsumHost(_SummariesBase):
    def __init__(self, tipcodes, weights, peel0, rooted, model, C, max_draws=1 << 30, **_):
        self.tipcodes = np.asarray(tipcodes, np.uint8)
        self.weights = np.asarray(weights, np.float64)
        self.peel0 = np.asarray(peel0, np.int64)
        self.rooted = bool(rooted)
        self.model = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
        self.C = int(C)
        self.S, self.P = self.tipcodes.shape
        self.B = 2 * self.S - 2 if self.rooted else 2 * self.S - 3
        self.model_len = 10 + 2 * self.C
        self.row_len = row_length(self.S, self.P, self.C)
        self.max_draws = int(max_draws)
        self._tips = ((self.tipcodes[..., None] >> np.arange(4)) & 1).astype(np.float64)  # [S, P, 4]
        self.reset()

    def close(self):
        pass

    def _row(self, blens, mv):
        """One draw: part (forward) and q (pre-order) per node, then
        anc = sum_c ps_c part q / L, cat = L_c / L, rate = sum_c rs_c cat."""
        S, P, C = self.S, self.P, self.C
        freqs, rates, rs, ps = mv[:4], mv[4:10], mv[10:10 + C], mv[10 + C:10 + 2 * C]
        row = np.zeros(self.row_len)
        # what makes the device's eigensystem or matrices NaN: rejected before numpy's eigh sees it
        if not (np.all(np.isfinite(blens)) and np.all(np.isfinite(mv))) or \
                (self.model != models.JC69 and np.any(freqs < 0)):
            row[0] = -np.inf
            return row
        with np.errstate(all="ignore"):
            pm = transition_matrices(self.model, freqs, rates, blens, rs)
            root = int(self.peel0[-1, 2])
            merged = None if self.rooted else int(self.peel0[-1, 1])
            part = [np.broadcast_to(self._tips[t], (C, P, 4)) for t in range(S)] + [None] * (S - 1)

            def moved(ch):  # P_ch part[ch] as the parent sees it, [C, P, 4]
                return part[ch] if ch == merged else np.einsum("cjk,cpk->cpj", pm[:, ch], part[ch])
            for x, y, v in self.peel0:
                part[v] = moved(x) * moved(y)
            Lc = ps[:, None] * np.einsum("j,cpj->cp", freqs, part[root])
            L = np.zeros(P)
            for c in range(C):
                L = L + Lc[c]
            ll = float(np.dot(self.weights, np.log(L)))
            if not np.isfinite(ll):
                row[0] = -np.inf
                return row
            _, anc, cat, rate = self.split(row)
            cat[:] = Lc / L
            for c in range(C):
                rate += rs[c] * cat[c]
            q = [None] * (2 * S - 1)
            q[root] = np.broadcast_to(freqs, (C, P, 4))
            for x, y, v in self.peel0[::-1]:
                for c in range(C):
                    anc[v - S] += (ps[c] * (part[v][c] * q[v][c])).T
                anc[v - S] /= L
                for u, sib in ((x, y), (y, x)):
                    if u < S:
                        continue
                    r = q[v] * moved(sib)
                    q[u] = r if u == merged else np.einsum("cjk,cpj->cpk", pm[:, u], r)
            row[0] = ll
        return row

    def evaluate_rows(self, blens, model_vecs):
        blens, mv, n = self._inputs(blens, model_vecs)
        return np.stack([self._row(blens[k], mv[k]) for k in range(n)]) if n else np.zeros((0, self.row_len))

    def reset(self):
        self._sum, self._n = np.zeros(self.row_len), 0

    def add(self, blens, model_vecs):
        rows = self.evaluate_rows(blens, model_vecs)
        for r in rows:  # sequential, in draw order
            if np.isfinite(r[0]):
                self._sum += r
                self._n += 1
        return rows[:, 0].copy()

    def read(self):
        return self._sum.copy(), self._n


def seqsum_host(tipcodes, weights, peel0, rooted, model, C, **kw):
    """``SequenceSummaries`` on the host: the same derivation (p o q / L) in
    numpy, the same interface and row conventions."""
    return _SeqsumHost(tipcodes, weights, peel0, rooted, model, C, **kw)


class SeqSummary:
    """The accumulator of a run's summary pass: after ``finish``, ``anc``
    [S-1, 4, P], ``cat`` [C, P], ``rate`` [P], ``subs`` [B] (expected
    substitutions per branch) and ``blens`` [B] are means over the ``count``
    draws with a finite likelihood."""

    def __init__(self, S, P, C, B):
        self.S, self.P, self.C, self.B = S, P, C, B
        self.count = 0
        self.subs, self.blens = np.zeros(B), np.zeros(B)
        self.anc = self.cat = self.rate = None
        self.loglik = float("nan")

    def add_branches(self, loglik, subs, blens):
        """Per-draw branch quantities of one chunk: the draws with a finite
        ``loglik`` are added."""
        ok = np.isfinite(np.asarray(loglik))
        self.subs += np.asarray(subs)[ok].sum(axis=0)
        self.blens += np.asarray(blens)[ok].sum(axis=0)
        self.count += int(ok.sum())

    def finish(self, sums, n_finite):
        """``sums, n_finite``: what the summary context's ``read`` returns."""
        if n_finite != self.count:
            raise ValueError("the summary pass kept %d draws, the branch pass %d" % (n_finite, self.count))
        if n_finite == 0:
            return self
        ll, anc, cat, rate = split_row(np.asarray(sums) / n_finite, self.S, self.P, self.C)
        self.loglik, self.anc, self.cat, self.rate = float(ll), anc, cat, rate
        self.subs, self.blens = self.subs / n_finite, self.blens / n_finite
        return self
