"""Partitioned alignments (include/phylo_hip_part.h): K disjoint site sets of
one alignment on one tree, each with its own model vector and relative rate,

    log L(t, mu, theta) = sum_k log L_k(mu_k t; theta_k).

``read_partitions`` / ``split_alignment`` turn a RAxML / IQ-TREE style
partition file into per-partition patterns.  ``PartitionedLikelihood`` binds
the device context; ``partition_host`` is a stand-in with the same interface
over K single-alignment evaluators (tests pass the CPU oracle in; product
code never imports ``oracle/``).  ``partition_combine_host`` restates the
device's fold of a draw's K rows operation for operation, so the two agree bit
for bit.
"""
import ctypes
import re

import numpy as np

from . import _lib, models
from .data import _compress

PLAN_FACTS = ("cols", "latency", "blocks", "P", "Ppad", "R", "extra_lo", "extra_hi", "cap_m", "chunks", "deep_in_lds",
              "deep_all_in_lds", "lds_bytes", "fin", "qf", "fin_qf")
ALIGN = 128  # a partition's first column of the padded alignment is a multiple of it


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


# ---------------------------------------------------------------- the scheme
class Partition:
    """One line of a partition file: ``name`` and the 0-based ``sites`` (sorted)."""

    def __init__(self, name, sites):
        self.name, self.sites = name, np.asarray(sites, dtype=np.int64)

    def __repr__(self):
        return "Partition(%r, %d sites)" % (self.name, self.sites.size)


_RANGE = re.compile(r"^(\d+)(?:\s*-\s*(\d+))?(?:\s*\\\s*(\d+))?$")


def read_partitions(path, n_sites):
    """RAxML / IQ-TREE style lines, ``DNA, name = 1-658\\3, 2-658\\3``: 1-based
    inclusive ranges with an optional ``\\stride``, comma separated (the data
    type before the first comma is optional and ignored).  Every site of the
    alignment must be in exactly one partition: a site in two, a site in
    none, or a site past the alignment is a ``ValueError`` naming the
    partition and the (1-based) site."""
    parts = []
    with open(path) as fp:
        for lineno, line in enumerate(fp, 1):
            line = line.split("#", 1)[0].strip()
            if not line:
                continue
            if "=" not in line:
                raise ValueError("%s:%d: expected 'name = ranges'" % (path, lineno))
            head, ranges = line.split("=", 1)
            name = head.split(",")[-1].strip()
            if not name:
                raise ValueError("%s:%d: partition without a name" % (path, lineno))
            sites = []
            for item in ranges.split(","):
                m = _RANGE.match(item.strip())
                if not m:
                    raise ValueError("%s:%d: partition %s: bad range %r" % (path, lineno, name, item.strip()))
                lo = int(m.group(1))
                hi = int(m.group(2)) if m.group(2) else lo
                stride = int(m.group(3)) if m.group(3) else 1
                if lo < 1 or hi < lo or stride < 1:
                    raise ValueError("%s:%d: partition %s: bad range %r" % (path, lineno, name, item.strip()))
                last = lo + (hi - lo) // stride * stride  # the last site the range lists
                if last > n_sites:
                    first = lo if lo > n_sites else lo + -(-(n_sites + 1 - lo) // stride) * stride
                    raise ValueError("partition %s: site %d is past the alignment's %d sites" % (name, first, n_sites))
                sites.extend(range(lo - 1, hi, stride))
            parts.append(Partition(name, sorted(sites)))
    if not parts:
        raise ValueError("%s: no partitions" % path)
    owner = np.full(n_sites, -1, np.int64)
    for k, p in enumerate(parts):
        dup = np.flatnonzero(np.diff(p.sites) == 0)
        if dup.size:
            raise ValueError("partition %s: site %d is listed twice" % (p.name, p.sites[dup[0]] + 1))
        taken = np.flatnonzero(owner[p.sites] >= 0)
        if taken.size:
            s = p.sites[taken[0]]
            raise ValueError("partition %s: site %d is already in partition %s" % (p.name, s + 1, parts[owner[s]].name))
        owner[p.sites] = k
    free = np.flatnonzero(owner < 0)
    if free.size:
        s = int(free[0])
        near = parts[int(owner[s - 1])].name if s > 0 and owner[s - 1] >= 0 else parts[0].name
        raise ValueError("site %d is in no partition (after partition %s)" % (s + 1, near))
    return parts


def split_alignment(chars, parts):
    """Per partition ``(tipcodes [S, P_k], weights [P_k], site_pattern
    [sites_k])`` of the ``uint8 [S, sites]`` char array: the partition's
    columns compressed on their own, as ``data.compress_patterns`` would."""
    out = []
    for p in parts:
        tip, w, _, sp = _compress(chars[:, p.sites])
        out.append((tip, w, sp))
    return out


# ------------------------------------------------------------------ the fold
def partition_combine_host(part_rows, t, mu):
    """The draw's output row from its K partition rows ``part_rows [K, 1 + B
    + tail]`` (``[log L][g_b][tail]``, g with respect to the scaled lengths),
    the shared lengths ``t [B]`` and the rates ``mu [K]``, in the device's
    order (part_combine_kernel): every product rounded once, no fused
    multiply-add,

        log L   = ((L_0 + L_1) + L_2) + ...
        d/dt_b  = ((mu_0 g_0b + mu_1 g_1b) + mu_2 g_2b) + ...   left to right over k
        d/dmu_k = ((t_0 g_k0 + t_1 g_k1) + t_2 g_k2) + ...      left to right over b

    then per partition ``[d/dmu_k][tail_k]``.  A partition whose log L is not
    finite makes the row ``-inf`` followed by zeros."""
    rows = np.asarray(part_rows, dtype=np.float64)
    t = np.asarray(t, dtype=np.float64)
    mu = np.asarray(mu, dtype=np.float64)
    K, B = rows.shape[0], t.shape[0]
    tail = rows.shape[1] - 1 - B
    out = np.zeros(1 + B + K * (1 + tail))
    if not np.all(np.isfinite(rows[:, 0])):
        out[0] = -np.inf
        return out
    g = rows[:, 1:1 + B]
    ll = rows[0, 0]
    dt = mu[0] * g[0]
    for k in range(1, K):
        ll = ll + rows[k, 0]
        dt = dt + mu[k] * g[k]
    tg = t[None, :] * g  # [K, B] rounded products
    dmu = tg[:, 0].copy()
    for b in range(1, B):
        dmu = dmu + tg[:, b]
    out[0] = ll
    out[1:1 + B] = dt
    blocks = out[1 + B:].reshape(K, 1 + tail)
    blocks[:, 0] = dmu
    blocks[:, 1:] = rows[:, 1 + B:]
    return out


class _Base:
    """Shapes and the argument checks both forms share."""

    def _shapes(self, blens, mu, model_vecs):
        blens = np.ascontiguousarray(np.atleast_2d(blens), dtype=np.float64)
        n = blens.shape[0]
        mu = np.ascontiguousarray(np.asarray(mu, dtype=np.float64).reshape(n, -1))
        mv = np.ascontiguousarray(np.asarray(model_vecs, dtype=np.float64).reshape(n, -1, self.model_len))
        if blens.shape != (n, self.B) or mu.shape != (n, self.K) or mv.shape != (n, self.K, self.model_len):
            raise ValueError("bad shapes: blens %s mu %s model %s" % (blens.shape, mu.shape, mv.shape))
        return n, blens, mu, mv

    @staticmethod
    def _result(out, rows, sl, part_rows, site_ll):
        if part_rows and site_ll:
            return out, rows, sl
        if part_rows:
            return out, rows
        if site_ll:
            return out, sl
        return out


class PartitionedLikelihood(_Base):
    """K partitions ``parts = [(tipcodes [S, P_k], weights [P_k]), ...]`` on
    one tree (``peel0`` [S-1, 3], 0-based).  ``evaluate_rows(blens, mu,
    model_vecs)`` returns the draws' rows ``[n, 1 + B + K (1 + 2C + 14)]``:
    ``[log L][d/dt B]`` then per partition ``[d/dmu_k][drs, dps, dfreqs
    (root), the six exchangeabilities, dfreqs (total)]``."""

    def __init__(self, parts, peel0, rooted, model, C, max_draws=1, device=0):
        self.lib = _lib.load()
        tips = [np.ascontiguousarray(p[0], dtype=np.uint8) for p in parts]
        ws = [np.ascontiguousarray(p[1], dtype=np.float64) for p in parts]
        self.K = len(tips)
        if self.K < 1:
            raise ValueError("need at least one partition")
        self.S = tips[0].shape[0]
        for k, (tp, w) in enumerate(zip(tips, ws)):
            if tp.ndim != 2 or tp.shape[0] != self.S or w.shape != (tp.shape[1],):
                raise ValueError("partition %d: tipcodes must be [S, P_k] and weights [P_k]" % k)
        self.Pk = np.array([tp.shape[1] for tp in tips], dtype=np.int32)
        self.off = np.concatenate([[0], np.cumsum(self.Pk)]).astype(np.int64)
        self.Psum = int(self.off[-1])
        self.C, self.rooted = int(C), bool(rooted)
        self.model = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
        tip = np.ascontiguousarray(np.concatenate(tips, axis=1)) if self.Psum else np.zeros((self.S, 1), np.uint8)
        w = np.ascontiguousarray(np.concatenate(ws)) if self.Psum else np.zeros(1)
        peel = np.ascontiguousarray(peel0, dtype=np.int32)
        self.max_draws = int(max_draws)
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_part_create(self.S, self.K, _ptr(self.Pk), self.C, int(self.rooted), self.model,
                                            _ptr(tip), _ptr(w), _ptr(peel), self.max_draws, int(device),
                                            ctypes.byref(ctx)), "phy_part_create")
        self.ctx = ctx
        self.B = self.lib.phy_part_num_branches(ctx)
        self.rowlen = self.lib.phy_part_row_len(ctx)
        self.outlen = self.lib.phy_part_output_len(ctx)
        self.model_len = 10 + 2 * self.C
        self._plan_args = (tips, peel)

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.phy_part_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        """The context's plan (``phy_part_info``): ``PLAN_FACTS`` and ``blocks [K, 2]``."""
        facts, blocks = np.zeros(len(PLAN_FACTS), np.int32), np.zeros((self.K, 2), np.int32)
        _lib.check(self.lib.phy_part_info(self.ctx, _ptr(facts), _ptr(blocks)), "phy_part_info")
        out = dict(zip(PLAN_FACTS, [int(v) for v in facts]))
        out["blocks"] = [[int(a), int(b)] for a, b in blocks]
        return out

    def evaluate_rows(self, blens, mu, model_vecs, part_rows=False, site_ll=False):
        """Rows [n, outlen]; with ``part_rows`` also the partitions' compact
        rows [n, K, rowlen] the fold consumed, with ``site_ll`` the site
        log-likelihoods [n, sum P_k] in the partitions' pattern order.  Calls
        above ``max_draws`` are chunked: a row's bits do not depend on it."""
        n, blens, mu, mv = self._shapes(blens, mu, model_vecs)
        out = np.empty((n, self.outlen))
        rows = np.empty((n, self.K, self.rowlen)) if part_rows else None
        sl = np.empty((n, self.Psum)) if site_ll else None
        for lo in range(0, n, self.max_draws):
            hi = min(n, lo + self.max_draws)
            _lib.check(self.lib.phy_part_eval(self.ctx, hi - lo, _ptr(blens[lo:hi]), _ptr(mu[lo:hi]), _ptr(mv[lo:hi]),
                                              _ptr(out[lo:hi]), _ptr(rows[lo:hi]) if part_rows else None,
                                              _ptr(sl[lo:hi]) if site_ll else None), "phy_part_eval")
        return self._result(out, rows, sl, part_rows, site_ll)


def plan_partitions(tipcodes_k, peel0, rooted, C, max_draws, model="JC69", cu_count=0):
    """The plan ``PartitionedLikelihood`` would take (no device, no context;
    ``phy_part_plan``): the common facts (``PLAN_FACTS``), every partition's
    block range ``blocks [K, 2]`` and the padded columns' ``col_part`` /
    ``col_pat`` maps."""
    lib = _lib.load()
    tips = [np.ascontiguousarray(t, dtype=np.uint8) for t in tipcodes_k]
    K = len(tips)
    Pk = np.array([t.shape[1] for t in tips], dtype=np.int32)
    S = tips[0].shape[0] if K else 0
    psum = int(Pk.sum()) if K else 0
    tip = np.ascontiguousarray(np.concatenate(tips, axis=1)) if psum else np.zeros((max(S, 1), 1), np.uint8)
    w = np.ones(max(psum, 1))
    peel = np.ascontiguousarray(peel0, dtype=np.int32)
    ptot = 0
    for p in Pk:
        ptot = (ptot + ALIGN - 1) // ALIGN * ALIGN + max(int(p), 0)
    facts = np.zeros(len(PLAN_FACTS), np.int32)
    blocks = np.zeros((max(K, 1), 2), np.int32)
    col_part, col_pat = np.zeros(max(ptot, 1), np.int32), np.zeros(max(ptot, 1), np.int32)
    kind = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
    _lib.check(lib.phy_part_plan(S, K, _ptr(Pk) if K else None, int(C), int(bool(rooted)), kind, _ptr(tip), _ptr(w),
                                 _ptr(peel), int(max_draws), int(cu_count), _ptr(facts), _ptr(blocks), _ptr(col_part),
                                 _ptr(col_pat)), "phy_part_plan")
    out = dict(zip(PLAN_FACTS, [int(v) for v in facts]))
    out.update(blocks=[[int(a), int(b)] for a, b in blocks[:K]], col_part=col_part[:ptot].copy(),
               col_pat=col_pat[:ptot].copy())
    return out


# ----------------------------------------------------------------- the host
class _PartitionHost(_Base):
    def __init__(self, evaluators, B, C, Pk):
        self.evaluators, self.K = list(evaluators), len(evaluators)
        self.B, self.C = B, C
        self.Pk = np.asarray(Pk, dtype=np.int64)
        self.off = np.concatenate([[0], np.cumsum(self.Pk)]).astype(np.int64)
        self.Psum = int(self.off[-1])
        self.rowlen = 1 + B + 2 * C + 14
        self.outlen = 1 + B + self.K * (1 + 2 * C + 14)
        self.model_len = 10 + 2 * C
        self.max_draws = 1 << 30

    def close(self):
        pass

    def evaluate_rows(self, blens, mu, model_vecs, part_rows=False, site_ll=False):
        n, blens, mu, mv = self._shapes(blens, mu, model_vecs)
        out = np.empty((n, self.outlen))
        rows = np.empty((n, self.K, self.rowlen))
        sl = np.empty((n, self.Psum)) if site_ll else None
        for d in range(n):  # one draw at a time: a row's bits are its own
            for k in range(self.K):
                row, s = self.evaluators[k](mu[d, k] * blens[d], mv[d, k], site_ll)
                row = np.asarray(row, dtype=np.float64)[:self.rowlen].copy()
                if not np.isfinite(row[0]):
                    row[0], row[1:] = -np.inf, 0.0
                rows[d, k] = row
                if site_ll:
                    sl[d, self.off[k]:self.off[k + 1]] = s
            out[d] = partition_combine_host(rows[d], blens[d], mu[d])
        return self._result(out, rows if part_rows else None, sl, part_rows, site_ll)


def partition_host(evaluators, B, C, Pk):
    """Partitions on the host: ``evaluators[k](scaled_blens, model_vec,
    site_ll)`` returns partition k's output row (at least the compact part,
    in include/phylo_hip.h's layout) and its site log-likelihoods or None.
    Same interface and row conventions as ``PartitionedLikelihood``; the fold
    is ``partition_combine_host``."""
    return _PartitionHost(evaluators, B, C, Pk)


# ------------------------------------------------------------- the posterior
from .posterior import Posterior  # noqa: E402  (after the likelihoods: posterior.py does not import this module)

_SUBST_NAMES = ("wshape", "pinv", "ps", "rate_unscaled", "kappa", "rates", "freqs")


class PartitionedPosterior(Posterior):
    """``Posterior`` over K partitions of one alignment: the tree, clock,
    coalescent and speciation parts are ``Posterior``'s own; the site-rate and
    substitution parameters are declared once per partition with the suffix
    ``_p{k}`` (1-based), each with the prior the single model gives it.  For
    K > 1 a ``relrates`` Simplex(K) with a flat prior gives the relative rates
    mu_k = relrates_k N / N_k (N_k sites in partition k, N their sum): the
    site-weighted mean of mu is 1, so an estimated clock rate or free branch
    lengths stay identified.  K = 1 has no ``relrates`` and its density is the
    plain ``Posterior``'s.

    ``likelihood.evaluate_rows(blens [n, B], mu [n, K], model_vecs [n, K, 10 +
    2C])`` returns the rows of ``PartitionedLikelihood`` / ``partition_host``.
    The native strict-clock fast path (hostlib) is not used."""

    def __init__(self, spec, tree, likelihood, n_sites):
        self.n_sites = np.asarray(n_sites, dtype=np.float64).reshape(-1)
        self.K = int(self.n_sites.size)
        if self.K < 1 or np.any(self.n_sites < 1):
            raise ValueError("every partition needs at least one site")
        self._mu_scale = self.n_sites.sum() / self.n_sites  # N / N_k
        super().__init__(spec, tree, likelihood, compact_rows=False)

    def _native_strict(self):
        return None

    # ------------------------------------------------------------------ layout
    @staticmethod
    def suffix(k):
        return "_p%d" % (k + 1)

    def _declare(self):
        P = self._declare_tree()
        for k in range(self.K):
            P += self._declare_site(self.suffix(k)) + self._declare_subst(self.suffix(k))
        if self.K > 1:
            from .transforms import Simplex
            from .posterior import _Param
            P.append(_Param("relrates", Simplex(self.K)))
        return P

    def _dropped_constants(self):
        import math
        one = Posterior._dropped_constants(self)  # the tree's constants and ONE partition's
        sp = self.spec
        sub = 0.0
        if sp.model in ("GTR", "HKY"):
            sub += math.lgamma(4.0)
        if sp.model == "GTR":
            sub += math.lgamma(6.0)
        if sp.model == "HKY":
            sub += -math.log(1.25) - 0.5 * math.log(2.0 * math.pi)
        if self.K == 1:
            return one
        return one + (self.K - 1) * sub + math.lgamma(float(self.K))  # relrates ~ dirichlet(1, ..., 1)

    def _view(self, d, k):
        """Partition k's entries of a by-name dict under their plain names (the arrays themselves)."""
        sfx = self.suffix(k)
        return {name: d[name + sfx] for name in _SUBST_NAMES if name + sfx in d}

    def relative_rates(self, vals, n):
        """mu [n, K]."""
        if self.K == 1:
            return np.ones((n, 1))
        return vals["relrates"] * self._mu_scale[None, :]

    # ------------------------------------------------------------ the pieces
    def _row_width(self):
        return 1 + self.B + self.K * (1 + 2 * self.C + 14)

    def _subst_forward(self, vals, n):
        mvs, subs = [self.relative_rates(vals, n)], []
        positive = np.ones(n, bool)
        for k in range(self.K):
            mv, pos, sub = Posterior._subst_forward(self, self._view(vals, k), n)
            mvs.append(mv)
            subs.append(sub)
            positive &= pos
        return np.concatenate(mvs, axis=1), positive, subs

    def _lik_rows(self, blens, mv, tags=None):
        if tags is not None:
            raise ValueError("tags: a partitioned likelihood has one tree")
        n, K = blens.shape[0], self.K
        return self.lik.evaluate_rows(blens, mv[:, :K], mv[:, K:].reshape(n, K, 10 + 2 * self.C))

    def _subst_prior(self, vals, lp, gx):
        for k in range(self.K):
            lp = Posterior._subst_prior(self, self._view(vals, k), lp, self._view(gx, k))
        return lp  # relrates: flat

    def _subst_backward(self, vals, rows, bad, gx, sub):
        B, blk = self.B, 1 + 2 * self.C + 14
        for k in range(self.K):
            o = 1 + B + k * blk
            # the partition's compact row: [log L, d/dt] of the draw, then the partition's own tail
            rk = np.concatenate([rows[:, :1 + B], rows[:, o + 1:o + blk]], axis=1)
            Posterior._subst_backward(self, self._view(vals, k), rk, bad, self._view(gx, k), sub[k])
            if self.K > 1:
                gx["relrates"][:, k] += rows[:, o] * self._mu_scale[k]

    # ------------------------------------------------------------------ output
    def model_vectors(self, U):
        """[n, K, 10 + 2C]"""
        U = np.atleast_2d(np.asarray(U, np.float64))
        n = U.shape[0]
        vals, _, _ = self.constrain(U)
        return self._subst_forward(vals, n)[0][:, self.K:].reshape(n, self.K, 10 + 2 * self.C)

    def transformed(self, U):
        """The columns of a sample file: the tree's parameters and transformed
        parameters as ``Posterior`` lists them, then every partition's block
        (its parameters, then its site rates), then ``mu``."""
        U = np.atleast_2d(np.asarray(U, np.float64))
        n = U.shape[0]
        vals, _, _ = self.constrain(U)
        sp = self.spec
        block = {p.name for k in range(self.K) for p in self._declare_site(self.suffix(k)) + self._declare_subst(self.suffix(k))}
        out = [(p.name, vals[p.name]) for p in self.params if p.name not in block and p.name != "relrates"]
        if self.clock:
            from . import clocks
            out.append(("heights", self._heights(vals, n)))
            if sp.relaxed and sp.clock in clocks.MRF:
                out.append(("substrates", self._substrates(vals)))
        for k in range(self.K):
            sfx = self.suffix(k)
            vk = self._view(vals, k)
            out += [(p.name, vals[p.name]) for p in self._declare_site(sfx) + self._declare_subst(sfx)]
            rs, ps = self._site_rates(vk, n)
            if sp.categories > 1 and sp.heterogeneity == "weibull":
                out += [("ps" + sfx, ps), ("rs" + sfx, rs)]
            elif sp.categories > 1:
                cons = vk["ps"] * vk["rate_unscaled"]
                out += [("rs" + sfx, rs), ("constraint" + sfx, cons / cons.sum(axis=1, keepdims=True))]
            elif sp.invariant:
                out += [("ps" + sfx, ps), ("rs" + sfx, rs)]
        if self.K > 1:
            out.append(("mu", self.relative_rates(vals, n)))
        return out
