"""Truths and host doubles of the trait clock rate (``P_b = exp(Q mu t_b)``),
shared by tests/test_geo_clock_cpu.py and tests/test_geo_clock_gpu.py.  numpy
only.

* log L_mix, ``tree_ll`` and the rates / freqs gradients: the existing truths
  (``geo_trees_truth.mix_truth_gradients``, expm(Q t), complex step) at the
  numpy product ``mu * blens``.
* d/dmu: ``Im mix_truth(blens * (mu + 1e-30 i)) / 1e-30``: the complex step on
  mu itself, no branch gradient and no eigenvalue in it.
* the bar of d/dmu: the scalar is a sum over trees and branches of terms of
  either sign and can sit near zero, so it is compared at 1e-9 of max(|truth|,
  size of the terms that cancel in it).  The terms are ``p_t t_tb dlogL_t /
  dt_eff,b``; written in the derivative with respect to the tree's own length
  (``dlogL_t/dt_tb = mu dlogL_t/dt_eff,b``) their size is mu times that.  Of
  the two readings the smaller is taken: ``min(1, mu) sum_t p_t sum_b |t_tb
  dlogL_t/dt_eff,b|``, from ``truth_gradients``' ``blens`` entries at ``mu *
  blens``.
  One floor under it, which binds only where d/dmu is zero to rounding (mu t
  in the thousands: every P is the stationary distribution, truth and terms
  are both ~1e-16 of noise and 1e-9 of them is 1e-25, below what the truth
  itself resolves): Q's zero eigenvalue is known to fp64 no better than K ulp
  of Q's unit scale, and in d/dmu it multiplies the tree's length, so nothing
  computed in fp64, the truth included, is better than ``K 2^-52 sum_t p_t
  length_t``.  At ordinary mu the floor is ~1e-15 beside a bar of ~1e-9.
* ``HostGeoClockLikelihood`` / ``HostGeoTreesClockLikelihood``: the host
  restatements with ``clock=``, what the CPU suite gives ``cli.run`` and the
  posterior classes in place of the device.
"""
import numpy as np

from phylostan_amd import geo
from tests import geo_oracle as go
from tests import geo_trees_truth as gt

STEP = go.STEP
LL_BAR, GRAD_BAR, K2_RATE_BAR = 1e-10, 1e-9, 1e-12


def dmu_truth(tips, peels, blens, rates, freqs, logw, mu, extended=False):
    """d log L_mix / d mu by the complex step on mu."""
    z = np.asarray(blens, float) * complex(mu, STEP)
    return float(gt.mix_truth(tips, peels, z, rates, freqs, logw, extended=extended)[0].imag / STEP)


def cancelling_size(tips, peels, blens, rates, freqs, logw, mu, lls, extended=False, host=False):
    """min(1, mu) sum_t p_t sum_b |t_tb dlogL_t/dt_eff,b|; the branch derivatives
    from ``truth_gradients`` at ``mu * blens`` (``host``: from
    ``geo_gradients_host``, where the complex step on every branch of a large
    sample would take minutes; the size is a scale, not a truth)."""
    blens = np.asarray(blens, float)
    p = gt.tree_weights(lls, logw)
    size = 0.0
    for t in range(len(peels)):
        if p[t] == 0.0:
            continue
        if host:
            g = geo.geo_gradients_host(tips, peels[t], mu * blens[t], rates, freqs)[1]
        else:
            idx, g = go.truth_gradients(tips, peels[t], mu * blens[t], rates, freqs, extended=extended)[1]["blens"]
            assert idx.size == blens.shape[1]
        size += p[t] * np.abs(blens[t] * g).sum()
    return min(1.0, mu) * size


def rounding_floor(blens, logw, lls, K):
    """K 2^-52 sum_t p_t length_t (the module's docstring)."""
    p = gt.tree_weights(lls, logw)
    return K * 2.0 ** -52 * float(p @ np.abs(np.asarray(blens, float)).sum(1))


def dmu_bar(truth, size, floor=0.0):
    return max(GRAD_BAR * max(abs(truth), size), floor)


def check_clock_row(row, tll, tips, peels, blens, params, logw, mu, entries=None, extended=False, seed=0):
    """One draw's clock row ``[log L_mix, d/drates, d/dfreqs, d/dmu]`` and
    ``tree_ll`` against the truth at the project's bars.  Returns the truth's
    log L_t."""
    K = tips.shape[1]
    R = geo.rate_count(K)
    rates, freqs = params[:R], params[R:]
    blens = np.asarray(blens, float)
    tl, tlls, tg = gt.mix_truth_gradients(tips, peels, mu * blens, rates, freqs, logw, extended=extended,
                                          max_entries=entries, seed=seed)
    print("S %d K %d T %d mu %g: log L_mix %.12g truth %.12g rel %.2e"
          % (tips.shape[0], K, len(peels), mu, row[0], tl, abs(row[0] - tl) / abs(tl)))
    assert abs(row[0] - tl) <= LL_BAR * abs(tl)
    assert np.all(np.abs(np.asarray(tll) - tlls) <= LL_BAR * np.abs(tlls))
    for name, got in (("rates", row[1:1 + R]), ("freqs", row[1 + R:1 + R + K])):
        idx, want = tg[name]
        scale = np.abs(got).max()
        err = np.abs(got[idx] - want).max()
        print("  d/d%s: |max| %.3e, vs truth %.2e" % (name, scale, err))
        # a gradient that is zero is compared absolutely, as the K = 2 tests always have: at K = 2 (one rate and a
        # normalised Q: the likelihood does not depend on it), and when the truth says so -- at mu t ~ 3000 every
        # P is the stationary distribution to the last bit and no rate moves the likelihood; 1e-9 of the largest
        # entry would then be 1e-9 of rounding noise
        if name == "rates" and (K == 2 or np.abs(want).max() <= K2_RATE_BAR):
            assert err <= K2_RATE_BAR and np.abs(got).max() <= K2_RATE_BAR
            continue
        assert err <= GRAD_BAR * scale, name
    want = dmu_truth(tips, peels, blens, rates, freqs, logw, mu, extended=extended)
    size = cancelling_size(tips, peels, blens, rates, freqs, logw, mu, tlls, extended=extended)
    bar = dmu_bar(want, size, rounding_floor(blens, logw, tlls, K))
    print("  d/dmu: %.12g truth %.12g, err %.2e, bar %.2e (cancelling terms %.3e)"
          % (row[-1], want, abs(row[-1] - want), bar, size))
    assert abs(row[-1] - want) <= bar
    return tlls


def host_clock_row(tips, peels, blens, params, logw, mu):
    """``(row [2 + R + K], tree_ll [T])`` of ``geo.geo_trees_host(..., clock=mu)``."""
    R = geo.rate_count(tips.shape[1])
    ll, gr, gf, tll, gm = geo.geo_trees_host(tips, peels, blens, params[:R], params[R:], logw, clock=mu)
    return np.concatenate([[ll], gr, gf, [gm]]), tll


# the shapes of the truth tests, shared by the CPU suite (host restatements) and the GPU suite (device)
def truth_cases():
    """name -> (tips, peels, blens, params, logw, mus, extended, entries)."""
    out = {}
    tips, peels, blens, params = gt.make_sample(7, 5, 7, 5100, missing=(0,))  # mixed topologies, tip 0 all ones,
    logw = np.log(np.random.default_rng(57).dirichlet(np.ones(7) * 2.0))      # a zero-length branch in tree 0
    assert np.all(tips[0] == 1.0) and blens[0, 1] == 0.0 and len({p.tobytes() for p in peels}) > 2
    out["mixed"] = (tips, peels, blens, params, logw, (0.2, 25.0), False, None)
    tips, peels, blens, params = gt.make_sample(3, 2, 1, 5200)
    out["k2"] = (tips, peels, blens, params, gt.uniform_logw(1), (0.7,), False, None)
    tips, peels, blens, params = gt.make_sample(7, 5, 3, 5300)
    out["fast"] = (tips, peels, blens, params, np.log([0.2, 0.5, 0.3]), (1e4,), True, None)
    tips, peels, blens, _ = gt.make_sample(7, 4, 3, 5400)
    tie = np.concatenate([np.ones(geo.rate_count(4)), np.full(4, 0.25)])
    out["tie"] = (tips, peels, blens, tie, np.log([0.5, 0.2, 0.3]), (3.0,), False, None)
    tips, peels, blens, _ = gt.make_sample(9, 5, 3, 905)  # test_repeated_eigenvalues' near-tie construction
    rates = np.ones(geo.rate_count(5))
    rates[1] += 1e-11
    out["near"] = (tips, peels, blens, np.concatenate([rates, np.full(5, 0.2)]), np.log([0.5, 0.2, 0.3]), (3.0,),
                   False, 5)
    return out


class HostGeoClockLikelihood(go.HostGeoLikelihood):
    """The single-tree host double with a trait clock and the summaries."""

    def __init__(self, tips, peel0, max_draws=128, device=0):
        super().__init__(tips, peel0, max_draws=max_draws, device=device)
        self.max_draws = max_draws
        self.clock_calls = 0

    def evaluate_rows_clock(self, blens, params, clock):
        blens, params = np.atleast_2d(blens), np.atleast_2d(params)
        clock = np.broadcast_to(np.asarray(clock, float).reshape(-1), (blens.shape[0],))
        self.clock_calls += 1
        rows = np.empty((blens.shape[0], 2 + self.B + self.R + self.K))
        for n in range(blens.shape[0]):
            ll, gb, gr, gf, gm = geo.geo_gradients_host(self.tips, self.peel, blens[n], params[n, :self.R],
                                                        params[n, self.R:], clock=clock[n])
            rows[n] = np.concatenate([[ll], gb, gr, gf, [gm]])
        return rows

    def _summaries(self, blens, params, clock):
        blens, params = np.atleast_2d(blens), np.atleast_2d(params)
        ok = np.isfinite(params).all(axis=1)  # the device's rule: a -inf row and a zero summary
        width = 1 + self.B + self.R + self.K + (clock is not None)
        rows = np.zeros((blens.shape[0], width))
        rows[~ok, 0] = -np.inf
        if ok.any():
            rows[ok] = self.evaluate_rows(blens[ok], params[ok]) if clock is None else \
                self.evaluate_rows_clock(blens[ok], params[ok], np.asarray(clock)[ok])
        each = [geo.geo_summaries_host(self.tips, self.peel, blens[n], params[n, :self.R], params[n, self.R:],
                                       clock=None if clock is None else clock[n]) for n in range(blens.shape[0])]
        return (rows,) + tuple(np.stack([e[k] for e in each]) for k in range(3))

    def evaluate_summaries(self, blens, params):
        return self._summaries(blens, params, None)

    def evaluate_summaries_clock(self, blens, params, clock):
        return self._summaries(blens, params, np.asarray(clock, float).reshape(-1))


class HostGeoTreesClockLikelihood(gt.HostGeoTreesLikelihood):
    """The tree-sample host double with a trait clock."""

    made = []

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.mean_length = geo.mean_tree_length(self.blens, self.log_weights)
        HostGeoTreesClockLikelihood.made.append(self)

    def evaluate_rows_clock(self, params, clock):
        params = np.atleast_2d(params)
        clock = np.broadcast_to(np.asarray(clock, float).reshape(-1), (params.shape[0],))
        rows = np.empty((params.shape[0], 2 + self.R + self.K))
        self.tree_loglik = np.empty((params.shape[0], self.T))
        for n in range(params.shape[0]):
            rows[n], self.tree_loglik[n] = host_clock_row(self.tips, self.peels, self.blens, params[n],
                                                          self.log_weights, clock[n])
        return rows

    def evaluate_summaries_clock(self, params, clock):
        params = np.atleast_2d(params)
        clock = np.broadcast_to(np.asarray(clock, float).reshape(-1), (params.shape[0],))
        rows = self.evaluate_rows_clock(params, clock)
        jumps = np.empty((params.shape[0], self.K, self.K))
        root = np.empty((params.shape[0], self.K))
        for n in range(params.shape[0]):
            jumps[n], root[n] = geo.geo_trees_summaries_host(self.tips, self.peels, self.blens, params[n, :self.R],
                                                             params[n, self.R:], self.log_weights, clock=clock[n])
        return rows, jumps, root
