"""Many tree topologies on one alignment (include/phylo_hip_forest.h).

``ForestLikelihood`` binds the forest context: the alignment once, T peels,
and calls whose rows each name their tree.  ``forest_host`` is a stand-in with
the same interface built on any single-tree evaluator (tests pass the CPU
oracle in; product code never imports ``oracle/``).  ``lockstep_advi`` runs T
independent mean-field optimisations of ``advi.ADVI.run``'s algorithm with one
likelihood call per phase for all topologies still running.
"""
import ctypes

import numpy as np

from . import _lib, models


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p)


class ForestLikelihood:
    """T trees (``peels`` [T, S-1, 3], 0-based, tip ids in ``tipcodes``' row
    order) on one alignment.  ``evaluate_rows(tree_of_row, blens, model_vecs)``
    returns the compact rows [n, 1 + B + 2C + 14] of ``phy_eval`` -- each row
    evaluated on its own tree, bitwise independent of the rest of the call."""

    def __init__(self, tipcodes, weights, peels, rooted, model, C, max_rows=None, device=0):
        self.lib = _lib.load()
        tipcodes = np.ascontiguousarray(tipcodes, dtype=np.uint8)
        self.S, self.P = tipcodes.shape
        self.C = int(C)
        self.rooted = bool(rooted)
        self.model = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
        w = np.ascontiguousarray(weights, dtype=np.float64)
        peels = np.ascontiguousarray(peels, dtype=np.int32)
        if w.shape != (self.P,):
            raise ValueError("weights must have shape (P,)")
        if peels.ndim != 3 or peels.shape[1:] != (self.S - 1, 3):
            raise ValueError("peels must have shape (T, S-1, 3)")
        self.T = peels.shape[0]
        self.max_rows = int(max_rows) if max_rows is not None else max(self.T, 1)
        ctx = ctypes.c_void_p()
        _lib.check(self.lib.phy_forest_create(self.S, self.P, self.C, int(self.rooted), self.model, _ptr(tipcodes),
                                              _ptr(w), self.T, _ptr(peels), self.max_rows, int(device),
                                              ctypes.byref(ctx)), "phy_forest_create")
        self.ctx = ctx
        self.B = self.lib.phy_forest_num_branches(ctx)
        self.outlen = self.lib.phy_forest_output_len(ctx)
        self.model_len = 10 + 2 * self.C

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.phy_forest_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def info(self):
        vals = [ctypes.c_int() for _ in range(8)]
        _lib.check(self.lib.phy_forest_info(self.ctx, *[ctypes.byref(v) for v in vals]), "phy_forest_info")
        return dict(zip(("cols", "cap_m", "max_chunks", "min_chunks", "max_depth", "min_depth", "deep_in_lds",
                         "lds_bytes"), [v.value for v in vals]))

    def evaluate_rows(self, tree_of_row, blens, model_vecs, site_ll=False):
        """Rows [n, outlen] (and [n, P] site log-likelihoods with
        ``site_ll``).  Calls above ``max_rows`` are chunked: a row's bits do
        not depend on the chunking."""
        tree = np.ascontiguousarray(tree_of_row, dtype=np.int32).reshape(-1)
        blens = np.ascontiguousarray(np.atleast_2d(blens), dtype=np.float64)
        mv = np.ascontiguousarray(np.atleast_2d(model_vecs), dtype=np.float64)
        n = tree.shape[0]
        if blens.shape != (n, self.B) or mv.shape != (n, self.model_len):
            raise ValueError("bad shapes: tree_of_row %s blens %s model %s" % (tree.shape, blens.shape, mv.shape))
        out = np.empty((n, self.outlen))
        sl = np.empty((n, self.P)) if site_ll else None
        for lo in range(0, n, self.max_rows):
            hi = min(n, lo + self.max_rows)
            _lib.check(self.lib.phy_forest_eval(self.ctx, hi - lo, _ptr(tree[lo:hi]), _ptr(blens[lo:hi]),
                                                _ptr(mv[lo:hi]), _ptr(out[lo:hi]),
                                                _ptr(sl[lo:hi]) if site_ll else None), "phy_forest_eval")
        return (out, sl) if site_ll else out


def plan_forest(tipcodes, peels, rooted, C, max_rows, model="JC69", cu_count=0):
    """The plan ``ForestLikelihood`` would take (no device, no context;
    ``phy_forest_plan``): the common facts and every tree's chunk count and
    deep stack."""
    lib = _lib.load()
    tipcodes = np.ascontiguousarray(tipcodes, dtype=np.uint8)
    S, P = tipcodes.shape
    peels = np.ascontiguousarray(peels, dtype=np.int32)
    T = peels.shape[0]
    w = np.ones(P)
    facts, chunks, depths = np.zeros(12, np.int32), np.zeros(max(T, 1), np.int32), np.zeros(max(T, 1), np.int32)
    kind = models.MODEL_IDS[model] if isinstance(model, str) else int(model)
    _lib.check(lib.phy_forest_plan(S, P, int(C), int(bool(rooted)), kind, _ptr(tipcodes), _ptr(w), T, _ptr(peels),
                                   int(max_rows), int(cu_count), _ptr(facts), _ptr(chunks), _ptr(depths)),
               "phy_forest_plan")
    out = dict(zip(("cols", "cap_m", "max_chunks", "min_chunks", "max_depth", "min_depth", "deep_in_lds", "lds_bytes",
                    "latency", "fin", "qf", "fin_qf"), [int(v) for v in facts]))
    out.update(chunks=[int(v) for v in chunks[:T]], depths=[int(v) for v in depths[:T]])
    return out


class _ForestHost:
    def __init__(self, evaluators, B, C, P):
        self.evaluators, self.T = list(evaluators), len(evaluators)
        self.B, self.C, self.P = B, C, P
        self.outlen = 1 + B + 2 * C + 14
        self.model_len = 10 + 2 * C
        self.max_rows = 1 << 30

    def info(self):
        return {}

    def close(self):
        pass

    def evaluate_rows(self, tree_of_row, blens, model_vecs, site_ll=False):
        tree = np.asarray(tree_of_row, dtype=np.int64).reshape(-1)
        blens = np.atleast_2d(np.asarray(blens, dtype=np.float64))
        mv = np.atleast_2d(np.asarray(model_vecs, dtype=np.float64))
        n = tree.shape[0]
        if blens.shape != (n, self.B) or mv.shape != (n, self.model_len):
            raise ValueError("bad shapes: tree_of_row %s blens %s model %s" % (tree.shape, blens.shape, mv.shape))
        if n and (tree.min() < 0 or tree.max() >= self.T):
            raise ValueError("tree_of_row entry outside 0..%d" % (self.T - 1))
        out = np.empty((n, self.outlen))
        sl = np.empty((n, self.P)) if site_ll else None
        for r in range(n):  # one row at a time: a row's bits are its own
            row, s = self.evaluators[tree[r]](blens[r], mv[r], site_ll)
            row = np.asarray(row, dtype=np.float64)[:self.outlen].copy()
            if not np.isfinite(row[0]):
                row[0], row[1:] = -np.inf, 0.0
            out[r] = row
            if site_ll:
                sl[r] = s
        return (out, sl) if site_ll else out


def forest_host(evaluators, B, C, P):
    """A forest on the host: ``evaluators[t](blens, model_vec, site_ll)``
    returns tree t's output row (at least the compact part, in
    include/phylo_hip.h's layout) and its site log-likelihoods or None.  Same
    interface and row conventions as ``ForestLikelihood``."""
    return _ForestHost(evaluators, B, C, P)


class TaggedLikelihood:
    """A forest behind ``Posterior``'s likelihood interface:
    ``evaluate_rows(blens, model_vecs, tags)`` with the row's tree as its tag
    (``Posterior.log_prob_grad(..., tags=)``)."""

    def __init__(self, forest):
        self.forest = forest

    def evaluate_rows(self, blens, model_vecs, tags=None):
        if tags is None:
            raise ValueError("a forest likelihood needs the tree of every row (tags)")
        return self.forest.evaluate_rows(tags, blens, model_vecs)


class _Lane:
    """One topology's view of the shared posterior: ``ADVI`` calls
    ``log_prob`` / ``log_prob_grad`` on it, and every call is answered by the
    hub's next batched evaluation."""

    def __init__(self, hub, tag, post):
        self._hub, self._tag, self._post = hub, tag, post
        self.dim = post.dim

    def __getattr__(self, name):  # everything else is the posterior's own
        return getattr(self._post, name)

    def log_prob_grad(self, U, propto=True, need_grad=True):
        return self._hub.ask(self, np.atleast_2d(np.asarray(U, np.float64)), bool(propto), bool(need_grad))

    def log_prob(self, U, propto=True):
        return self.log_prob_grad(U, propto=propto, need_grad=False)[0]


class _Hub:
    """Rendezvous of the lanes: a lane that asks blocks; once every live lane
    has asked (or ended), the requests of a kind go to the posterior as ONE
    call, rows tagged with their lane's tree, and every lane gets its rows."""

    def __init__(self, post):
        import threading
        self.post = post
        self.cv = threading.Condition()
        self.live = 0
        self.asked = {}    # lane -> (U, propto, need_grad)
        self.answer = {}   # lane -> (lp, G) or an exception
        self.calls = 0     # batched posterior calls made

    def ask(self, lane, U, propto, need_grad):
        with self.cv:
            self.asked[lane] = (U, propto, need_grad)
            self.cv.notify_all()
            while lane not in self.answer:
                self.cv.wait()
            res = self.answer.pop(lane)
        if isinstance(res, BaseException):
            raise res
        return res

    def ended(self):
        with self.cv:
            self.live -= 1
            self.cv.notify_all()

    def serve(self):
        """Until every lane has ended: wait for all live lanes to ask, answer them."""
        while True:
            with self.cv:
                while self.live > 0 and len(self.asked) < self.live:
                    self.cv.wait()
                if self.live == 0:
                    return
                asked, self.asked = self.asked, {}
            groups = {}
            for lane, (U, propto, need_grad) in asked.items():
                groups.setdefault((propto, need_grad), []).append((lane, U))
            out = {}
            for (propto, need_grad), members in sorted(groups.items(), key=lambda kv: kv[0]):
                members.sort(key=lambda m: m[0]._tag)
                U = np.concatenate([u for _, u in members])
                tags = np.concatenate([np.full(u.shape[0], lane._tag, np.int32) for lane, u in members])
                try:
                    lp, G = self.post.log_prob_grad(U, propto=propto, need_grad=need_grad, tags=tags)
                    self.calls += 1
                    lo = 0
                    for lane, u in members:
                        hi = lo + u.shape[0]
                        out[lane] = (lp[lo:hi].copy(), G[lo:hi].copy() if G is not None else None)
                        lo = hi
                except Exception as e:  # noqa: BLE001  the lanes of the call see it
                    for lane, _ in members:
                        out[lane] = e
            with self.cv:
                self.answer.update(out)
                self.cv.notify_all()


class LockstepResult:
    """One topology's outcome: ``q`` (MeanField), ``eta``, ``iterations``,
    ``trace`` [(iter, seconds, elbo)], ``draws`` [samples, dim] unconstrained
    output draws, ``converged`` (stopped before ``max_iterations``), and
    ``error`` (the ``ADVIError`` message that ended it, else None)."""

    def __init__(self, tag):
        self.tag, self.q, self.eta, self.iterations, self.trace = tag, None, None, 0, []
        self.draws, self.error, self.converged, self.q0 = None, None, False, None


def lockstep_advi(post, tags, seed, grad_samples=1, elbo_samples=100, eval_elbo=100, eta=None, tol_rel_obj=0.01,
                  max_iterations=10000, samples=0, log=None, diag=None, ids=None):
    """Mean-field ADVI on every topology of ``tags`` (their trees in the
    forest, which are also their generators' second seed word), in lockstep.

    Topology t is exactly ``cli.run``'s solo sequence on a single-tree
    likelihood of tree t with ``np.random.default_rng((seed, t))`` as its one generator:
    ``Posterior.initialize``, ``ADVI.run`` (eta adaptation unless ``eta`` is
    given, stochastic gradient ascent) and ``samples`` output draws -- the
    same code, run as one lane per topology, with the lanes' likelihood
    requests of a phase answered by one ``post.log_prob_grad(..., tags=)``
    call for all topologies still running.  A lane consumes its own generator
    in ``ADVI``'s order and sees only its own rows, so with a deterministic,
    row-independent likelihood its result does not depend on which other
    topologies run, and equals the solo run bit for bit.  An ``ADVIError`` (or
    a failed initialisation) ends that topology alone.  ``diag(t)`` gives the
    per-evaluation callback of topology t.  ``ids[t]`` replaces t as the
    generator's second seed word (a topology's index in its file when the
    forest holds a selection).  Returns {t: LockstepResult}."""
    import threading
    from .advi import ADVI, ADVIError
    hub = _Hub(post)
    results = {int(t): LockstepResult(int(t)) for t in tags}
    quiet = lambda *_: None  # noqa: E731

    def lane_main(t):
        res = results[t]
        try:
            lane = _Lane(hub, t, post)
            rng = np.random.default_rng((seed, int(ids[t]) if ids is not None else t))
            adv = ADVI(lane, rng, grad_samples=grad_samples, elbo_samples=elbo_samples, eval_elbo=eval_elbo,
                       log=(lambda msg, t=t: log("[tree %d] %s" % (t, msg))) if log else quiet)
            res.q0 = type(post).initialize(lane, rng)
            cb = diag(t) if diag else None

            def on_elbo(it, sec, elbo):
                res.trace.append((it, sec, elbo))
                if cb:
                    cb(it, sec, elbo)
            res.q, res.eta, res.iterations = adv.run(res.q0, eta=eta, adapt_engaged=eta is None,
                                                     tol_rel_obj=tol_rel_obj, max_iterations=max_iterations,
                                                     diag=on_elbo, family="meanfield")
            res.converged = res.iterations < max_iterations
            res.draws = res.q.sample(rng, samples) if samples > 0 else np.zeros((0, post.dim))
        except (ADVIError, RuntimeError) as e:
            res.error = str(e)
        finally:
            hub.ended()

    hub.live = len(results)
    threads = [threading.Thread(target=lane_main, args=(t,), daemon=True) for t in results]
    for th in threads:
        th.start()
    hub.serve()
    for th in threads:
        th.join()
    return results
