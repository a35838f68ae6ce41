"""Extended-range reference for trees whose per-site likelihood leaves fp64.

``oracle.numpy_pruner.prune`` carries the dtype of its P-matrices through the
whole recurrence.  Fed the fp64 matrices of ``model_matrices`` cast to
``np.longdouble`` (x86 80-bit: a 15-bit exponent, good to 3.4e-4932) it is the
unchanged oracle without rescaling over a range no tree a context can hold
leaves -- an independent reference for the rescaled sweep.  Results are cast
back to float64.
"""
import numpy as np
import pytest

HAS_EXTENDED = np.finfo(np.longdouble).maxexp >= 16384


def require_extended():
    if not HAS_EXTENDED:
        pytest.skip("np.longdouble has no extended exponent range on this platform")


def extended_oracle(case, blens=None):
    """The oracle's dict for ``case`` (at ``blens`` when given), computed in
    np.longdouble and returned in float64."""
    from oracle import numpy_pruner as npr
    blens = case.blens if blens is None else np.asarray(blens, dtype=np.float64)
    P, Q = npr.model_matrices(npr.MODEL_IDS[case.model], case.freqs, case.rates, blens, case.rs)
    out = npr.prune(case.tipcodes, case.weights, case.peel0, case.rooted, P.astype(np.longdouble), case.freqs,
                    case.ps, Q=Q, blens=blens, rs=case.rs)
    return {k: (float(v) if np.ndim(v) == 0 else np.asarray(v, dtype=np.float64)) for k, v in out.items()}
