"""Records the mixture truth that is too slow to recompute in a test
(``python -m tests.kseq_mix_record_truth``): the shifted caterpillar's log L,
site log L, class log-likelihoods and d/dblens, d/drs, d/dps from the
extended-range complex-step truth, and every array of
``kseq_mix_truth.edge_cases()``, to ``tests/golden/kseq/<case>.npz``.
``kseq_mix_truth.load_truth`` reads it."""
import os

import numpy as np

from tests import kseq_mix_truth as mt


def main():
    os.makedirs(mt.GOLDEN, exist_ok=True)
    case = mt.shifted_caterpillar()
    sh = mt.shift_counts(case)
    assert np.any(sh[0] != sh[1]), "the two components' root shifts must differ"
    ref = case.truth_row(only=("blens", "rs", "ps"))
    np.savez_compressed(mt.golden_path(case.name), **ref)
    print(case.name, ref["loglik"], "shifts", sh.tolist(), mt.golden_path(case.name))
    for case in mt.edge_cases():
        ref = case.truth_row()
        np.savez_compressed(mt.golden_path(case.name), **ref)
        print(case.name, ref["loglik"], mt.golden_path(case.name))


if __name__ == "__main__":
    main()
