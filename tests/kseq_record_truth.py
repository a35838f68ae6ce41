"""Records the truth rows the tests read (``python -m tests.kseq_record_truth
[name ...]``, every case without names): the 400-tip caterpillar's log L and
d/dblens from the extended-range complex-step truth, and every array of
``kseq_truth.edge_cases()`` (the 300-tip +I caterpillar among them takes ten
minutes), to ``tests/golden/kseq/<case>.npz``.  ``kseq_truth.load_truth`` reads
them."""
import os
import sys

import numpy as np

from tests import kseq_truth as kt


def main(names):
    os.makedirs(kt.GOLDEN, exist_ok=True)
    todo = [(kt.caterpillar400(), ("blens",))] + [(c, None) for c in kt.edge_cases()]
    for case, only in todo:
        if names and case.name not in names:
            continue
        ref = case.truth_row(only=only)
        np.savez_compressed(kt.golden_path(case.name), **ref)
        print(case.name, ref["loglik"], kt.golden_path(case.name), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
