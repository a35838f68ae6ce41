"""Records the truth rows that are too slow to recompute in a test
(``python -m tests.kseq_record_truth``): the 400-tip caterpillar's log L and
d/dblens from the extended-range complex-step truth, to
``tests/golden/kseq/<case>.npz``.  ``kseq_truth.load_truth`` reads them."""
import os

import numpy as np

from tests import kseq_truth as kt


def main():
    os.makedirs(kt.GOLDEN, exist_ok=True)
    case = kt.caterpillar400()
    ref = case.truth_row(only=("blens",))
    np.savez_compressed(kt.golden_path(case.name), **ref)
    print(case.name, ref["loglik"], kt.golden_path(case.name))


if __name__ == "__main__":
    main()
