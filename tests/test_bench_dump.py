"""CPU: bench.py --dump-outputs writes float64 .npy files under its size
limit, the whole buffer when it fits and otherwise a sample of the draws that
is the same from run to run; --steps is checked.  (CPU tensors stand in for
the device buffer: dump_outputs only indexes and copies it.)"""
import os
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_small_buffer_is_dumped_whole(tmp_path):
    import bench
    out = torch.arange(7 * 5, dtype=torch.float64).reshape(7, 5)
    bench.dump_outputs(str(tmp_path / "d"), out, 0)
    got = _load(str(tmp_path / "d"))
    assert sorted(got) == ["loglik", "row_index", "rows"]
    assert all(v.dtype == np.float64 for v in got.values())
    np.testing.assert_array_equal(got["rows"], out.numpy())
    np.testing.assert_array_equal(got["row_index"], np.arange(7.0))
    np.testing.assert_array_equal(got["loglik"], out.numpy()[:, 0])


def test_large_buffer_is_sampled_the_same_way_every_run(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 8 * 5 * 3)  # room for three rows of five doubles
    out = torch.arange(11 * 5, dtype=torch.float64).reshape(11, 5)
    bench.dump_outputs(str(tmp_path / "a"), out, 0)
    bench.dump_outputs(str(tmp_path / "b"), out, 0)
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    idx = a["row_index"].astype(int)
    assert len(idx) == 3 and len(set(idx)) == 3 and np.all(np.diff(idx) > 0) and idx[0] >= 0 and idx[-1] < 11
    np.testing.assert_array_equal(a["rows"], out.numpy()[idx])
    assert a["loglik"].shape == (11,)
    for k in a:
        np.testing.assert_array_equal(a[k], b[k])
    # another rank's files do not overwrite rank 0's
    bench.dump_outputs(str(tmp_path / "a"), out, 1)
    assert "rows_rank1" in _load(str(tmp_path / "a"))


def test_the_real_limit_keeps_a_dump_under_64_mb():
    import bench
    for outlen in (1, 23, 8863, 70000):
        keep = max(1, bench.DUMP_MAX_BYTES // (8 * outlen))
        draws = 8192
        total = 8 * outlen * min(keep, draws) + 8 * min(keep, draws) + 8 * draws  # rows + row_index + loglik
        assert total <= 64 * 10**6


def test_steps_must_be_positive():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "0"], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr
