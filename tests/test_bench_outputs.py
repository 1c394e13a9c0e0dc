"""bench.py --dump-outputs: the arrays a run writes (CPU; the GPU run itself is exercised by the benchmark)."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_dump_writes_float32_or_float64(bench, tmp_path):
    bench.dump_outputs(str(tmp_path / "out"), {"errors": np.array([1.5, 2.25]), "palette": np.arange(6, dtype=np.uint8).reshape(2, 3),
                                               "best_k": np.array([7], np.int32)})
    e = np.load(tmp_path / "out" / "errors.npy")
    p = np.load(tmp_path / "out" / "palette.npy")
    k = np.load(tmp_path / "out" / "best_k.npy")
    assert e.dtype == np.float64 and e.tolist() == [1.5, 2.25]
    assert p.dtype == np.float32 and p.shape == (2, 3) and p.ravel().tolist() == list(range(6))
    assert k.dtype == np.float32 and k.tolist() == [7.0]


def test_dump_refuses_more_than_its_budget(bench, tmp_path):
    too_big = np.zeros(bench.DUMP_MAX_BYTES // 8 + 1, np.float64)
    with pytest.raises(SystemExit):
        bench.dump_outputs(str(tmp_path / "out"), {"errors": too_big})
    assert not (tmp_path / "out").exists()


def test_dump_sample_is_fixed_and_sorted(bench):
    assert bench.dump_sample(5, 64).tolist() == list(range(5))
    a, b = bench.dump_sample(1000, 64), bench.dump_sample(1000, 64)
    assert a.tolist() == b.tolist() and len(set(a.tolist())) == 64
    assert np.all(np.diff(a) > 0) and a[0] >= 0 and a[-1] < 1000
