"""bench.py --dump-outputs: which rows of the chain state are written, and the 64 MB bound (CPU only)."""
import os

import numpy as np

import bench


def _state(N, B, seed=0):
    rng = np.random.default_rng(seed)
    return rng.random((N, N)) < 0.3, rng.standard_normal((N, N, B)), rng.standard_normal(N)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_dump_writes_the_whole_state_when_it_fits(tmp_path):
    A, W, b = _state(16, 3)
    assert bench.dump_outputs(str(tmp_path), A, W, b) == ["adjacency", "biases", "weights"]
    got = _load(str(tmp_path))
    assert got["adjacency"].dtype == np.float32 and np.array_equal(got["adjacency"], A.astype(np.float32))
    assert got["weights"].dtype == np.float64 and np.array_equal(got["weights"], W)
    assert got["biases"].dtype == np.float64 and np.array_equal(got["biases"], b)


def test_dump_of_a_large_state_is_a_fixed_sample_of_rows(tmp_path):
    N, B = 64, 8
    A, W, b = _state(N, B)
    per_row = N * 4 + N * B * 8 + 8
    cap = 10 * per_row + per_row // 2
    got = []
    for k in range(2):
        d = str(tmp_path / str(k))
        assert bench.dump_outputs(d, A, W, b, max_bytes=cap) == ["adjacency", "biases", "rows", "weights"]
        g = _load(d)
        rows = g["rows"].astype(np.int64)
        assert g["rows"].dtype == np.float64 and rows.size == 10 and np.all(np.diff(rows) > 0) and rows.max() < N
        assert np.array_equal(g["weights"], W[rows]) and np.array_equal(g["adjacency"], A[rows]) and np.array_equal(g["biases"], b[rows])
        assert sum(v.nbytes for v in g.values() if v is not g["rows"]) <= cap
        got.append(rows)
    assert np.array_equal(got[0], got[1])
    # a shard that fits is written whole, without a row index
    d = str(tmp_path / "shard")
    assert bench.dump_outputs(d, A, W, b, rows=np.arange(8, 16), max_bytes=cap) == ["adjacency", "biases", "weights"]
    assert np.array_equal(_load(d)["weights"], W[8:16])

