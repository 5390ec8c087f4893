"""bench.py's --dump-outputs writer without a GPU: device downloads are stood in for by host arrays, so that the 64 MiB limit and the
seeded sample of a large batch are checked on any machine."""
import os
import types

import numpy as np


def _fake_batch(n, ncat, seed):
    r = np.random.default_rng(seed)
    host = {1: r.integers(0, 600, n, dtype=np.uint32), 2: r.integers(0, 600, n * ncat, dtype=np.uint32),
            3: r.integers(0, 600, n * ncat, dtype=np.uint32), 4: r.random(n * ncat), 5: r.integers(0, 3, n).astype(np.uint8),
            6: r.integers(0, 250, n).astype(np.uint8), 7: r.integers(0, 2, n).astype(np.uint8)}
    api = types.SimpleNamespace(device_download=lambda dev, ptr, nbytes, dt: host[ptr].view(np.uint8)[:nbytes].view(dt).copy())
    res = types.SimpleNamespace(num_hashes=1, counts=2, unique_counts=3, probabilities=4, call=5, confidence=6, flags=7)
    return host, api, res


def _sizes(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_dump_outputs_whole_batch(tmp_path):
    import bench
    n, ncat = 5000, 3
    host, api, res = _fake_batch(n, ncat, 1)
    bench.dump_outputs(str(tmp_path), api, 0, res, n, ncat)
    assert sorted(os.listdir(tmp_path)) == sorted(x + ".npy" for x in ("num_hashes", "counts", "unique_counts", "probabilities", "call",
                                                                       "confidence", "flags"))
    assert np.array_equal(np.load(tmp_path / "counts.npy"), host[2].reshape(n, ncat).astype(np.float32))
    assert np.array_equal(np.load(tmp_path / "probabilities.npy"), host[4].reshape(n, ncat))
    assert np.load(tmp_path / "call.npy").dtype == np.float32 and np.array_equal(np.load(tmp_path / "call.npy"), host[5])


def test_dump_outputs_samples_a_large_batch_the_same_way_every_time(tmp_path):
    import bench
    n, ncat = 1 << 21, 2  # 96 MiB of results
    host, api, res = _fake_batch(n, ncat, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), api, 0, res, n, ncat)
    bench.dump_outputs(str(b), api, 0, res, n, ncat)
    assert _sizes(a) <= 64 << 20
    rows = np.load(a / "read_index.npy")
    assert rows.dtype == np.float64 and len(rows) > n // 2 and (np.diff(rows) > 0).all()
    rows = rows.astype(np.int64)
    assert np.array_equal(np.load(a / "unique_counts.npy"), host[3].reshape(n, ncat)[rows].astype(np.float32))
    assert np.array_equal(np.load(a / "flags.npy"), host[7][rows].astype(np.float32))
    for f in os.listdir(a):
        assert np.array_equal(np.load(a / f), np.load(b / f)), f
