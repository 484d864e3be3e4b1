"""bench.py --dump-outputs: the writer is device-agnostic, so its contract
(exact float encodings, fixed seeded sample of large outputs, identical
files from run to run) is checked here on CPU tensors."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import bench  # noqa: E402


def test_small_outputs_are_written_whole_and_exact(tmp_path):
    rng = np.random.default_rng(7)
    parity = rng.integers(0, 256, (3, 2, 160), np.uint8)
    crcs = np.array([0, 1, 0x7FFFFFFF, 0x80000000, 0xFFFFFFFF, 0xE8B7BE43],
                    np.uint32)
    bench.dump_outputs(str(tmp_path), {
        "parity": torch.from_numpy(parity),
        "crc32": torch.from_numpy(crcs.view(np.int32)),
    })
    got_p = np.load(tmp_path / "parity.npy")
    got_c = np.load(tmp_path / "crc32.npy")
    assert got_p.dtype == np.float32 and got_c.dtype == np.float64
    assert np.array_equal(got_p, parity.reshape(-1).astype(np.float32))
    assert np.array_equal(got_c.astype(np.uint32), crcs)


def test_large_output_sample_is_fixed_and_bounded(tmp_path):
    n = 4 * bench.DUMP_MAX_ELEMS + 3 * bench.DUMP_CHUNK + 5
    a = torch.arange(n, dtype=torch.int64).remainder(251).to(torch.uint8)
    bench.dump_outputs(str(tmp_path / "a"), {"out": a})
    bench.dump_outputs(str(tmp_path / "b"), {"out": a})
    s1 = np.load(tmp_path / "a" / "out.npy")
    s2 = np.load(tmp_path / "b" / "out.npy")
    assert s1.dtype == np.float32 and s1.size == bench.DUMP_MAX_ELEMS
    assert np.array_equal(s1, s2)
    # every sampled run is DUMP_CHUNK consecutive elements of the source
    runs = s1.reshape(-1, bench.DUMP_CHUNK)
    step = (runs[:, 1:] - runs[:, :-1]) % 251
    assert np.all(step == 1)
    # a changed source byte inside a sampled run changes the dump
    rng = np.random.default_rng(bench.DUMP_SEED)
    starts = np.sort(rng.choice(n // bench.DUMP_CHUNK,
                                bench.DUMP_MAX_ELEMS // bench.DUMP_CHUNK,
                                replace=False)) * bench.DUMP_CHUNK
    b = a.clone()
    b[int(starts[17]) + 3] ^= 0x40
    bench.dump_outputs(str(tmp_path / "c"), {"out": b})
    s3 = np.load(tmp_path / "c" / "out.npy")
    assert np.count_nonzero(s1 != s3) == 1
