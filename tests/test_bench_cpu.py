"""CPU: bench.py's options that need no GPU -- argument checks, and what --dump-outputs writes (a stub handle stands in for the
device: the writer only reads fields through Device.get)."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def bench(monkeypatch):
    # importing bench.py sets HSA_ENABLE_IPC_MODE_LEGACY when it is unset: keep that out of the rest of the session
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    return bench


class _StubDevice:
    def __init__(self, shape):
        self.shape = shape
        self._host = {}

    def get(self, name):
        rng = np.random.default_rng(sum(map(ord, name)))
        self._host[name] = rng.standard_normal(self.shape)
        return self._host[name]


def test_dump_outputs_whole_fields_on_a_small_grid(bench, tmp_path):
    dev = _StubDevice((19, 36))
    bench.dump_outputs(dev, str(tmp_path), with_ocean=True, with_phys=True)
    names = ["U", "V", "H", "TS", "Q", "CLOUD", "HICE", "ALBEDO", "OLR", "PRECIP", "UO", "VO", "ETA", "SST", "QNET"]
    assert sorted(os.listdir(tmp_path)) == sorted(n + ".npy" for n in names)
    for n in names:
        a = np.load(tmp_path / (n + ".npy"))
        assert a.dtype == np.float64 and a.shape == (19, 36)
        assert np.array_equal(a, _StubDevice((19, 36)).get(n))
    assert dev._host == {}                                           # no host copy left behind to be uploaded again
    bench.dump_outputs(_StubDevice((19, 36)), str(tmp_path / "atm"), with_ocean=False, with_phys=False)
    assert sorted(os.listdir(tmp_path / "atm")) == sorted(n + ".npy" for n in names[:9])


def test_dump_outputs_samples_the_same_cells_within_64_mb(bench, tmp_path):
    shape = (721, 1440)
    bench.dump_outputs(_StubDevice(shape), str(tmp_path / "a"), with_ocean=True, with_phys=True)
    bench.dump_outputs(_StubDevice(shape), str(tmp_path / "b"), with_ocean=True, with_phys=True)
    files = sorted(os.listdir(tmp_path / "a"))
    assert "sample_cells.npy" in files and len(files) == 16
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= 64_000_000
    cells = np.load(tmp_path / "a" / "sample_cells.npy")
    assert cells.dtype == np.float64 and np.all(np.diff(cells) > 0) and cells[-1] < shape[0] * shape[1]
    assert len(cells) > shape[0] * shape[1] // 3
    idx = cells.astype(np.int64)
    for f in files:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float64 and np.array_equal(a, b)       # the same sample from run to run
        if f != "sample_cells.npy":
            assert np.array_equal(a, _StubDevice(shape).get(f[:-4]).reshape(-1)[idx])


@pytest.mark.parametrize("args, msg", [(["--steps", "0"], "--steps must be at least 1"),
                                       (["--gpus", "2", "--dump-outputs", "x"], "--dump-outputs needs the whole globe")])
def test_bench_rejects_bad_arguments_before_any_work(args, msg, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, env=env, capture_output=True, text=True,
                         timeout=120, cwd=str(tmp_path))
    assert out.returncode == 2 and msg in out.stderr, out.stderr
    assert out.stdout == "" and os.listdir(tmp_path) == []
