"""GPU (-m gpu): bench.py as a program on a small grid.  A plain run prints the headline line only and times exactly --steps steps;
--dump-outputs writes what the last timed step left on the device (checked against the same loop run in this process); --full adds
the supplementary figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from util import relerr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NLAT, NLON, K, W, DT = 91, 180, 3, 2, 300.0


def _bench(*args):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--nlat", str(NLAT), "--nlon", str(NLON),
                          "--steps", str(K), "--warmup", str(W)] + list(args), env=env, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_dumps_the_last_step(gpu, tmp_path, monkeypatch):
    r = _bench("--dump-outputs", str(tmp_path / "out"))
    assert (r["steps"], r["warmup"], r["n_gpus"], r["dtype"], r["unit"], r["higher_is_better"]) == (K, W, 1, "f64", "planet-days/s", True)
    assert r["metric"] == f"simulated planet-days/sec at {NLAT}x{NLON} f64"
    assert r["ms_per_step"] > 0 and r["value"] == pytest.approx(DT / 72000.0 / (r["ms_per_step"] / 1e3), rel=1e-9)
    for k in ("roofline", "roofline_ocean_substep", "cpu_baseline", "gpu_over_cpu", "ecology_config5"):
        assert k not in r, k
    names = ["U", "V", "H", "TS", "Q", "CLOUD", "HICE", "ALBEDO", "OLR", "PRECIP", "UO", "VO", "ETA", "SST", "QNET"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(n + ".npy" for n in names)

    # the same loop in this process: warm-up span, then the timed span
    monkeypatch.setenv("HSA_ENABLE_IPC_MODE_LEGACY", os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    import bench
    _, m, _, forcing, _, _, _ = bench.build_case(NLAT, NLON, True)
    dev = m._dev
    dev.step_n(forcing.star_table([i * DT for i in range(W)]), DT, with_ocean=True, with_physics=True, pass_albedo=True)
    dev.step_n(forcing.star_table([(W + i) * DT for i in range(K)]), DT, with_ocean=True, with_physics=True, pass_albedo=True)
    try:
        for n in names:
            got = np.load(tmp_path / "out" / (n + ".npy"))
            assert got.dtype == np.float64 and got.shape == (NLAT, NLON), n
            want = dev.get(n)
            assert np.array_equal(np.isnan(got), np.isnan(want)), n
            ok = ~np.isnan(want)
            assert relerr(got[ok], want[ok]) < 1e-12, n
    finally:
        dev.close()


def test_full_run_adds_the_supplementary_figures(gpu):
    r = _bench("--full", "--cpu-budget", "0.5")
    assert (r["steps"], r["warmup"]) == (K, W) and r["ms_per_step"] > 0
    assert r["roofline"]["kernel"] == "k_dyn_hyper" and r["roofline"]["launches"] > 0 and r["roofline"]["avg_kernel_ms"] > 0
    assert r["roofline_ocean_substep"]["launches"] > 0
    assert r["cpu_baseline"]["value"] > 0 and r["gpu_over_cpu"] > 0
    assert "error" not in r["ecology_config5"] and r["ecology_config5"]["ms_per_step"] > 0
