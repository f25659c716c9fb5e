"""The daily phytoplankton step (P017) without a GPU: the NumPy restatement against the reference's goldens, the host tables, the
firing clock, the C-ABI parameter block and data/plankton.nc."""
import ctypes
import glob
import os

import numpy as np
import pytest

import phyto_daily_ref as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDENS = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "phyto_daily_*.npz")))


def _rel(a, b):
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def _env(monkeypatch, z):
    for k in [k for k in os.environ if k.startswith(("QD_PHYTO_", "QD_ECO_", "QD_STAR_"))]:
        monkeypatch.delenv(k)
    for k, v in zip(z["env_keys"], z["env_vals"]):
        monkeypatch.setenv(str(k), str(v))


def test_goldens_present():
    assert len(GOLDENS) >= 5


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[12:-4])
def test_restatement_matches_reference_goldens(path):
    z = np.load(path)
    tab = ref.tables_from_golden(z)
    C, N = z["C0"], z["N0"]
    from qingdai_amd import SphericalGrid
    g = SphericalGrid(int(z["n_lat"]), int(z["n_lon"]))
    lat, lon = g.lat, g.lon
    n = int(z["n_days"])
    for d in range(n):
        a, b = ref.insolation(z["stars"][d], lat, lon)
        assert np.array_equal(a, z["insA"][d]) and np.array_equal(b, z["insB"][d])
        r = ref.step_daily(C, N, a, b, z["T_w"][d], tab, z["land_mask"])
        C, N = r["C"], r["N"]
        assert np.allclose(r["means"], z["means"][d], rtol=1e-13, atol=0)
        line = z["lines"][d]
        assert f"{r['means'][0]:.3f}" in line and f"{r['means'][2]:.3f}" in line
        for tag, day in (("first", 0), ("last", n - 1)):
            if d == day:
                for k, key in (("C", "C"), ("N", "N"), ("alpha_bands", "alpha_bands"), ("alpha_scalar", "alpha_scalar"),
                               ("kd490", "kd490")):
                    assert _rel(r[k], z[f"{tag}_{key}"]) < 1e-13, (tag, k)
    land = z["land_mask"] == 1
    assert np.all(C[:, land] == 0.0) and np.all(N[land] == 0.0)


@pytest.mark.parametrize("path", GOLDENS, ids=lambda p: os.path.basename(p)[12:-4])
def test_host_tables_match_reference(path, monkeypatch):
    from qingdai_amd.phyto import daily_tables, daily_device_tables
    z = np.load(path)
    _env(monkeypatch, z)
    S = z["tab_shape_sb"].shape[0]
    t = ref.tables_from_host(daily_tables(S, H_mld_m=float(z["H_arg"])))
    g = ref.tables_from_golden(z)
    for k, v in g.items():
        if k in ("specA", "specB", "T_ray"):
            assert np.allclose(t[k], v, rtol=1e-14, atol=0), k
        else:
            assert np.array_equal(np.asarray(t[k]), np.asarray(v)), k
    band, species, shape = daily_device_tables(daily_tables(S, H_mld_m=float(z["H_arg"])))
    NB = len(g["Kd0_b"])
    assert band.shape == (8, NB) and species.shape == (6, S) and shape.shape == (S, NB)


def test_firing_schedule():
    from qingdai_amd.phyto import daily_schedule
    day = 2 * np.pi / 8.726646259971648e-5
    assert day == 72000.0
    fire, nxt = daily_schedule(0.0, 0.0, 300.0, 500, day)
    assert list(np.nonzero(fire)[0]) == [0, 240, 480] and nxt == 480 * 300.0 + day
    # any split of the span gives the same firing steps
    for cuts in ([1, 239, 1, 259], [7, 200, 33, 100, 160], [240, 240, 20], [1] * 500):
        clock, t, got = 0.0, 0.0, []
        for n in cuts:
            f, clock = daily_schedule(clock, t, 300.0, n, day)
            got += list(f)
            t = float((t + 300.0 * np.arange(n))[-1] + 300.0)
        assert list(np.nonzero(got)[0]) == [0, 240, 480]
    # a restart at t0 != 0: the clock starts at 0 again, so the first step fires
    t0 = 1234567.0
    fire, _ = daily_schedule(0.0, t0, 300.0, 500, day)
    assert list(np.nonzero(fire)[0]) == [0, 240, 480]


def test_params_struct_matches_header():
    from qingdai_amd import _lib
    # field names, types and offsets against the compiler's: tests/test_abi_cpu.py, for every struct
    assert ctypes.sizeof(_lib.qd_phyto_daily_params) == 6 * 4 + 10 * 8
    assert "qd_phyto_daily" in _lib.SYMBOLS and _lib.FIELDS[-2:] == ["PHYTO_N", "KD490"]


class _FakeDev:
    """Stands in for the device in the plankton.nc round trip: fields and the band stack in host memory."""

    def __init__(self, shape, nb):
        self.f = {k: np.zeros(shape) for k in ("WATER_ALPHA", "KD490", "PHYTO_N")}
        self.bands = np.zeros((nb,) + shape)

    def get(self, name):
        return self.f[name]

    def upload_now(self, name, arr):
        self.f[name] = np.array(arr, dtype=np.float64)

    def phyto_daily_bands(self, nb):
        return self.bands.copy()


def test_plankton_nc_round_trip_keeps_N(tmp_path, monkeypatch):
    from qingdai_amd import SphericalGrid, ncio
    from qingdai_amd.phyto import PhytoDaily, PhytoTracers
    for k in [k for k in os.environ if k.startswith(("QD_PHYTO_", "QD_ECO_"))]:
        monkeypatch.delenv(k)
    monkeypatch.setenv("QD_PHYTO_NSPECIES", "3")
    g = SphericalGrid(9, 18)
    mask = np.zeros((9, 18), dtype=np.uint8)
    mask[3:5, 4:9] = 1
    tr = PhytoTracers(g, mask)
    pd = PhytoDaily(tr, H_mld_m=40.0, diag=False)
    pd.dev = _FakeDev((9, 18), pd.NB)
    r = np.random.default_rng(1)
    pd.dev.f["WATER_ALPHA"] = r.uniform(0.05, 0.1, (9, 18))
    pd.dev.f["KD490"] = r.uniform(0.04, 0.2, (9, 18))
    pd.dev.f["PHYTO_N"] = r.uniform(0.0, 2.0, (9, 18))
    pd.dev.bands = r.uniform(0.05, 0.1, (pd.NB, 9, 18))
    pd.n_steps = 1
    tr.C_phyto_s = r.uniform(0.0, 0.05, (3, 9, 18))
    path = str(tmp_path / "plankton.nc")
    assert pd.save_distribution_nc(path, day_value=2.0)
    v, attrs = ncio.read_nc(path)
    assert set(v) == {"lat", "lon", "C_phyto_s", "alpha_water_bands", "alpha_water_scalar", "Kd_490", "N", "bands_lambda_centers"}
    assert int(attrs["NB"]) == pd.NB and int(attrs["S"]) == 3 and float(attrs["H_mld_m"]) == 40.0 and float(attrs["day"]) == 2.0
    assert v["alpha_water_bands"].shape == (pd.NB, 9, 18) and v["N"].dtype == np.float32
    # load into a fresh state: C, alpha and Kd come back (f4), N does not
    tr2 = PhytoTracers(g, mask)
    pd2 = PhytoDaily(tr2, H_mld_m=40.0, diag=False)
    pd2.dev = _FakeDev((9, 18), pd2.NB)
    N_before = pd2.dev.f["PHYTO_N"].copy()
    assert pd2.load_distribution_nc(path)
    assert np.allclose(tr2.C_phyto_s, tr.C_phyto_s, rtol=1e-6)
    assert np.allclose(pd2.dev.f["WATER_ALPHA"], pd.dev.f["WATER_ALPHA"], rtol=1e-6)
    assert np.allclose(pd2.dev.f["KD490"], pd.dev.f["KD490"], rtol=1e-6)
    assert np.array_equal(pd2.dev.f["PHYTO_N"], N_before)
    # before any daily step the file has no band stack (phyto.py:768-770)
    pd.n_steps = 0
    assert pd.save_distribution_nc(path)
    v, _ = ncio.read_nc(path)
    assert "alpha_water_bands" not in v and "N" in v
