"""GPU (-m gpu): the procedural planet on the device (qd_topogen.hip) -- the Gaussian filter bit for bit against
topography._smooth (the LDS path and the global-memory path), every golden of the reference's generator within 1e-9 m with
an equal mask, 181 x 360 against the host recipe, determinism, the refusals, the driver's QD_TOPO_DEVICE switch and the CLI."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

import qingdai_amd as qa
import topogen_ref as tr
from qingdai_amd import topogen
from qingdai_amd.device import Device
from qingdai_amd.topogen import TopoGenError
from qingdai_amd.topography import _smooth, create_land_sea_mask, generate_elevation_map, load_topography_from_netcdf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "topogen_*.npz")))
IDS = [os.path.basename(p)[8:-4] for p in GOLDENS]
TOL_FIXTURE = 1e-9          # m, at 13 x 24 .. 37 x 72: a hundred times the reference's own summation-order spread there
TOL_181 = 1e-8              # m, at 181 x 360: fifty times that spread


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


FILTER_CASES = [((13, 24), (4.0, 8.0)),       # both radii (16, 32) larger than their axes
                ((19, 36), (0.5, 0.5)),       # the smallest radius (2)
                ((37, 72), (3.0, 6.0)),
                ((23, 50), (2.0, 5.0)),       # no power of two anywhere
                ((5, 130), (1.0, 10.0)),      # a row spanning three waves
                ((181, 360), (15.0, 30.0))]


@pytest.mark.parametrize("shape,sigma", FILTER_CASES, ids=[f"{s[0]}x{s[1]}" for s, _ in FILTER_CASES])
def test_filter_bitwise(gpu, shape, sigma):
    """lds_bytes=8 leaves room for ONE double: no row and no column fits, so both passes of that call read global memory; the
    default call stages rows and column strips in LDS.  Both must equal the host filter bit for bit."""
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    field = np.random.default_rng(shape[0] * 1000 + shape[1]).standard_normal(shape)
    want = _bits(_smooth(field, *sigma))
    assert np.array_equal(_bits(topogen.smooth(field, sigma[0], sigma[1], dev)), want)
    assert np.array_equal(_bits(topogen.smooth(field, sigma[0], sigma[1], dev, lds_bytes=8)), want)
    dev.close()


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_golden(gpu, path):
    z = np.load(path)
    shape, seed, params, frac = tr.case(z)
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    out = topogen.generate(grid, seed=seed, params=params, target_land_frac=frac, dev=dev)
    dev.close()
    err = float(np.max(np.abs(out["elevation"] - z["elevation"])))
    sea_err = abs(out["sea_level_m"] - float(z["sea_level_m"]))
    print(f"\n{os.path.basename(path)}: max |elevation - reference| {err:.3e} m, |sea level - reference| {sea_err:.3e} m")
    assert out["elevation"].dtype == np.float64 and out["land_mask"].dtype == np.uint8
    assert err <= TOL_FIXTURE and sea_err <= TOL_FIXTURE
    assert np.array_equal(out["land_mask"], z["land_mask"])
    assert np.any(out["elevation"] == out["sea_level_m"])                       # one of the field's own values
    assert np.array_equal(out["land_mask"], (out["elevation"] >= out["sea_level_m"]).astype(np.uint8))
    for k in ("cont_lats", "cont_lons", "cont_amps"):
        assert np.array_equal(_bits(out[k]), _bits(z[k])), k
    if "flat" in os.path.basename(path):
        assert np.all(out["elevation"] == 0.0) and out["sea_level_m"] == 0.0 and np.all(out["land_mask"] == 1)
        assert out["land_frac"] > 0.999


def test_181x360_defaults_against_host(gpu):
    grid = qa.SphericalGrid(181, 360)
    dev = Device(grid)
    out = topogen.generate(grid, dev=dev)
    dev.close()
    host = generate_elevation_map(grid, seed=42)
    err = float(np.max(np.abs(out["elevation"] - host)))
    print(f"\n181x360: max |device - host| {err:.3e} m, sea level {out['sea_level_m']:.6f} m, land_frac {out['land_frac']:.4f}")
    assert err <= TOL_181
    assert np.array_equal(out["land_mask"], create_land_sea_mask(grid))


def test_deterministic(gpu):
    grid = qa.SphericalGrid(37, 72)
    draws = topogen.draw(grid, 5, {"N_CONTINENTS": 4})
    dev = Device(grid)
    a = topogen.generate(grid, seed=5, params={"N_CONTINENTS": 4}, dev=dev, draws=draws)
    b = topogen.generate(grid, seed=5, params={"N_CONTINENTS": 4}, dev=dev, draws=draws)
    dev.close()
    fresh = Device(grid)
    c = topogen.generate(grid, seed=5, params={"N_CONTINENTS": 4}, dev=fresh)
    fresh.close()
    for other in (b, c):
        assert np.array_equal(_bits(a["elevation"]), _bits(other["elevation"]))
        assert np.array_equal(a["land_mask"], other["land_mask"])
        assert _bits(a["sea_level_m"]) == _bits(other["sea_level_m"])


def test_refusals(gpu):
    grid = qa.SphericalGrid(37, 72)
    banded = Device(grid, row0=12, n_rows=12, halo=6)
    with pytest.raises(TopoGenError, match="whole-globe"):
        topogen.generate(grid, dev=banded)
    with pytest.raises(TopoGenError, match="whole-globe"):
        topogen.smooth(np.zeros((37, 72)), 1.0, 1.0, banded)
    banded.close()
    dev = Device(grid)
    with pytest.raises(TopoGenError, match="shape"):                            # another grid's fields on this handle
        topogen.generate(qa.SphericalGrid(19, 36), dev=dev)
    with pytest.raises(TopoGenError, match="shape"):
        topogen.smooth(np.zeros((19, 36)), 1.0, 1.0, dev)
    draws = topogen.draw(grid, 42)
    draws["octave_noise"][2, 5, 7] = np.nan
    with pytest.raises(TopoGenError, match="non-finite noise"):
        topogen.generate(grid, dev=dev, draws=draws)
    with pytest.raises(TopoGenError, match="non-finite"):
        topogen.smooth(np.full((37, 72), np.inf), 1.0, 1.0, dev)
    with pytest.raises(TopoGenError, match="FBM_OCTAVES"):
        topogen.generate(grid, params={"FBM_OCTAVES": topogen.MAX_OCTAVES + 1}, dev=dev)
    with pytest.raises(TopoGenError, match="N_CONTINENTS"):
        topogen.generate(grid, params={"N_CONTINENTS": topogen.MAX_CONTINENTS + 1}, dev=dev)
    with pytest.raises(TopoGenError, match="non-finite parameter"):
        topogen.generate(grid, params={"SCALE_M": float("nan")}, dev=dev)
    z = np.load(os.path.join(HERE, "golden", "topogen_default_37x72.npz"))      # the handle still works
    out = topogen.generate(grid, dev=dev)
    assert np.array_equal(out["land_mask"], z["land_mask"])
    dev.close()


def test_device_caps_are_checked_on_the_device_side_too(gpu):
    """the C entry refuses the counts by itself (a caller that goes round topogen.generate)"""
    import ctypes
    grid = qa.SphericalGrid(13, 24)
    dev = Device(grid)
    a = topogen.build_inputs(grid, None, topogen.draw(grid, 42), 0.29)
    elev, mask, sea = np.empty((13, 24)), np.empty((13, 24), np.uint8), ctypes.c_double(0.0)
    dp = lambda x: x.ctypes.data_as(ctypes.POINTER(ctypes.c_double))

    def call(n_oct, n_cont):
        return dev.lib.qd_topogen_build(dev.h, 13, 24, dp(a["par"]), n_oct, dp(a["oct_amp"]), dp(a["noise"]), n_cont, dp(a["cont"]),
                                        dp(a["cont_coslon"]), dp(a["sin_lat"]), dp(a["cos_lat"]), dp(a["area_w"]),
                                        a["radii"].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), dp(a["weights"]), dp(elev),
                                        mask.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)), ctypes.byref(sea))
    assert call(17, 3) != 0 and b"octave count" in dev.lib.qd_last_error(dev.h)
    assert call(5, 65) != 0 and b"continent count" in dev.lib.qd_last_error(dev.h)
    assert call(5, 3) == 0
    dev.close()


def test_driver_switch(gpu, monkeypatch):
    from qingdai_amd.driver import Simulation
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    got = {}
    for sw in ("0", "1"):
        monkeypatch.setenv("QD_TOPO_DEVICE", sw)
        sim = Simulation(37, 72, use_ocean=True, quiet=True, ecology=False, individuals=False, phyto=False)
        assert sim.elevation is None
        sim.run_steps(2)
        got[sw] = {"land_mask": np.array(sim.land_mask), "base_albedo": np.array(sim.base_albedo), "friction": np.array(sim.friction)}
        got[sw].update({k: np.array(sim.dev.get(k)) for k in ("U", "H", "TS", "SST")})
        sim.dev.close()
    assert np.array_equal(got["0"]["land_mask"], got["1"]["land_mask"])
    for k in ("base_albedo", "friction", "U", "H", "TS", "SST"):
        assert np.array_equal(_bits(got["0"][k]), _bits(got["1"][k])), k
    assert np.ptp(got["1"]["U"]) > 0.0


def test_cli(gpu, tmp_path):
    z = np.load(os.path.join(HERE, "golden", "topogen_cli_19x36.npz"))
    env = {k: v for k, v in os.environ.items() if not k.startswith("QD_")}
    env.update({"QD_N_LAT": "19", "QD_N_LON": "36"})
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "generate_topography.py")], cwd=str(tmp_path), env=env,
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    files = glob.glob(str(tmp_path / "data" / "topography_qingdai_19x36_seed42_*Z.nc"))
    assert len(files) == 1, r.stdout
    lines = r.stdout.split("\n")
    assert lines[0] == "[Topo] Grid 19x36, seed=42, target_land_frac=0.4" and lines[1].startswith("[Topo] Params: {'N_CONTINENTS': 3")
    assert any(ln.startswith("[Topography] Target land fraction=0.400, achieved=") and ln.endswith(f"sea_level={float(z['sea_level_m']):.1f} m")
               for ln in lines), r.stdout
    assert "[Topo] Exporting to NetCDF: " + os.path.join("data", os.path.basename(files[0])) in lines and "[Topo] Done." in lines
    from qingdai_amd.ncio import read_nc
    v, attrs = read_nc(files[0])                                                # the file itself: every column
    assert np.array_equal(v["land_mask"], z["land_mask"]) and abs(float(attrs["sea_level_m"]) - float(z["sea_level_m"])) <= TOL_FIXTURE
    assert np.allclose(v["elevation"], z["elevation"], rtol=0, atol=1e-3)       # f4 of values 1e-9 m apart
    assert np.allclose(v["base_albedo"], z["base_albedo"], rtol=0, atol=1e-6) and np.allclose(v["friction"], z["friction"], rtol=1e-5, atol=0)
    # the loader drops the duplicated 0 / 360 seam column and regrids, as the reference's does: the last column is the first's image
    elev, mask, alb, fric = load_topography_from_netcdf(files[0], qa.SphericalGrid(19, 36), quiet=True)
    assert np.array_equal(mask[:, :-1], z["land_mask"][:, :-1]) and np.array_equal(mask[:, -1], mask[:, 0])
    assert elev is not None and alb.shape == fric.shape == (19, 36)
