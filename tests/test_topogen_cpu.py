"""CPU: the procedural planet's host side (qingdai_amd/topogen.py) without a GPU -- the random draws against the reference's
goldens, the goldens' margin conditions, the inputs of the device build through a NumPy restatement (tests/topogen_ref.py), the
CLI's environment parsing, base properties, the NetCDF writer and loader, the driver switch and the C-ABI declarations."""
import glob
import os

import numpy as np
import pytest

import qingdai_amd as qa
import topogen_ref as tr
from qingdai_amd import topogen
from qingdai_amd.topography import _smooth, load_topography_from_netcdf

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "topogen_*.npz")))
IDS = [os.path.basename(p)[8:-4] for p in GOLDENS]
CLI_PARAMS = {"N_CONTINENTS": 3, "CONTINENT_SIGMA_DEG": 30.0, "CONTINENT_SHAPE_P": 2.0, "CONT_MIN_DIST_DEG": 40.0, "W_VLF": 0.35,
              "FBM_OCTAVES": 5, "HURST_H": 0.8, "W1": 1.0, "W3": 0.6, "SCALE_M": 4500.0}


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def test_goldens_cover_the_cases():
    assert len(GOLDENS) == 15 and all(os.path.getsize(p) < 64 * 1024 for p in GOLDENS)
    for shape in ("13x24", "19x36", "37x72"):
        for case in ("default", "cli", "wide", "crowded"):
            assert f"{case}_{shape}" in IDS
    assert {"flat_19x36", "nocont_19x36", "nooct_19x36"} <= set(IDS)
    z = np.load(os.path.join(HERE, "golden", "topogen_cli_19x36.npz"))
    assert tr.case(z) == ((19, 36), 42, CLI_PARAMS, 0.40)


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_draw_reproduces_reference_centres(path):
    z = np.load(path)
    shape, seed, params, _ = tr.case(z)
    d = topogen.draw(qa.SphericalGrid(*shape), seed, params)
    for k in ("cont_lats", "cont_lons", "cont_amps"):
        assert d[k].shape == z[k].shape and np.array_equal(_bits(d[k]), _bits(z[k])), k
    assert d["vlf_noise"].shape == shape and d["octave_noise"].shape == (int(params.get("FBM_OCTAVES", 5)),) + shape


def test_crowded_exhausts_the_spacing_loop():
    """12 centres 90 degrees apart do not exist: the rejection loop gives up and the rest is drawn unspaced"""
    z = np.load(os.path.join(HERE, "golden", "topogen_crowded_19x36.npz"))
    lat, lon = np.deg2rad(z["cont_lats"]), np.deg2rad(z["cont_lons"])
    cosd = np.sin(lat)[:, None] * np.sin(lat)[None, :] + np.cos(lat)[:, None] * np.cos(lat)[None, :] * np.cos(lon[:, None] - lon[None, :])
    d = np.rad2deg(np.arccos(np.clip(cosd, -1.0, 1.0))) + 360.0 * np.eye(12)
    assert d.min() < 90.0


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_golden_margins(path):
    """conditions on the inputs: every cell at least 1e-3 m from sea level, the quantile decision at least 1e-9 from the next"""
    z = np.load(path)
    if "flat" in os.path.basename(path):
        assert np.all(z["elevation"] == 0.0) and float(z["sea_level_m"]) == 0.0 and np.all(z["land_mask"] == 1)
        return
    assert float(z["elev_gap"]) >= 1e-3 and float(z["cw_above"]) >= 1e-9 and float(z["cw_below"]) >= 1e-9
    assert np.isfinite(z["elevation"]).all()


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_build_inputs_restated_reproduce_golden(path):
    """the tables, weights, amplitudes and the fixed-point select handed to the device give the reference's planet when NumPy
    evaluates the same stages"""
    z = np.load(path)
    shape, seed, params, frac = tr.case(z)
    grid = qa.SphericalGrid(*shape)
    a = topogen.build_inputs(grid, params, topogen.draw(grid, seed, params), frac)
    elev, sea, mask = tr.build(a, shape)
    assert np.max(np.abs(elev - z["elevation"])) <= 1e-9 and abs(sea - float(z["sea_level_m"])) <= 1e-9
    assert np.array_equal(mask, z["land_mask"])


def test_half_filter_restatement_is_the_host_filter():
    f = np.random.default_rng(3).standard_normal((13, 24))
    wa, wo = topogen._half_kernel(4.0), topogen._half_kernel(8.0)
    assert (wa[1], wo[1]) == (16, 32)
    got = tr._half_filter(tr._half_filter(f, wa[0], 0, "nearest"), wo[0], 1, "wrap")
    assert np.array_equal(_bits(got), _bits(_smooth(f, 4.0, 8.0)))


def test_params_from_env():
    assert topogen.params_from_env({}) == (42, 0.40, CLI_PARAMS)
    env = {"QD_SEED": "7", "QD_TARGET_LAND_FRAC": "0.55", "QD_N_CONTINENTS": "6", "QD_CONT_SIGMA_DEG": "18", "QD_CONT_SHAPE_P": "1.5",
           "QD_CONT_MIN_DIST_DEG": "55", "QD_W_VLF": "0.5", "QD_FBM_OCTAVES": "3", "QD_HURST_H": "0.6", "QD_W1": "0.8", "QD_W3": "0.9",
           "QD_SCALE_M": "3000"}
    z = np.load(os.path.join(HERE, "golden", "topogen_wide_19x36.npz"))
    seed, frac, params = topogen.params_from_env(env)
    assert (seed, frac, params) == (7, 0.55, tr.case(z)[2])
    assert isinstance(params["N_CONTINENTS"], int) and isinstance(params["FBM_OCTAVES"], int) and isinstance(params["W1"], float)
    bad = {"QD_SEED": "x", "QD_TARGET_LAND_FRAC": "", "QD_N_CONTINENTS": "2.5", "QD_W1": "one", "QD_SCALE_M": "1e3"}
    seed, frac, params = topogen.params_from_env(bad)
    assert (seed, frac, params["N_CONTINENTS"], params["W1"], params["SCALE_M"]) == (42, 0.40, 3, 1.0, 1000.0)


def test_unknown_parameter_and_counts_are_refused():
    grid = qa.SphericalGrid(13, 24)
    with pytest.raises(topogen.TopoGenError, match="unknown"):
        topogen.draw(grid, 42, {"N_CONTINENT": 4})
    d = topogen.draw(grid, 42)
    with pytest.raises(topogen.TopoGenError, match="FBM_OCTAVES"):
        topogen.build_inputs(grid, {"FBM_OCTAVES": 17}, d, 0.29)
    with pytest.raises(topogen.TopoGenError, match="noise shapes"):
        topogen.build_inputs(qa.SphericalGrid(19, 36), None, d, 0.29)


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_base_properties_match_reference(path):
    z = np.load(path)
    grid = qa.SphericalGrid(*tr.case(z)[0])
    alb, fric = topogen.base_properties(z["land_mask"], z["elevation"], grid)
    assert np.array_equal(_bits(alb), _bits(z["base_albedo"])) and np.array_equal(_bits(fric), _bits(z["friction"]))


def test_base_properties_without_elevation_are_the_drivers():
    from qingdai_amd.topography import generate_base_properties
    z = np.load(os.path.join(HERE, "golden", "topogen_default_19x36.npz"))
    a, f = topogen.base_properties(z["land_mask"])
    a0, f0 = generate_base_properties(z["land_mask"])
    assert np.array_equal(a, a0) and np.array_equal(f, f0)


def test_writer_round_trips_through_the_loader(tmp_path):
    """The file holds the fixture's fields at f4, every column.  load_topography_from_netcdf, like the reference's loader, drops
    the duplicated 0 / 360 seam column of the model grid and regrids (tests/test_driver_io_cpu.py): nodes coincide to the f4
    rounding of the stored axes, and the last column comes back as the cyclic image of the first."""
    from qingdai_amd.ncio import read_nc
    z = np.load(os.path.join(HERE, "golden", "topogen_cli_37x72.npz"))
    grid = qa.SphericalGrid(37, 72)
    path = str(tmp_path / "sub" / "topo.nc")
    topogen.write_topography(path, grid, z["elevation"], z["land_mask"], z["base_albedo"], z["friction"], float(z["sea_level_m"]))
    f4 = lambda a: np.asarray(a).astype(np.float32)
    v, attrs = read_nc(path)
    assert v["elevation"].dtype == np.float32 and v["land_mask"].dtype == np.int8 and v["lat"].dtype == np.float32
    assert np.array_equal(v["land_mask"], z["land_mask"]) and np.array_equal(v["elevation"], f4(z["elevation"]))
    assert np.array_equal(v["base_albedo"], f4(z["base_albedo"])) and np.array_equal(v["friction"], f4(z["friction"]))
    assert np.array_equal(v["lat"], f4(grid.lat)) and np.array_equal(v["lon"], f4(grid.lon))
    assert attrs["title"] == "Qingdai Topography and Surface Properties" and attrs["institution"] == "PyGCM for Qingdai"
    assert float(attrs["sea_level_m"]) == float(z["sea_level_m"]) and float(attrs["target_land_fraction"]) == 0.29
    assert float(attrs["planet_radius_m"]) == 6.371e6 and float(attrs["planet_axial_tilt_deg"]) == 27.0
    assert float(attrs["planet_omega_rad_s"]) == 8.726646259971648e-5
    elev, mask, alb, fric = load_topography_from_netcdf(path, grid, quiet=True)
    assert mask.dtype == np.uint8 and np.array_equal(mask[:, :-1], z["land_mask"][:, :-1]) and np.array_equal(mask[:, -1], mask[:, 0])
    scale = float(np.abs(z["elevation"]).max())
    assert np.allclose(elev[:, :-1], z["elevation"][:, :-1], rtol=0, atol=1e-5 * scale)
    assert np.allclose(alb[:, :-1], z["base_albedo"][:, :-1], rtol=0, atol=1e-5)
    assert np.allclose(fric[:, :-1], z["friction"][:, :-1], rtol=1e-4, atol=0)


def test_driver_switch_defaults_to_the_host_path():
    from qingdai_amd.driver import topo_device
    assert topo_device({}) is False and topo_device({"QD_TOPO_DEVICE": "0"}) is False and topo_device({"QD_TOPO_DEVICE": "1"}) is True
    src = open(os.path.join(ROOT, "qingdai_amd", "driver.py")).read()
    assert "topo.create_land_sea_mask(self.grid)" in src


def test_cabi_declarations_present():
    from qingdai_amd import _lib
    assert "qd_topogen.hip" in open(os.path.join(ROOT, "qingdai_amd", "csrc", "Makefile")).read()
    assert (topogen.MAX_OCTAVES, topogen.MAX_CONTINENTS) == (_lib.C["QD_TOPOGEN_MAX_OCTAVES"], _lib.C["QD_TOPOGEN_MAX_CONTINENTS"])
