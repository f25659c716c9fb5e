"""GPU (-m gpu): network generation on the device (qd_hydronet.hip) -- every golden of the reference's generator bit for bit,
721 x 1440 pit-fill sweeps and stages against the restatements (tests/hydronet_ref.py), determinism, the driver's
QD_HYDRO_AUTOGEN path, and the refusals."""
import glob
import os
import time

import numpy as np
import pytest

import qingdai_amd as qa
import hydronet_ref as hr
from qingdai_amd.device import Device
from qingdai_amd.hydronet import HydroNetError, generate_network, host_tables, write_network
from qingdai_amd.topography import create_land_sea_mask, generate_elevation_map

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "hydronet_*.npz")))
IDS = [os.path.basename(p)[9:-4] for p in GOLDENS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_golden_bitwise(gpu, path):
    z = np.load(path)
    shape, land, elev, eps, max_iters = hr.case_inputs(z)
    grid = qa.SphericalGrid(*shape)
    dev = Device(grid)
    net = generate_network(grid, land, elev, eps=eps, max_iters=max_iters, dev=dev)
    assert net["sweeps"] == int(z["sweeps"])
    assert np.array_equal(_bits(net["elevation_filled"]), _bits(hr.golden_filled(z, elev)))
    assert net["flow_to_index"].dtype == np.int64 and net["flow_order"].dtype == np.int64
    for k in ("flow_to_index", "flow_order", "lake_mask", "lake_id", "lake_outlet_index"):
        assert np.array_equal(net[k], z[k]), k
    assert net["lake_mask"].dtype == np.uint8 and net["lake_id"].dtype == np.int32 and net["lake_outlet_index"].dtype == np.int32
    assert np.array_equal(net["land_mask"], land) and net["n_lakes"] == int(z["n_lakes"])
    dev.close()


def _fullsize(kind):
    grid = qa.SphericalGrid(721, 1440)
    land = create_land_sea_mask(grid)
    elev = np.zeros((721, 1440)) if kind == "zero" else generate_elevation_map(grid, seed=42)
    return grid, land, elev


@pytest.mark.parametrize("kind", ["zero", "proc"])
def test_fullsize_first_sweeps(gpu, kind):
    grid, land, elev = _fullsize(kind)
    dev = Device(grid)
    for it in (1, 3):
        net = generate_network(grid, land, elev, max_iters=it, dev=dev)
        want, run = hr.pit_fill_sweeps(elev, land, 1e-3, it)
        assert net["sweeps"] == run
        assert np.array_equal(_bits(net["elevation_filled"]), _bits(want)), it
    dev.close()


@pytest.mark.parametrize("kind", ["zero", "proc"])
def test_fullsize_stages(gpu, kind):
    grid, land, elev = _fullsize(kind)
    dev = Device(grid)
    generate_network(grid, land, elev, dev=dev)                     # warm-up (module load, first allocations)
    t0 = time.perf_counter()
    net = generate_network(grid, land, elev, dev=dev)
    wall = time.perf_counter() - t0
    print(f"\n721x1440 {kind}: {wall:.3f} s, {net['sweeps']} sweeps, {net['n_lakes']} lakes")
    ef = net["elevation_filled"]
    assert np.array_equal(ef[land != 1], elev[land != 1])
    if net["sweeps"] < 200:                                          # converged: one more sweep changes nothing
        again, run = hr.pit_fill_sweeps(ef, land, 1e-3, 1)
        assert np.array_equal(_bits(again), _bits(ef))
    lat, lon, cp = host_tables(grid)
    flow = hr.d8(lat, lon, cp, land, ef)
    assert np.array_equal(net["flow_to_index"], flow)
    lm, lid, nl = hr.lakes(flow, land)
    assert np.array_equal(net["lake_mask"], lm) and np.array_equal(net["lake_id"], lid) and net["n_lakes"] == nl
    assert np.array_equal(net["lake_outlet_index"], hr.outlets(ef, lm, lid, land, nl))
    assert np.array_equal(net["flow_order"], hr.flow_order(flow, land))
    again = generate_network(grid, land, elev, dev=dev)             # two runs are bit-identical
    for k in ("elevation_filled", "flow_to_index", "flow_order", "lake_mask", "lake_id", "lake_outlet_index"):
        assert np.array_equal(np.asarray(again[k]).view(np.uint8), np.asarray(net[k]).view(np.uint8)), k
    dev.close()


def _driver_run(tmp_path, monkeypatch, capsys, sub, extra):
    from qingdai_amd import driver
    for k in list(os.environ):
        if k.startswith("QD_"):
            monkeypatch.delenv(k)
    d = tmp_path / sub
    d.mkdir()
    env = {"QD_N_LAT": "19", "QD_N_LON": "36", "QD_SIM_DAYS": "0.05", "QD_ECO_ENABLE": "0", "QD_DATA_DIR": str(d / "data"),
           "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1", "QD_HYDRO_DT_HOURS": "0.5", "QD_AUTOSAVE_ENABLE": "0"}
    env.update(extra)
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    monkeypatch.chdir(d)
    assert driver.main() == 0
    return capsys.readouterr().out


def test_driver_autogen_matches_golden_file(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd.ncio import read_nc
    z = np.load(os.path.join(HERE, "golden", "hydronet_zero_19x36.npz"))
    auto = str(tmp_path / "gen" / "hydro" / "auto.nc")
    out_a = _driver_run(tmp_path, monkeypatch, capsys, "a", {"QD_HYDRO_NETCDF": auto, "QD_HYDRO_AUTOGEN": "1"})
    assert f"[HydroRouting] Auto-generating network to '{auto}' (source=procedural)..." in out_a, out_a
    assert "[HydroRouting] Network auto-generation complete." in out_a and "WITHOUT routing" not in out_a
    assert f"[HydroRouting] Enabled with network '{auto}'." in out_a
    v, attrs = read_nc(auto)
    assert attrs["created_by"] == "scripts/run_simulation.py (auto)"
    for k in ("flow_to_index", "flow_order", "lake_id", "lake_outlet_index"):
        assert np.array_equal(v[k], z[k]), k
    # the same run given a file written from the golden routes exactly alike
    shape, land, elev, _, _ = hr.case_inputs(z)
    gold = str(tmp_path / "golden.nc")
    write_network(gold, qa.SphericalGrid(*shape), {"land_mask": land, "elevation_filled": hr.golden_filled(z, elev),
                                                   "flow_to_index": z["flow_to_index"], "flow_order": z["flow_order"],
                                                   "lake_mask": z["lake_mask"], "lake_id": z["lake_id"],
                                                   "lake_outlet_index": z["lake_outlet_index"]})
    out_b = _driver_run(tmp_path, monkeypatch, capsys, "b", {"QD_HYDRO_NETCDF": gold})
    ev = lambda o: [ln for ln in o.split("\n") if ln.startswith("[HydroRouting] ocean_inflow=") or ln.startswith("[Routing]")]
    assert len(ev(out_a)) >= 3 and ev(out_a) == ev(out_b), (out_a, out_b)
    # without the switch: no generation, the run goes on without routing
    missing = str(tmp_path / "missing.nc")
    out_c = _driver_run(tmp_path, monkeypatch, capsys, "c", {"QD_HYDRO_NETCDF": missing})
    assert "Auto-generating" not in out_c and "[HydroRouting] Enabled but network not available; running WITHOUT routing" in out_c
    assert not os.path.exists(missing)


def test_refusals(gpu):
    grid = qa.SphericalGrid(73, 144)
    banded = Device(grid, row0=20, n_rows=30, halo=6)
    land = create_land_sea_mask(grid)
    with pytest.raises(HydroNetError, match="whole-globe"):
        generate_network(grid, land, dev=banded)
    banded.close()
    dev = Device(grid)
    elev = np.zeros((73, 144))
    j, i = np.argwhere(land == 1)[0]
    elev[j, i] = np.nan
    with pytest.raises(HydroNetError, match="non-finite"):
        generate_network(grid, land, elev, dev=dev)
    with pytest.raises(HydroNetError, match="0 and 1"):
        generate_network(grid, land * 2, dev=dev)
    net = generate_network(grid, land, dev=dev)                     # the handle still works
    assert net["sweeps"] > 0
    dev.close()
