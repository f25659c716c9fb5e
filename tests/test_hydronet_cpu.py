"""CPU: network generation (qingdai_amd/hydronet.py) without a GPU -- the host tables against the reference's, the NetCDF
writer and RiverRouting's reader, the QD_HYDRO_AUTOGEN switch, the C-ABI declarations, and the test restatements
(tests/hydronet_ref.py) against the reference's goldens."""
import glob
import os

import numpy as np
import pytest

import qingdai_amd as qa
import hydronet_ref as hr
from qingdai_amd.hydronet import host_tables, write_network

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "hydronet_*.npz")))
IDS = [os.path.basename(p)[9:-4] for p in GOLDENS]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.mark.parametrize("path", GOLDENS, ids=IDS)
def test_host_tables_equal_reference_tables(path):
    z = np.load(path)
    lat, lon, cos_pair = host_tables(qa.SphericalGrid(*(int(x) for x in z["shape"])))
    for name, got in (("lat_rad", lat), ("lon_rad", lon), ("cos_pair", cos_pair)):
        assert np.array_equal(_bits(got), _bits(z[name])), (
            f"{name}: this host's NumPy / CPU rounds the spherical_distance tables differently from the host that wrote the "
            f"golden -- an environment mismatch, not a kernel bug")


def test_goldens_cover_the_cases():
    z = {i: np.load(p) for i, p in zip(IDS, GOLDENS)}
    assert len(z) >= 10
    assert all(os.path.getsize(p) < 450 * 1024 for p in GOLDENS)
    assert int(z["zero_73x144"]["sweeps"]) < 200 and int(z["proc_181x360_it200"]["sweeps"]) == 200
    assert int(np.sum(z["inland_37x72"]["lake_outlet_index"] >= 0)) > 10          # lakes with real outlets
    land = z["valley_25x400"]["land_mask"]
    assert land[0].all() and land[-1].all()                                         # land on both pole rows


@pytest.mark.parametrize("path", [p for p, i in zip(GOLDENS, IDS) if "it200" not in i], ids=[i for i in IDS if "it200" not in i])
def test_restatements_reproduce_golden(path):
    """The plain restatements the 721 x 1440 GPU checks lean on agree with the reference's generator."""
    z = np.load(path)
    shape, land, elev, eps, max_iters = hr.case_inputs(z)
    lat, lon, cp = host_tables(qa.SphericalGrid(*shape))
    ef, sweeps = hr.pit_fill_sweeps(elev, land, eps, max_iters)
    want = hr.golden_filled(z, elev)
    assert np.array_equal(_bits(ef), _bits(want)) and sweeps == int(z["sweeps"])
    flow = hr.d8(lat, lon, cp, land, want)
    assert np.array_equal(flow, z["flow_to_index"])
    lm, lid, nl = hr.lakes(flow, land)
    assert np.array_equal(lm, z["lake_mask"]) and np.array_equal(lid, z["lake_id"]) and nl == int(z["n_lakes"])
    assert np.array_equal(hr.outlets(want, lm, lid, land, nl), z["lake_outlet_index"])
    assert np.array_equal(hr.flow_order(flow, land), z["flow_order"])


def _golden_net(z):
    shape, land, elev, _, _ = hr.case_inputs(z)
    return shape, {"land_mask": land, "elevation_filled": hr.golden_filled(z, elev), "flow_to_index": z["flow_to_index"],
                   "flow_order": z["flow_order"], "lake_mask": z["lake_mask"], "lake_id": z["lake_id"],
                   "lake_outlet_index": z["lake_outlet_index"]}


@pytest.mark.parametrize("auto", [False, True])
def test_writer_round_trips_and_routing_reader_accepts(tmp_path, auto):
    from qingdai_amd.ncio import read_nc
    from qingdai_amd.routing import build_plan, cell_area_rows, network_from_vars
    z = np.load(os.path.join(HERE, "golden", "hydronet_inland_37x72.npz"))
    shape, net = _golden_net(z)
    grid = qa.SphericalGrid(*shape)
    path = str(tmp_path / "net.nc")
    write_network(path, grid, net, auto=auto)
    v, attrs = read_nc(path)
    assert np.array_equal(v["land_mask"], net["land_mask"]) and np.array_equal(v["lake_mask"], net["lake_mask"])
    for k in ("flow_to_index", "flow_order", "lake_id", "lake_outlet_index"):
        assert v[k].dtype == np.int32 and np.array_equal(v[k], net[k]), k
    assert v["elevation_filled"].dtype == np.float32
    assert np.array_equal(v["elevation_filled"], net["elevation_filled"].astype(np.float32))
    assert np.array_equal(v["lat"], grid.lat.astype(np.float32)) and np.array_equal(v["lon"], grid.lon.astype(np.float32))
    assert attrs["title"] == ("Qingdai Hydrology Network (auto-generated)" if auto else "Qingdai Hydrology Network")
    assert attrs["created_by"] == ("scripts/run_simulation.py (auto)" if auto else "scripts/generate_hydrology_maps.py")
    assert ("notes" in attrs) != auto and attrs["projection"] == "latlon"
    rn = network_from_vars(v, shape)                      # what RiverRouting reads, validated
    assert rn.n_lakes == int(z["n_lakes"]) > 0 and np.array_equal(rn.lake_outlet_index, z["lake_outlet_index"])
    build_plan(rn, cell_area_rows(grid))


def test_writer_without_lakes_has_no_lake_dimension(tmp_path):
    from qingdai_amd.ncio import read_nc_full
    grid = qa.SphericalGrid(5, 8)
    land = np.zeros((5, 8), np.uint8)
    net = {"land_mask": land, "elevation_filled": np.zeros((5, 8)), "flow_to_index": np.full((5, 8), -1),
           "flow_order": np.zeros(0, np.int64), "lake_mask": land, "lake_id": np.zeros((5, 8), np.int32),
           "lake_outlet_index": np.zeros(0, np.int32)}
    write_network(str(tmp_path / "n.nc"), grid, net)
    dims, v, _ = read_nc_full(str(tmp_path / "n.nc"))
    assert "n_lakes" not in dims and "lake_outlet_index" not in v and dims["n_land"] == 0


def test_autogen_switch_parsing():
    from qingdai_amd.driver import hydro_autogen
    assert hydro_autogen({}) is False
    assert hydro_autogen({"QD_HYDRO_AUTOGEN": "0"}) is False
    assert hydro_autogen({"QD_HYDRO_AUTOGEN": "1"}) is True


def test_autogen_unset_is_unchanged_and_failure_is_reported(tmp_path, capsys):
    import types
    from qingdai_amd.driver import Simulation
    missing = str(tmp_path / "nope.nc")
    no_route = f"[HydroRouting] Enabled but network not available; running WITHOUT routing (QD_HYDRO_NETCDF='{missing}')."
    sim = types.SimpleNamespace()
    assert Simulation.enable_routing(sim, {"QD_HYDRO_NETCDF": missing}) is None
    out = capsys.readouterr().out
    assert out.strip() == no_route                                   # nothing generated, nothing else said
    # QD_HYDRO_AUTOGEN=1 with a run that cannot build one: the reference's failure line, then the run goes on without routing
    sim = types.SimpleNamespace(autogen_network=lambda p, e: Simulation.autogen_network(sim, p, e))
    assert Simulation.enable_routing(sim, {"QD_HYDRO_NETCDF": missing, "QD_HYDRO_AUTOGEN": "1"}) is None
    out = capsys.readouterr().out.strip().split("\n")
    assert out[0] == f"[HydroRouting] Auto-generating network to '{missing}' (source=procedural)..."
    assert out[1].startswith("[HydroRouting] Auto-generation failed: ") and out[2] == no_route
    assert not os.path.exists(missing)


def test_cabi_declarations_present():
    assert "qd_hydronet.hip" in open(os.path.join(ROOT, "qingdai_amd", "csrc", "Makefile")).read()
