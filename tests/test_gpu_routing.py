"""GPU (-m gpu): river routing on the device (qd_route.hip) -- the class seam against the reference's goldens, a
721 x 1440 network and the resident loop (qd_step_n bit7) against the sequential restatement (tests/routing_ref.py),
no feedback on the prognostic state, the driver's event lines, and the refusal on a banded handle."""
import glob
import os
from collections import deque

import numpy as np
import pytest

import qingdai_amd as qa
from qingdai_amd.device import Device
from qingdai_amd.routing import RiverRouting, cell_area_rows, network_from_vars
from qingdai_amd.topography import create_land_sea_mask
from routing_ref import SeqRouting, case_inputs, case_vars

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "routing_*.npz")))


def synthetic_network(land, seed):
    """Steepest descent on a seeded smooth field over `land` (D8, periodic in longitude), pits become one-cell lakes whose
    outlet is their lowest land neighbour (pointing anywhere in the order), then Kahn order over the land edges."""
    n_lat, n_lon = land.shape
    rng = np.random.default_rng(seed)
    lat = np.linspace(-np.pi / 2, np.pi / 2, n_lat)[:, None]
    lon = np.linspace(0, 2 * np.pi, n_lon)[None, :]
    z = np.zeros((n_lat, n_lon))
    for _ in range(6):
        z += rng.uniform(100, 600) * np.sin(rng.uniform(1, 6) * lat + rng.uniform(0, 6)) * np.cos(rng.integers(1, 8) * lon + rng.uniform(0, 6))
    z += rng.normal(0, 5.0, z.shape)
    jj, ii = np.meshgrid(np.arange(n_lat), np.arange(n_lon), indexing="ij")
    best = z.copy()
    best_idx = np.full((n_lat, n_lon), -1, np.int64)
    low_land = np.full((n_lat, n_lon), np.inf)
    low_land_idx = np.full((n_lat, n_lon), -1, np.int64)
    for dj in (-1, 0, 1):
        for di in (-1, 0, 1):
            if dj == 0 and di == 0:
                continue
            nj = np.clip(jj + dj, 0, n_lat - 1)
            ni = (ii + di) % n_lon
            zn = z[nj, ni]
            nidx = nj * n_lon + ni
            better = zn < best
            best = np.where(better, zn, best)
            best_idx = np.where(better, nidx, best_idx)
            lb = (land[nj, ni] == 1) & (zn < low_land) & (nidx != jj * n_lon + ii)
            low_land = np.where(lb, zn, low_land)
            low_land_idx = np.where(lb, nidx, low_land_idx)
    lf = land.ravel() == 1
    ft = best_idx.ravel().copy()
    ft[~lf] = -1
    ft = np.where((ft >= 0) & ~lf[np.clip(ft, 0, None)], -1, ft)
    pits = lf & (best_idx.ravel() < 0)
    lake_mask = pits.astype(np.uint8)
    lake_id = np.zeros(land.size, np.int32)
    n_lakes = min(int(pits.sum()), 256)          # pits grouped into at most 256 lakes (the reference's P-E split is O(lakes x cells))
    lake_id[pits] = 1 + np.arange(pits.sum()) % max(n_lakes, 1)
    outlet = low_land_idx.ravel()[pits][:n_lakes]
    # Kahn over land -> land edges
    indeg = np.bincount(ft[lf & (ft >= 0)], minlength=land.size)
    q = deque(np.where(lf & (indeg == 0))[0].tolist())
    ftl = ft.tolist()
    order = []
    while q:
        u = q.popleft()
        order.append(u)
        d = ftl[u]
        if d >= 0:
            indeg[d] -= 1
            if indeg[d] == 0:
                q.append(d)
    return dict(land_mask=land.astype(np.uint8), flow_to_index=ft.reshape(land.shape), flow_order=np.array(order, np.int64),
                lake_mask=lake_mask.reshape(land.shape), lake_id=lake_id.reshape(land.shape), lake_outlet_index=outlet)


def _close(got, want, scale):
    assert abs(got - want) <= 1e-12 * max(abs(scale), 1e-300), (got, want)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[8:-4] for p in GOLDENS])
def test_class_seam_reproduces_golden(gpu, path):
    z = np.load(path)
    n_lat, n_lon = (int(x) for x in z["shape"])
    grid = qa.SphericalGrid(n_lat, n_lon)
    dev = Device(grid)
    rr = RiverRouting.from_arrays(grid, dt_hydro_hours=float(z["dt_hydro_hours"]), diag=False, dev=dev, **case_vars(z))
    d0 = rr.diagnostics()
    assert d0["ocean_inflow_kgps"] == 0.0 and not np.any(d0["flow_accum_kgps"])
    ev = 0
    for k in range(int(z["nsteps"])):
        R, P, E = case_inputs(z, k)
        rr.step(R, float(z["dt"]), precip_flux=P, evap_flux=E)
        if rr.t_accum != 0.0:                    # dt > 0: only an event leaves t_accum at zero
            continue
        d = rr.diagnostics()
        rec = dev.route_last_event()
        assert k == z["ev_step"][ev]
        np.testing.assert_array_equal(d["flow_accum_kgps"], z["ev_flow"][ev])         # bitwise
        _close(d["ocean_inflow_kgps"], z["ev_ocean"][ev], z["ev_ocean"][ev])
        _close(d["mass_closure_error_kg"], z["ev_err"][ev], rec["mass_input_kg"])
        if rr.n_lakes > 0:
            np.testing.assert_allclose(d["lake_volume_kg"], z["ev_lake"][ev], rtol=1e-12, atol=1e-12 * rec["mass_input_kg"])
        ev += 1
    assert ev == len(z["ev_step"]) >= 2
    np.testing.assert_array_equal(rr.buffer_kg().ravel(), z["buffer"])
    assert rr.t_accum == float(z["t_accum"])
    rr.reset()
    assert not np.any(rr.buffer_kg()) and rr.diagnostics()["ocean_inflow_kgps"] == 0.0
    rr.close()
    dev.close()


def test_fullsize_network_two_events(gpu):
    n_lat, n_lon = 721, 1440
    grid = qa.SphericalGrid(n_lat, n_lon)
    land = create_land_sea_mask(grid)
    v = synthetic_network(land, 11)
    dev = Device(grid)
    rr = RiverRouting.from_arrays(grid, dt_hydro_hours=1.0, diag=False, dev=dev, **v)
    net = network_from_vars(v, (n_lat, n_lon))
    seq = SeqRouting(net, cell_area_rows(grid), rr.dt_hydro_seconds)
    rng = np.random.default_rng(3)
    n_ev = 0
    for k in range(8):
        R = rng.uniform(-1e-6, 2e-5, (n_lat, n_lon))
        P = rng.uniform(0, 4e-5, (n_lat, n_lon))
        E = rng.uniform(0, 3e-5, (n_lat, n_lon))
        rr.step(R, 900.0, precip_flux=P, evap_flux=E)
        want = seq.step(R, 900.0, P, E)
        if want is None:
            continue
        n_ev += 1
        d = rr.diagnostics()
        np.testing.assert_array_equal(d["flow_accum_kgps"], want["flow"])
        _close(d["ocean_inflow_kgps"], want["ocean_inflow_kgps"], want["ocean_inflow_kgps"])
        _close(d["mass_closure_error_kg"], want["mass_closure_error_kg"], want["mass_input_kg"])
        np.testing.assert_allclose(d["lake_volume_kg"], want["lake_volume_kg"], rtol=1e-12, atol=1e-12 * want["mass_input_kg"])
    assert n_ev == 2
    rr.close()
    dev.close()


def _sim(n_lat, n_lon):
    from qingdai_amd.driver import Simulation
    return Simulation(n_lat, n_lon, quiet=True, use_ocean=True, ecology=False, phyto=False)


def test_resident_loop_spans(gpu):
    """bit7 in one span of 160 steps and in 160 one-step spans: identical event logs and flow maps, equal to the restatement
    fed with the RUNOFF / PRECIP / EFLUX each step left on the device."""
    n = 160
    runs = []
    for one_step in (False, True):
        sim = _sim(181, 360)
        v = synthetic_network(sim.land_mask, 5)
        sim.routing = RiverRouting.from_arrays(sim.grid, dt_hydro_hours=3.0, diag=False, dev=sim.dev, **v)
        log, fields = [], []
        if one_step:
            for k in range(n):
                sim._run_chunk(1)
                log += [sim.routing.dev.route_last_event()] if sim.routing.t_accum == 0.0 else []
                fields.append(tuple(sim.dev.get(f).copy() for f in ("RUNOFF", "PRECIP", "EFLUX")))
        else:
            sim.dev.step_n(sim.forcing.star_table(sim.t + sim.dt * np.arange(n)), float(sim.dt), with_ocean=True, with_physics=True,
                           pass_albedo=False, with_hydrology=True, routing=sim.routing)
            log = sim.dev.route_events()
            sim.routing.take_events(log)
        runs.append((log, sim.routing.diagnostics()["flow_accum_kgps"].copy(), fields, v, sim))
    (log_a, flow_a, _, v, sim_a), (log_b, flow_b, fields, _, sim_b) = runs
    assert len(log_a) >= 2
    assert [tuple(e.values()) for e in log_a] == [tuple(e.values()) for e in log_b]
    np.testing.assert_array_equal(flow_a, flow_b)
    net = network_from_vars(v, sim_b.grid.lat_mesh.shape)
    seq = SeqRouting(net, cell_area_rows(sim_b.grid), 3.0 * 3600.0)
    for k, (R, P, E) in enumerate(fields):
        seq.step(R, sim_b.dt, P, E, step_index=k + 1)
    assert len(seq.events) == len(log_a)
    for e, w in zip(log_a, seq.events):
        assert e["step"] == w["step"] and e["event_dt"] == w["event_dt"]
        _close(e["ocean_inflow_kgps"], w["ocean_inflow_kgps"], w["ocean_inflow_kgps"])
        _close(e["mass_closure_error_kg"], w["mass_closure_error_kg"], w["mass_input_kg"])
    np.testing.assert_array_equal(flow_a, seq.events[-1]["flow"])


def test_routing_has_no_feedback(gpu):
    """The prognostic state after a span with routing is bit-identical to the same span without it."""
    states = []
    for with_routing in (False, True):
        sim = _sim(91, 180)
        if with_routing:
            sim.routing = RiverRouting.from_arrays(sim.grid, dt_hydro_hours=1.0, diag=False, dev=sim.dev,
                                                   **synthetic_network(sim.land_mask, 2))
        sim._run_chunk(40)
        states.append({f: sim.dev.get(f).copy() for f in ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "UO", "VO", "ETA", "SST",
                                                           "W_LAND", "S_SNOW", "RUNOFF", "PRECIP", "EFLUX")})
    for f in states[0]:
        np.testing.assert_array_equal(states[0][f], states[1][f], err_msg=f)


def test_driver_main_prints_event_lines(gpu, tmp_path, monkeypatch, capsys):
    from qingdai_amd import driver, ncio
    for k in list(os.environ):
        if k.startswith("QD_"):
            monkeypatch.delenv(k)
    grid = qa.SphericalGrid(37, 72)
    v = synthetic_network(create_land_sea_mask(grid), 4)
    nc = tmp_path / "hydrology.nc"
    nl = int(v["lake_outlet_index"].size)
    ncio.write_nc(str(nc), {"lat": 37, "lon": 72, "n_land": int(v["flow_order"].size), "n_lakes": nl},
                  {"land_mask": ("u1", ("lat", "lon"), v["land_mask"]), "flow_to_index": ("i4", ("lat", "lon"), v["flow_to_index"]),
                   "flow_order": ("i4", ("n_land",), v["flow_order"]), "lake_mask": ("u1", ("lat", "lon"), v["lake_mask"]),
                   "lake_id": ("i4", ("lat", "lon"), v["lake_id"]), "lake_outlet_index": ("i4", ("n_lakes",), v["lake_outlet_index"])})
    env = {"QD_N_LAT": "37", "QD_N_LON": "72", "QD_SIM_DAYS": "0.05", "QD_ECO_ENABLE": "0", "QD_DATA_DIR": str(tmp_path / "data"),
           "QD_DYN_DIAG_PRINT": "0", "QD_USE_OCEAN": "1", "QD_HYDRO_NETCDF": str(nc), "QD_HYDRO_DT_HOURS": "0.5",
           "QD_AUTOSAVE_ENABLE": "0"}
    for k, val in env.items():
        monkeypatch.setenv(k, val)
    monkeypatch.chdir(tmp_path)
    assert driver.main() == 0
    out = capsys.readouterr().out
    assert "[Routing] Loaded network:" in out and f"[HydroRouting] Enabled with network '{nc}'." in out, out
    assert out.count("[HydroRouting] ocean_inflow=") == 2, out          # 12 steps of 300 s, an event every 1800 s


def test_banded_handle_refuses_routing(gpu):
    grid = qa.SphericalGrid(73, 144)
    dev = Device(grid, row0=20, n_rows=30, halo=6)
    with pytest.raises(qa._lib.QdError, match="whole-globe"):
        RiverRouting.from_arrays(grid, diag=False, dev=dev, **synthetic_network(create_land_sea_mask(grid), 1))
    import ctypes
    st = np.zeros((1, 7))
    rc = dev.lib.qd_step_n(dev.h, 1, 300.0, 8 | 128, st.ctypes.data_as(ctypes.POINTER(ctypes.c_double)))
    assert rc != 0 and b"whole-globe" in dev.lib.qd_last_error(dev.h)
    dev.close()
