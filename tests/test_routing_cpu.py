"""CPU: the river-routing planner (qingdai_amd/routing.py).

The planner refuses what the reference could not run; its segment / junction schedule, emulated in NumPy
(tests/routing_ref.py), reproduces the reference's goldens (flow map bitwise) and a sequential restatement
on a deep snake river and a wide binary tree."""
import glob
import os

import numpy as np
import pytest

from qingdai_amd.grid import SphericalGrid
from qingdai_amd.routing import build_plan, cell_area_rows, network_from_vars
from routing_ref import SeqRouting, case_inputs, case_vars, emulate_accumulate, emulate_event

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "routing_*.npz")))


def _simple(n_lat=5, n_lon=8):
    land = np.zeros((n_lat, n_lon), np.uint8)
    land[1:4, 1:7] = 1
    ft = np.full(n_lat * n_lon, -1, np.int64)
    li = np.where(land.ravel() == 1)[0]
    ft[li[:-1]] = li[1:]
    return dict(land_mask=land, flow_to_index=ft.reshape(n_lat, n_lon), flow_order=li.copy())


def test_refuses_duplicate_flow_order():
    v = _simple()
    v["flow_order"] = np.concatenate([v["flow_order"], v["flow_order"][:1]])
    with pytest.raises(ValueError, match="duplicate"):
        network_from_vars(v, (5, 8))


@pytest.mark.parametrize("bad", [-1, 40, 1000])
def test_refuses_flow_order_outside_grid(bad):
    v = _simple()
    v["flow_order"] = np.concatenate([v["flow_order"], [bad]])
    with pytest.raises(ValueError, match="outside"):
        network_from_vars(v, (5, 8))


def test_refuses_downstream_outside_grid():
    v = _simple()
    ft = v["flow_to_index"].ravel().copy()
    ft[v["flow_order"][2]] = 40
    v["flow_to_index"] = ft.reshape(5, 8)
    net = network_from_vars(v, (5, 8))
    with pytest.raises(ValueError, match="outside the grid"):
        build_plan(net, np.ones(5))


def test_refuses_lake_id_beyond_storages():
    v = _simple()
    lm = np.zeros((5, 8), np.int32)
    lid = np.zeros((5, 8), np.int32)
    lm[2, 3] = 1
    lid[2, 3] = 3
    lid[1, 1] = 1          # max id 3; two outlets coerce n_lakes to 2; the lake cell names lake 3
    v.update(lake_mask=lm, lake_id=lid, lake_outlet_index=np.array([-1, -1]))
    net = network_from_vars(v, (5, 8))
    assert net.n_lakes == 2
    with pytest.raises(ValueError, match="lake id"):
        build_plan(net, np.ones(5))


def test_refuses_bad_shapes_and_missing_variables():
    v = _simple()
    with pytest.raises(ValueError, match="land_mask"):
        network_from_vars({k: a for k, a in v.items() if k != "land_mask"}, (5, 8))
    with pytest.raises(ValueError, match="flow_to_index"):
        network_from_vars({k: a for k, a in v.items() if k != "flow_to_index"}, (5, 8))
    with pytest.raises(ValueError, match="shape"):
        network_from_vars(v, (5, 9))


def test_fallback_order_and_ij_outlets():
    v = _simple()
    del v["flow_order"]
    v.update(lake_mask=np.zeros((5, 8)), lake_id=np.zeros((5, 8)), lake_outlet_i=np.array([2]), lake_outlet_j=np.array([3]))
    v["lake_id"][2, 2] = 1
    net = network_from_vars(v, (5, 8))
    np.testing.assert_array_equal(net.flow_order, np.where(v["land_mask"].ravel() == 1)[0])
    np.testing.assert_array_equal(net.lake_outlet_index, [3 * 8 + 2])


def _check_event(got, want, lake_got=None, lake_want=None):
    np.testing.assert_array_equal(got["flow"], want["flow"])        # bitwise
    s = max(abs(want["mass_input_kg"]), 1e-300) if "mass_input_kg" in want else max(abs(got["mass_input_kg"]), 1e-300)
    assert abs(got["ocean_inflow_kgps"] - want["ocean_inflow_kgps"]) <= 1e-12 * max(abs(want["ocean_inflow_kgps"]), 1e-300)
    assert abs(got["mass_closure_error_kg"] - want["mass_closure_error_kg"]) <= 1e-12 * s
    if lake_want is not None and lake_want.size:
        np.testing.assert_allclose(lake_got, lake_want, rtol=1e-12, atol=1e-12 * s)


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[8:-4] for p in GOLDENS])
def test_schedule_reproduces_golden(path):
    z = np.load(path)
    n_lat, n_lon = (int(x) for x in z["shape"])
    grid = SphericalGrid(n_lat, n_lon)
    net = network_from_vars(case_vars(z), (n_lat, n_lon))
    assert net.n_lakes == int(z["n_lakes"])
    plan = build_plan(net, cell_area_rows(grid))
    buf = np.zeros(n_lat * n_lon)
    lake = np.zeros(max(net.n_lakes, 0))
    dt, dt_h = float(z["dt"]), float(z["dt_hydro_hours"]) * 3600.0
    t_accum, ev = 0.0, 0
    for k in range(int(z["nsteps"])):
        R, P, E = case_inputs(z, k)
        emulate_accumulate(plan, buf, R, dt)
        t_accum += dt
        if t_accum + 1e-9 < dt_h:
            continue
        got = emulate_event(plan, buf, lake, t_accum, P, E)
        t_accum = 0.0
        assert k == z["ev_step"][ev]
        np.testing.assert_array_equal(got["flow"], z["ev_flow"][ev])
        s = max(abs(got["mass_input_kg"]), 1e-300)
        assert abs(got["ocean_inflow_kgps"] - z["ev_ocean"][ev]) <= 1e-12 * abs(z["ev_ocean"][ev])
        assert abs(got["mass_closure_error_kg"] - z["ev_err"][ev]) <= 1e-12 * s
        if net.n_lakes > 0:
            np.testing.assert_allclose(lake, z["ev_lake"][ev], rtol=1e-12, atol=1e-12 * s)
        ev += 1
    assert ev == len(z["ev_step"]) and ev >= 2
    np.testing.assert_array_equal(buf, z["buffer"])
    assert t_accum == float(z["t_accum"])


def _run_both(v, shape, nsteps, dt, dt_h, seed):
    grid = SphericalGrid(*shape)
    net = network_from_vars(v, shape)
    area = cell_area_rows(grid)
    plan = build_plan(net, area)
    seq = SeqRouting(net, area, dt_h)
    rng = np.random.default_rng(seed)
    buf = np.zeros(net.land_mask.size)
    lake = np.zeros(max(net.n_lakes, 0))
    t_accum, n_ev = 0.0, 0
    for k in range(nsteps):
        R = rng.uniform(-2e-6, 2e-5, shape)
        want = seq.step(R, dt)
        emulate_accumulate(plan, buf, R, dt)
        t_accum += dt
        if t_accum + 1e-9 < dt_h:
            assert want is None
            continue
        got = emulate_event(plan, buf, lake, t_accum)
        t_accum = 0.0
        _check_event(got, want)
        n_ev += 1
    np.testing.assert_array_equal(buf, seq.buffer)
    return plan, n_ev


def test_deep_snake_river():
    """One chain of >= 20 000 cells (a boustrophedon river): one segment, one lane."""
    n_lat, n_lon = 160, 144
    land = np.zeros((n_lat, n_lon), np.uint8)
    land[2:n_lat - 2, :] = 1
    cells = []
    for j in range(2, n_lat - 2):
        row = [j * n_lon + i for i in range(n_lon)]
        cells += row if j % 2 == 0 else row[::-1]
    cells = np.array(cells, np.int64)
    assert cells.size >= 20000
    ft = np.full(n_lat * n_lon, -1, np.int64)
    ft[cells[:-1]] = cells[1:]
    v = dict(land_mask=land, flow_to_index=ft.reshape(n_lat, n_lon), flow_order=cells)
    plan, n_ev = _run_both(v, (n_lat, n_lon), 13, 1800.0, 3 * 3600.0, 1)
    assert n_ev == 2
    assert len(plan.seg_start) - 1 == 1 and plan.n_levels == 1


def test_wide_binary_tree():
    """A complete binary tree of 2^13 - 1 cells (the root drains to the ocean): one junction level per depth."""
    n_lat, n_lon = 64, 160
    depth = 13
    n_tree = 2 ** depth - 1
    rng = np.random.default_rng(5)
    cells = rng.permutation(np.arange(n_lon, n_lat * n_lon))[:n_tree]     # row 0 stays ocean
    land = np.zeros(n_lat * n_lon, np.uint8)
    land[cells] = 1
    ft = np.full(n_lat * n_lon, -1, np.int64)
    for k in range(1, n_tree):                  # heap layout: node k drains to (k - 1) // 2
        ft[cells[k]] = cells[(k - 1) // 2]
    order = cells[::-1].copy()                  # leaves first
    v = dict(land_mask=land.reshape(n_lat, n_lon), flow_to_index=ft.reshape(n_lat, n_lon), flow_order=order)
    plan, n_ev = _run_both(v, (n_lat, n_lon), 5, 3600.0, 2 * 3600.0, 2)
    assert n_ev == 2
    assert plan.n_levels == depth


def test_driver_hydro_env_defaults_and_overrides():
    from qingdai_amd.driver import hydro_env
    assert hydro_env({}) == (True, "data/hydrology.nc", 6.0, True)
    assert hydro_env({"QD_HYDRO_ENABLE": "0", "QD_HYDRO_NETCDF": "x.nc", "QD_HYDRO_DT_HOURS": "3", "QD_HYDRO_DIAG": "0"}) == \
        (False, "x.nc", 3.0, False)


def test_driver_missing_network_runs_without_routing(tmp_path, capsys):
    import types
    from qingdai_amd.driver import Simulation
    sim = types.SimpleNamespace()
    missing = str(tmp_path / "nope.nc")
    assert Simulation.enable_routing(sim, {"QD_HYDRO_NETCDF": missing}) is None and sim.routing is None
    assert (f"[HydroRouting] Enabled but network not available; running WITHOUT routing (QD_HYDRO_NETCDF='{missing}')."
            in capsys.readouterr().out)
    assert Simulation.enable_routing(sim, {"QD_HYDRO_ENABLE": "0"}) is None
    assert "[HydroRouting] Disabled by QD_HYDRO_ENABLE=0." in capsys.readouterr().out
