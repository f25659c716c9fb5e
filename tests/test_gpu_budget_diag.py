"""GPU (-m gpu): the periodic budget diagnostics lane (csrc/qd_budget_diag.hip, qingdai_amd/budget_diag.py).

Records, through the C-ABI with an arbitrary schedule (one-step spans, so that the fields a position read can be downloaded):
each position's numbers against tests/budget_diag_ref.py on the downloaded fields.
  * extrema (eta min / max, max_flow) are selections: exact;
  * weighted means and Umax differ from NumPy by summation order only: |got - want| / (|want| + 1) < 1e-12, the bound
    test_gpu_parity.py::test_energy_diagnostics_vs_oracle holds for the same kind of comparison;
  * closure: total_reservoir_mean, d/dt and the three flux means at that bound; the residual is a difference of near-equal numbers
    and gets the absolute bound those imply: 1e-12 * (2 (|total| + 1) / dt_since_prev + |E| + |P| + |R| + 3).
[EnergyDiag] reads T_s, h, u, v, h_ice, LH as the previous step left them and this step's isr / albedo; [OceanE] reads the SST in
front of the polar fill -- the downloaded SST differs from it only on the two pole rows, whose weight is cos(90 deg) = 6e-17.
Span invariance and no-perturbation are bitwise."""
import os

import numpy as np
import pytest

from test_gpu_routing import synthetic_network

pytestmark = pytest.mark.gpu

DT = 300.0
TOL = 1e-12
RESTART = ("U", "V", "H", "TS", "Q", "CLOUD", "HICE", "W_LAND", "S_SNOW", "UO", "VO", "ETA", "SST")


def close(got, want, keys=None):
    for k in (keys or want):
        e = abs(got[k] - want[k]) / (abs(want[k]) + 1.0)
        print(f"  {k}: got {got[k]!r} want {want[k]!r} err {e:.2e}")
        assert e < TOL, (k, got[k], want[k], e)


def make(monkeypatch, nlat, nlon, *, ocean=True, routing=True, lw_v2=1, ice=False, env=None, fires=None):
    """A Simulation without ecology and tracers, a seeded state, a synthetic river network and a budget lane whose schedule is
    `fires` {run-local index: value} instead of the i % 200 clock."""
    import qingdai_amd as qa
    from qingdai_amd import budget_diag as bd
    from qingdai_amd.driver import Simulation
    from qingdai_amd.routing import RiverRouting
    for k in [k for k in os.environ if k.startswith(("QD_ECO_", "QD_PHYTO_", "QD_OCEAN_", "QD_BUDGET", "QD_LW_"))]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    sim = Simulation(nlat, nlon, params=qa.QdParams(lw_v2=lw_v2), use_ocean=ocean, quiet=True, ecology=False, individuals=False, phyto=False)
    r = np.random.default_rng(nlat * 1000 + nlon)
    lat = np.deg2rad(sim.grid.lat_mesh)
    land = sim.land_mask == 1
    sim.gcm.h = 8000.0 - 400.0 * np.sin(lat) ** 2 + 20.0 * r.normal(size=lat.shape)
    sim.gcm.T_s = 262.0 + 36.0 * np.cos(lat) ** 2 + r.normal(size=lat.shape)
    sim.gcm.u = 8.0 * np.cos(lat) + r.normal(size=lat.shape)
    sim.gcm.v = r.normal(size=lat.shape)
    dev = sim.dev
    dev.set("S_SNOW", np.where(land & (np.abs(sim.grid.lat_mesh) > 55), 60.0, 0.0))
    dev.set("W_LAND", np.where(land, 40.0 * r.random(lat.shape), 0.0))
    dev.set("LH", np.abs(r.normal(40.0, 20.0, lat.shape)))
    dev.set("CLOUD_EFF", np.clip(0.5 + 0.2 * r.normal(size=lat.shape), 0.0, 1.0))       # cloud_for_rad: stays as uploaded
    if ocean:
        dev.set("SST", np.where(~land, 271.0 + 28.0 * np.cos(lat) ** 2 + 0.5 * r.normal(size=lat.shape), 288.0))
        dev.set("UO", np.where(~land, 0.1 * r.normal(size=lat.shape), 0.0))
        dev.set("VO", np.where(~land, 0.1 * r.normal(size=lat.shape), 0.0))
        dev.set("ETA", np.where(~land, 0.05 * r.normal(size=lat.shape), 0.0))
    if ice:                                                  # sea ice over the ocean poleward of 50 degrees, cold enough to stay
        icy = ~land & (np.abs(sim.grid.lat_mesh) > 50)
        dev.set("HICE", np.where(icy, 0.8, 0.0))
        sim.gcm.T_s = np.where(icy, 255.0, sim.gcm.T_s)
    dev.flush()
    sim.routing = None
    if routing:
        sim.routing = RiverRouting.from_arrays(sim.grid, dt_hydro_hours=2 * DT / 3600.0, diag=False, dev=dev, **synthetic_network(sim.land_mask, 4))

    class Scheduled(bd.BudgetDiag):
        def span_schedule(self, t0, dt, n):
            fire = np.array([fires.get(self.i + s, 0) for s in range(n)], dtype=np.int32)
            self.dev.budget_diag_schedule(fire)
            return [(self.i + int(s), int(fire[s])) for s in np.flatnonzero(fire)], int(n)
    lines = []
    if fires is not None:
        sim.budget = Scheduled(dev, sim.grid, dict(os.environ), with_ocean=ocean, routed=routing, out=lines.append)
    sim.budget_lines = lines
    return sim


def fetch(dev, names):
    for k in names:
        dev._host.pop(k, None)
    return {k: np.array(dev.get(k)) for k in names}


CASES = {
    "default_19x36": dict(shape=(19, 36)),
    "default_37x72": dict(shape=(37, 72)),
    "default_25x400": dict(shape=(25, 400)),
    "lw_v1": dict(shape=(19, 36), lw_v2=0),
    "no_ocean": dict(shape=(19, 36), ocean=False),
    "routing_off": dict(shape=(19, 36), routing=False),
    "sea_ice": dict(shape=(37, 72), ice=True),
    "no_polar_ocean": dict(shape=(19, 36), env={"QD_OCEAN_POLAR_LAT": "95"}),
}


@pytest.mark.parametrize("case", list(CASES))
def test_records_vs_restatement(gpu, monkeypatch, case):
    import qd_oracle as qo
    import budget_diag_ref as ref
    from qingdai_amd import budget_diag as bd
    cfg = dict(CASES[case])
    nlat, nlon = cfg.pop("shape")
    ocean, routing = cfg.get("ocean", True), cfg.get("routing", True)
    sim = make(monkeypatch, nlat, nlon, fires={0: 3, 1: 3}, **cfg)
    dev, p, lat_mesh = sim.dev, sim.dev.params, sim.grid.lat_mesh
    P = qo.defaults(lw_v2=cfg.get("lw_v2", 1))
    fmt = sim.budget.fmt
    polar_lat = float((cfg.get("env") or {}).get("QD_OCEAN_POLAR_LAT", "60"))
    land = sim.land_mask
    prev_sst, prev_total = None, None
    for i in range(2):
        pre = fetch(dev, ("TS", "H", "U", "V", "HICE", "LH", "CLOUD_EFF"))
        got_recs = []
        orig = dev.budget_diag_log
        dev.budget_diag_log = lambda: got_recs.append(orig()) or got_recs[-1]
        sim.run_steps(1)
        dev.budget_diag_log = orig
        rec = got_recs[0]
        assert rec.shape == (1, bd.LOG_W) and rec[0, bd.REC["FIRE"]] == 3.0
        rec = rec[0]
        post = fetch(dev, ("ISR", "ALBEDO", "EFLUX", "PCOND", "LH", "LHREL", "PRECIP", "RUNOFF", "Q", "HICE", "W_LAND", "S_SNOW", "UO", "VO", "ETA",
                           "SST", "QNET", "TS"))
        print(f"{case} step {i}")
        assert rec[bd.REC["RAN_ENERGY"]] == 1.0 and rec[bd.REC["RAN_HUMIDITY"]] == 1.0 and rec[bd.REC["RAN_WATER"]] == 1.0
        close(bd.energy_values(rec, fmt.wsum), ref.energy(lat_mesh, post["ISR"], post["ALBEDO"], pre["CLOUD_EFF"], pre["TS"], pre["H"], pre["U"],
                                                          pre["V"], land, pre["HICE"], pre["LH"], P))
        close(bd.humidity_values(rec, fmt.wsum), ref.humidity(lat_mesh, post["EFLUX"], post["PCOND"], post["LH"], post["LHREL"]))
        assert (rec[bd.REC["RAN_OCEAN"]] == 1.0) == ocean and (rec[bd.REC["RAN_OCEAN_ENERGY"]] == 1.0) == ocean
        if ocean:
            assert 150.0 < post["SST"].min() and post["SST"].max() < 340.0           # the final clamp did not act
            want = ref.ocean(lat_mesh, post["UO"], post["VO"], post["ETA"], fmt.cfl)
            got = bd.ocean_values(rec, fmt.wsum, fmt.cfl)
            assert got["eta_min"] == want["eta_min"] and got["eta_max"] == want["eta_max"]
            close(got, want, ("KE_mean", "U_max"))
            want = ref.ocean_energy(lat_mesh, land, post["QNET"], post["HICE"] > 0.0, post["SST"], prev_sst, DT, p.rho_w, p.cp_w, p.H_ocean,
                                    p.ocean_ice_qfac, polar_lat)
            got = bd.ocean_energy_values(rec, p.rho_w, p.cp_w, p.H_ocean)
            close(got, want)
            if case == "no_polar_ocean":
                assert got["Qp_mean"] == 0.0 and got["implied_p"] == 0.0 and got["resid_p"] == 0.0
            if case == "sea_ice":
                assert ((post["HICE"] > 0.0) & (land == 0)).any()
            if i == 0:
                assert got["implied"] == 0.0 and got["resid"] == 0.0
            prev_sst = post["SST"]
        else:
            assert not any(s.startswith(("[OceanE]", "[OceanDiag]")) for s in sim.budget_lines)
        dts = None if i == 0 else DT
        want = ref.water(lat_mesh, post["Q"], p.rho_a, p.h_mbl, post["HICE"], p.rho_i, post["W_LAND"], post["S_SNOW"], post["EFLUX"], post["PRECIP"],
                         post["RUNOFF"], dts, prev_total)
        got = bd.water_values(rec, fmt.wsum, dts, prev_total)
        close(got, want, [k for k in want if k != "closure_residual"])
        if i == 1:
            lim = TOL * (2.0 * (abs(want["total_reservoir_mean"]) + 1.0) / DT + abs(want["E_mean"]) + abs(want["P_mean"]) + abs(want["R_mean"]) + 3.0)
            print("  closure_residual", got["closure_residual"], want["closure_residual"], lim)
            assert abs(got["closure_residual"] - want["closure_residual"]) <= lim
        prev_total = want["total_reservoir_mean"]
        if routing:
            last = dev.route_last_event() or {"ocean_inflow_kgps": 0.0, "mass_closure_error_kg": 0.0}
            want = ref.routing(dev.route_download("FLOW"), last["ocean_inflow_kgps"], last["mass_closure_error_kg"])
            assert bd.routing_values(rec, True) == want, (bd.routing_values(rec, True), want)
            if i == 1:
                assert want["max_flow"] > 0.0 and dev.route_last_event() is not None      # the event of step 1 came first
    tags = [s.split("]")[0] + "]" for s in sim.budget_lines]
    order = [t for t in ("[EnergyDiag]", "[OceanE]", "[OceanDiag]", "[HumidityDiag]", "[WaterDiag]", "[HydroRoutingDiag]")
             if (ocean or "Ocean" not in t) and (routing or "Routing" not in t)]
    assert tags == order * 2, tags
    water = [s for s in sim.budget_lines if s.startswith("[WaterDiag]")]
    assert "residual=" not in water[0] and "residual=" in water[1]


def run6(monkeypatch, cuts, fires):
    sim = make(monkeypatch, 19, 36, fires=fires)
    recs = []
    orig = sim.dev.budget_diag_log
    sim.dev.budget_diag_log = lambda: recs.append(orig()) or recs[-1]
    for n in cuts:
        sim.run_steps(n)
    state = fetch(sim.dev, RESTART)
    state["route_buffer"] = sim.dev.route_download("BUFFER")
    return (np.concatenate(recs) if recs else None), state, sim


def test_span_invariance_and_no_perturbation(gpu, monkeypatch):
    fires = {0: 3, 2: 1, 5: 3}
    a, sa, _ = run6(monkeypatch, [6], fires)
    assert a.shape[0] == 3
    for cuts in ([1] * 6, [2, 4]):
        b, sb, _ = run6(monkeypatch, cuts, fires)
        assert a.tobytes() == b.tobytes(), cuts
        for k in sa:
            assert sa[k].tobytes() == sb[k].tobytes(), (cuts, k)
    _, off, sim = run6(monkeypatch, [6], None)
    assert sim.budget is None
    for k in sa:
        assert sa[k].tobytes() == off[k].tobytes(), k


def test_nanmax_of_flow_map(gpu, monkeypatch):
    """A NaN in the flow accumulation: np.nanmax skips it.  The model scrubs NaN out of every field it writes, so the NaN comes in
    through the plan: one land row's cell area is NaN, which makes that row's buffer, and the flow of everything downstream of it,
    NaN -- the other rows keep finite flows."""
    import budget_diag_ref as ref
    from qingdai_amd import budget_diag as bd
    sim = make(monkeypatch, 19, 36, fires={1: 1})
    dev = sim.dev
    plan = sim.routing.plan
    row = int(np.argmax((sim.land_mask == 1).sum(axis=1)))
    plan.area_row = np.array(plan.area_row, dtype=np.float64)
    plan.area_row[row] = np.nan
    dev.route_configure(plan)
    recs = []
    orig = dev.budget_diag_log
    dev.budget_diag_log = lambda: recs.append(orig()) or recs[-1]
    sim.run_steps(2)                                          # the routing event of step 1 fills the flow map
    flow = dev.route_download("FLOW")
    rec = np.concatenate(recs)[0]
    assert np.isnan(flow).any() and np.isfinite(flow).any()
    assert bd.routing_values(rec, True)["max_flow"] == ref.routing(flow, 0.0, 0.0)["max_flow"] > 0.0


def test_banded_handle_is_refused(gpu):
    import qingdai_amd as qa
    from qingdai_amd._lib import QdError
    from qingdai_amd.device import Device
    dev = Device(qa.SphericalGrid(73, 144), row0=20, n_rows=30, halo=6)
    with pytest.raises(QdError, match="whole-globe handle"):
        dev.budget_diag_configure(31, np.zeros(73, dtype=np.uint8))
    dev.close()


def test_driver_201_steps(gpu, monkeypatch, capsys):
    """The driver's own clock: 201 steps, two firings of the driver's cadence (i = 0 and 200), [OceanE] on the ocean's 200th step
    (i = 199); the second [WaterDiag] line carries the closure part, the first does not; the reference's order within a firing."""
    from qingdai_amd import budget_diag as bd
    sim = make(monkeypatch, 19, 36, env={"QD_BUDGET_DIAG": "1"})
    assert sim.enable_budget_diag() is not None
    sim.budget.out = sim.budget_lines.append
    done = 0
    while done < 201:                                         # the driver's chunks: spans are not cut at firing steps
        n = min(67, 201 - done)
        sim.run_steps(n)
        done += n
    tags = [s.split("]")[0] + "]" for s in sim.budget_lines]
    firing = ["[EnergyDiag]", "[OceanDiag]", "[HumidityDiag]", "[WaterDiag]", "[HydroRoutingDiag]"]
    assert tags == firing + ["[OceanE]"] + firing, tags
    water = [s for s in sim.budget_lines if s.startswith("[WaterDiag]")]
    assert "d/dt Σ=" not in water[0] and "d/dt Σ=" in water[1] and "residual=" in water[1]
    assert sim.budget.i == 201 and sim.budget.fmt._hydro_prev_time == 200 * DT
