"""CPU: the host side of the periodic budget diagnostics (qingdai_amd/budget_diag.py) and the tests' restatement
(tests/budget_diag_ref.py) against tests/golden/budget_diag_*_19x36.npz, which scripts/gen_golden_budget_diag.py wrote from the
reference's own functions: every stored number is reproduced, and the [OceanE] lines -- captured from the reference's stdout, two
consecutive firings -- are reproduced character for character from a record of NumPy sums laid out as the device lays it out."""
import glob
import json
import os
import re

import numpy as np
import pytest

import budget_diag_ref as ref
from qingdai_amd import budget_diag as bd

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "budget_diag_*_19x36.npz")))


def load(path):
    d = np.load(path)
    return json.loads(str(d["meta"])), d


def near(a, b, tol=1e-13):
    return abs(a - b) <= tol * (abs(b) + 1.0)


def ocean_energy_record(d, k, polar_lat, ice_qfac=0.2):
    """The sums the device leaves for firing k, formed with NumPy in the reference's order."""
    w = ref.weights(d["lat_mesh"])
    ocean = d["land_mask"] == 0
    ice = d["h_ice"] > 0.0
    Q, Ts = d[f"oe_Q{k}"], d[f"oe_Ts{k}"]
    eff = np.where(ocean & ~ice, Q, 0.0) + np.where(ocean & ice, ice_qfac * Q, 0.0)
    dT = (Ts - d["oe_Ts0"]) / 300.0 if k else np.zeros_like(Ts)
    polar = bd.polar_rows(d["lat_mesh"][:, 0], polar_lat).astype(bool)[:, None] & ocean
    rec = np.zeros(bd.LOG_W)
    for name, v in (("OE_Q", np.sum(eff * w)), ("OE_DT", np.sum(dT * w * ocean)), ("OE_W", np.sum(w * ocean)), ("OE_QP", np.sum((eff * w)[polar])),
                    ("OE_DTP", np.sum(dT * w * polar)), ("OE_WP", np.sum(w * polar)), ("OE_NP", float(polar.sum())), ("OE_PREV", float(k > 0))):
        rec[bd.REC[name]] = v
    return rec


def test_goldens_exist():
    assert len(GOLDENS) == 4, GOLDENS


@pytest.mark.parametrize("path", GOLDENS, ids=[os.path.basename(p)[12:-10] for p in GOLDENS])
def test_restatement_reproduces_the_reference(path):
    import qd_oracle as qo
    meta, d = load(path)
    P = qo.defaults(lw_v2=meta["lw_v2"])
    e = ref.energy(d["lat_mesh"], d["isr"], d["albedo"], d["cloud"], d["T_s"], d["h"], d["u"], d["v"], d["land_mask"], d["h_ice"], d["LH"], P)
    for k, want in zip(("TOA_net", "SFC_net", "ATM_net", "Ts_mean"), d["energy"]):
        assert near(e[k], want), (k, e[k], want)
    rho_w, cp_w, H, g, a, dlat, dlon = d["ocean_consts"]
    o = ref.ocean(d["lat_mesh"], d["uo"], d["vo"], d["eta"], bd.cfl_per_s(g, H, a, dlat, dlon))
    for k, want in zip(("KE_mean", "U_max", "eta_min", "eta_max", "cfl_per_s"), d["ocean"]):
        assert (o[k] == want) if k.startswith("eta") else near(o[k], want), (k, o[k], want)
    prev = None
    for k in range(2):
        w = ref.water(d["lat_mesh"], d[f"w_q{k}"], 1.2, 800.0, d["h_ice"], 917.0, d[f"w_W_land{k}"], d[f"w_S_snow{k}"], d[f"w_E{k}"], d[f"w_P{k}"],
                      d[f"w_R{k}"], None if k == 0 else 200 * 300.0, prev)
        keys = meta["water_keys"] + (["d/dt_total_mean", "closure_residual"] if k else [])
        assert ("closure_residual" in w) == bool(k)
        for name, want in zip(keys, d[f"water{k}"]):
            assert near(w[name], want), (name, w[name], want)
        prev = w["total_reservoir_mean"]
    # [OceanE]: the restatement's numbers give the captured text, and so does the host formatter from a record of sums
    ice = d["h_ice"] > 0.0
    for k in range(2):
        v = ref.ocean_energy(d["lat_mesh"], d["land_mask"], d[f"oe_Q{k}"], ice, d[f"oe_Ts{k}"], d["oe_Ts0"] if k else None, 300.0, rho_w, cp_w, H,
                             0.2, meta["polar_lat"])
        label = int(float(str(meta["polar_lat"])))
        assert bd.ocean_energy_line(v, label) == str(d["oe_text"][k])
        rec = ocean_energy_record(d, k, meta["polar_lat"])
        assert bd.ocean_energy_line(bd.ocean_energy_values(rec, rho_w, cp_w, H), label) == str(d["oe_text"][k])
    if meta["polar_lat"] > 90:
        assert "⟨Q⟩=+0.00, implied=+0.00, resid=+0.00" in str(d["oe_text"][1])
    assert "implied=+0.00 | resid=+0.00 " in str(d["oe_text"][0])


def test_lines_from_a_record():
    """The formatter on a hand-made record: the reference's order within a step, the closure part only from the second firing on,
    its state carried over."""
    _, d = load(GOLDENS[0])
    wsum = bd.weight_sum(d["lat_mesh"])
    w = ref.weights(d["lat_mesh"])
    fmt = bd.BudgetFormatter(wsum, 3.87e-5, 1000.0, 4200.0, 50.0)
    rec = np.zeros(bd.LOG_W)
    for k in ("RAN_ENERGY", "RAN_OCEAN_ENERGY", "RAN_OCEAN", "RAN_HUMIDITY", "RAN_WATER"):
        rec[bd.REC[k]] = 1.0
    rec[bd.REC["E_TS_SUM"]], rec[bd.REC["E_TS_CNT"]] = 288.0 * 5, 5
    rec[bd.REC["OE_W"]] = 1.0
    for name, f in (("W_CWV", 1.2 * 800.0 * d["w_q0"]), ("W_WLAND", d["w_W_land0"]), ("W_SSNOW", d["w_S_snow0"]), ("W_E", d["w_E0"])):
        rec[bd.REC[name]] = np.sum(f * w)
    first = fmt.lines(rec, 0, 300.0, routed=True)
    tags = [s.split("]")[0] + "]" for s in first]
    assert tags == ["[EnergyDiag]", "[OceanE]", "[OceanDiag]", "[HumidityDiag]", "[WaterDiag]", "[HydroRoutingDiag]"]
    assert first[0] == "[EnergyDiag] TOA_net=0.00 W/m^2 | SFC_net=0.00 | ATM_net=0.00 | <Ts>=288.00 K"
    assert "residual=" not in first[4] and fmt._hydro_prev_time == 0.0
    assert near(fmt._hydro_prev_total, d["water0"][7] - d["water0"][1])          # no ice term in this record
    rec[bd.REC["W_WLAND"]] *= 1.5
    second = fmt.lines(rec, 200, 300.0, routed=False)
    assert [s.split("]")[0] for s in second][-1] == "[WaterDiag" and fmt._hydro_prev_time == 60000.0
    m = re.search(r"d/dt Σ=(\S+) vs \(E−P−R\) -> residual=(\S+)$", second[-1])
    assert m and float(m.group(1)) > 0.0
    assert second[-1].startswith("[WaterDiag] ⟨E⟩=") and " | ⟨P⟩=0.000e+00 | ⟨R⟩=0.000e+00 | ⟨CWV⟩=" in second[-1]
    assert fmt.lines(np.zeros(bd.LOG_W), 7, 300.0) == []


def test_schedule():
    f = bd.schedule(0, 401)
    assert list(np.flatnonzero(f)) == [0, 200, 400] and set(f[f != 0]) == {bd.FIRE_MAIN}
    # run-local origin: a run that starts from a restart still fires on ITS step 0; chunks continue the count
    cut = np.concatenate([bd.schedule(0, 150), bd.schedule(150, 100), bd.schedule(250, 151)])
    assert np.array_equal(cut, f)
    # the ocean's own count (raised at the top of its step): step counts 200, 400 are the run's i = 199, 399 from a fresh ocean
    o = bd.schedule(0, 401, ocean_step0=0, ocean_every=200)
    assert list(np.flatnonzero(o & bd.FIRE_OCEAN_E)) == [199, 399] and list(np.flatnonzero(o & bd.FIRE_MAIN)) == [0, 200, 400]
    o = bd.schedule(5, 10, ocean_step0=57, ocean_every=3)            # a restored counter: 58, 59, 60 -> the third step fires
    assert list(np.flatnonzero(o & bd.FIRE_OCEAN_E)) == [2, 5, 8]
    both = bd.schedule(199, 2, ocean_step0=199, ocean_every=200)
    assert list(both) == [bd.FIRE_OCEAN_E, bd.FIRE_MAIN]
    assert bd.schedule(0, 1, ocean_step0=199, ocean_every=200)[0] == 3
    # across a chunk boundary
    a = np.concatenate([bd.schedule(190, 9, 190, 200), bd.schedule(199, 12, 199, 200)])
    assert np.array_equal(a, bd.schedule(190, 21, 190, 200))


def test_env_defaults_and_switch():
    c = bd.read_env({})
    assert c == {"enabled": False, "lines": 31, "ocean_every": 200, "polar_lat": 60.0, "polar_label": 60}
    assert bd.from_env(None, None, {}) is None and bd.from_env(None, None, {"QD_BUDGET_DIAG": "0"}) is None     # switch 0: no lane
    assert bd.read_env({"QD_BUDGET_DIAG": "1"})["enabled"]
    for name, bit in (("QD_ENERGY_DIAG", bd.LINE_ENERGY), ("QD_OCEAN_DIAG", bd.LINE_OCEAN), ("QD_OCEAN_ENERGY_DIAG", bd.LINE_OCEAN_ENERGY),
                      ("QD_HUMIDITY_DIAG", bd.LINE_HUMIDITY), ("QD_WATER_DIAG", bd.LINE_WATER)):
        assert bd.read_env({name: "0"})["lines"] == 31 & ~bit and bd.read_env({name: "1"})["lines"] == 31
    assert bd.read_env({"QD_OCEAN_DIAG_EVERY": "0"})["ocean_every"] == 200 and bd.read_env({"QD_OCEAN_DIAG_EVERY": "-5"})["ocean_every"] == 200
    assert bd.read_env({"QD_OCEAN_DIAG_EVERY": "50"})["ocean_every"] == 50
    c = bd.read_env({"QD_OCEAN_POLAR_LAT": "66.5"})
    assert c["polar_lat"] == 66.5 and c["polar_label"] == 66


def test_simulation_without_the_switch_creates_no_lane():
    from qingdai_amd.driver import Simulation

    class Dev:
        def __getattr__(self, name):
            raise AssertionError(f"switch 0 touched the device: {name}")
    sim = object.__new__(Simulation)
    sim.dev, sim.grid, sim.ocean = Dev(), None, None
    assert sim.enable_budget_diag({}) is None and sim.budget is None


def test_abi_surface():
    from qingdai_amd import _lib
    assert _lib.BUDGET_LOG_W == bd.LOG_W == _lib.C["QD_BUDGET_LOG_W"]           # the header's own value: tests/test_abi_cpu.py
    assert (bd.LINE_ENERGY, bd.LINE_OCEAN, bd.LINE_OCEAN_ENERGY, bd.LINE_HUMIDITY, bd.LINE_WATER) == (1, 2, 4, 8, 16)
    assert max(bd.REC.values()) < bd.LOG_W and len(set(bd.REC.values())) == len(bd.REC)
    assert "budget" not in " ".join(_lib.STEP_BITS)          # no flag bit: a schedule turns the lane on
