"""Regenerate tests/golden/budget_diag_<case>_19x36.npz from the reference's own functions.

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR).  Each case builds a
small state by hand and calls energy.shortwave_radiation, longwave_radiation[_v2], surface_emissivity_map, boundary_layer_fluxes,
compute_energy_diagnostics, WindDrivenSlabOcean.diagnostics, hydrology.diagnose_water_closure (twice: the second call carries the
closure part) and -- for [OceanE], which the reference only prints -- two consecutive firings of WindDrivenSlabOcean.step with
QD_OCEAN_DIAG_EVERY=1 under redirect_stdout.  The golden holds the inputs, the returned numbers and the captured line text; the
ocean state behind each [OceanE] line is taken from the ocean object between the last sub-step and the polar fill by running the
step with QD_OCEAN_POLAR_FIX=0 (the line is printed before the fill either way).  Data only: no program text is stored.
"""
import argparse
import contextlib
import io
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON, DT = 19, 36, 300.0


def state(rng, ice):
    lat = np.linspace(-90.0, 90.0, NLAT)
    lon = np.linspace(0.0, 360.0, NLON)
    lon_mesh, lat_mesh = np.meshgrid(lon, lat)
    phi = np.deg2rad(lat_mesh)
    land = (rng.uniform(size=(NLAT, NLON)) < 0.3).astype(int)
    land[:, 20:30] = 0
    s = {"lat_mesh": lat_mesh, "lon_mesh": lon_mesh, "land_mask": land,
         "isr": np.maximum(0.0, 600.0 * np.cos(phi) + rng.normal(0, 20, phi.shape)), "albedo": rng.uniform(0.05, 0.7, phi.shape),
         "cloud": rng.uniform(-0.1, 1.1, phi.shape), "T_s": 262.0 + 36.0 * np.cos(phi) ** 2 + rng.normal(size=phi.shape),
         "h": 8000.0 + 300.0 * rng.normal(size=phi.shape), "u": 8.0 * np.cos(phi) + rng.normal(size=phi.shape), "v": rng.normal(size=phi.shape),
         "LH": np.abs(rng.normal(40.0, 20.0, phi.shape)),
         "h_ice": np.where((land == 0) & (np.abs(lat_mesh) > 50), 0.8, 0.0) if ice else np.zeros(phi.shape)}
    return s


def run_case(name, ref, lw_v2, ice, polar_lat):
    energy, ocean_mod, hydrology, grid_mod = ref
    rng = np.random.default_rng(sum(map(ord, "budget_diag_" + name)))
    s = state(rng, ice)
    out = dict(s)
    os.environ["QD_LW_V2"] = str(lw_v2)
    ep = energy.get_energy_params_from_env()
    # ---- [EnergyDiag] (run_simulation.py:2150-2185)
    _, SW_sfc, R = energy.shortwave_radiation(s["isr"], s["albedo"], s["cloud"], ep)
    T_a = 288.0 + (9.81 / 1004.0) * s["h"]
    if lw_v2:
        ice_frac = 1.0 - np.exp(-np.maximum(s["h_ice"], 0.0) / 0.5)
        eps = energy.surface_emissivity_map(s["land_mask"], ice_frac)
        _, LW_sfc, OLR, _, _ = energy.longwave_radiation_v2(s["T_s"], T_a, s["cloud"], eps, ep)
    else:
        _, LW_sfc, OLR, _, _ = energy.longwave_radiation(s["T_s"], T_a, s["cloud"], ep)
    SH, _ = energy.boundary_layer_fluxes(s["T_s"], T_a, s["u"], s["v"], s["land_mask"], C_H=1.5e-3, rho=1.2, c_p=1004.0, B_land=0.7, B_ocean=0.3)
    dE = energy.compute_energy_diagnostics(s["lat_mesh"], s["isr"], R, OLR, SW_sfc, LW_sfc, SH, s["LH"])
    out["energy"] = np.array([dE["TOA_net"], dE["SFC_net"], dE["ATM_net"], float(np.nanmean(s["T_s"]))])
    # ---- the ocean: two firings of step() (ocean.py:446-516), then diagnostics() (ocean.py:535-561)
    grid = grid_mod.SphericalGrid(NLAT, NLON)
    assert np.array_equal(grid.lat_mesh, s["lat_mesh"])
    os.environ.update({"QD_OCEAN_DIAG_EVERY": "1", "QD_OCEAN_POLAR_LAT": str(polar_lat), "QD_OCEAN_POLAR_FIX": "0", "QD_OCEAN_ENERGY_DIAG": "1"})
    oc = ocean_mod.WindDrivenSlabOcean(grid, s["land_mask"], 50.0, init_Ts=np.where(s["land_mask"] == 0, s["T_s"], 288.0))
    ice_mask = s["h_ice"] > 0.0
    texts = []
    for k in range(2):
        Q = rng.normal(20.0, 60.0, s["T_s"].shape)
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            oc.step(DT, s["u"], s["v"], Q_net=Q, ice_mask=ice_mask)
        line = [x for x in buf.getvalue().splitlines() if x.startswith("[OceanE]")]
        assert len(line) == 1, buf.getvalue()
        texts.append(line[0])
        out[f"oe_Q{k}"] = Q
        out[f"oe_Ts{k}"] = oc._Ts_prev_for_diag.copy()       # the SST the line was computed from
    out["oe_text"] = np.array(texts)
    od = oc.diagnostics()
    out.update(uo=oc.uo.copy(), vo=oc.vo.copy(), eta=oc.eta.copy())
    out["ocean"] = np.array([od["KE_mean"], od["U_max"], od["eta_min"], od["eta_max"], od["cfl_per_s"]])
    out["ocean_consts"] = np.array([oc.rho_w, oc.cp_w, oc.H, oc.g, oc.a, oc.dlat, oc.dlon])
    # ---- [WaterDiag] (hydrology.py:270-340): two firings 200 steps apart
    land = s["land_mask"] == 1
    keys = ("CWV_mean", "ICE_mean", "W_land_mean", "S_snow_mean", "E_mean", "P_mean", "R_mean", "total_reservoir_mean")
    prev_total = None
    for k in range(2):
        f = {"q": rng.uniform(0.0, 0.02, land.shape), "W_land": np.where(land, 40.0 * rng.random(land.shape), 0.0),
             "S_snow": np.where(land & (np.abs(s["lat_mesh"]) > 55), 60.0 * rng.random(land.shape), 0.0), "E": rng.uniform(0, 5e-5, land.shape),
             "P": rng.uniform(0, 5e-5, land.shape), "R": np.where(land, rng.uniform(0, 1e-5, land.shape), 0.0)}
        d = hydrology.diagnose_water_closure(s["lat_mesh"], f["q"], 1.2, 800.0, s["h_ice"], 917.0, f["W_land"], f["S_snow"], f["E"], f["P"], f["R"],
                                             None if k == 0 else 200 * DT, prev_total)
        for n, a in f.items():
            out[f"w_{n}{k}"] = a
        out[f"water{k}"] = np.array([d[x] for x in keys] + ([d["d/dt_total_mean"], d["closure_residual"]] if k else []))
        prev_total = d["total_reservoir_mean"]
    meta = {"case": name, "nlat": NLAT, "nlon": NLON, "dt": DT, "lw_v2": lw_v2, "ice": ice, "polar_lat": polar_lat, "water_keys": list(keys)}
    np.savez_compressed(os.path.join(OUT, f"budget_diag_{name}_{NLAT}x{NLON}.npz"), meta=json.dumps(meta), **out)
    print(name, out["energy"], texts, out["ocean"], out["water1"])


CASES = {"default": (1, False, 60.0), "lw_v1": (0, False, 60.0), "sea_ice": (1, True, 60.0), "no_polar": (1, False, 95.0)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    sys.path.insert(0, os.path.abspath(a.reference))
    from pygcm import energy, hydrology, ocean as ocean_mod, grid as grid_mod
    for name in a.cases:
        run_case(name, (energy, ocean_mod, hydrology, grid_mod), *CASES[name])


if __name__ == "__main__":
    main()
