"""NumPy restatement of the reference driver's periodic budget diagnostics, written for the tests: what scripts/run_simulation.py
(2148-2188, 2263-2287, 2349-2398), pygcm/ocean.py (446-516, 535-561) and pygcm/hydrology.py (263-340) compute on whole arrays, as
plain functions of the fields.  tests/test_budget_diag_cpu.py holds it against the goldens written from the reference's own
functions; tests/test_gpu_budget_diag.py holds the device records against it at shapes the goldens do not cover."""
import numpy as np

from qd_oracle import column as col


def weights(lat_mesh):
    return np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)


def wmean(x, w):
    return float(np.sum(x * w) / (np.sum(w) + 1e-15))


def energy(lat_mesh, isr, albedo, cloud, Ts, h, u, v, land_mask, h_ice, LH, P):
    """run_simulation.py:2150-2185 with the oracle's flux functions (P: qd_oracle parameters)."""
    T_a = 288.0 + (9.81 / 1004.0) * h
    _, SW_sfc, R = col.shortwave(isr, albedo, cloud, P)
    if int(P.lw_v2):
        ice_frac = 1.0 - np.exp(-np.maximum(h_ice, 0.0) / 0.5)
        eps_sfc = col.surface_emissivity_map(land_mask, ice_frac, P)
        _, LW_sfc, OLR, _, _ = col.longwave_v2(Ts, T_a, cloud, eps_sfc, P)
    else:
        _, LW_sfc, OLR, _, _ = col.longwave_v1(Ts, T_a, cloud, P)
    SH = col.sensible_heat(Ts, T_a, u, v, P)
    w = weights(lat_mesh)
    TOA = isr - R - OLR
    SFC = SW_sfc - LW_sfc - SH - LH
    return {"TOA_net": wmean(TOA, w), "SFC_net": wmean(SFC, w), "ATM_net": wmean(TOA - SFC, w), "Ts_mean": float(np.nanmean(Ts))}


def ocean_energy(lat_mesh, land_mask, Q_net, ice_mask, Ts, Ts_prev, dt, rho_w, cp_w, H, ice_qfac=0.2, polar_lat=60.0):
    """ocean.py:453-510.  Ts_prev None: the first firing (no snapshot yet)."""
    lat_rad = np.deg2rad(lat_mesh)
    w = np.maximum(np.cos(lat_rad), 0.0)
    ocean = land_mask == 0
    wsum_ocean = float(np.sum(w * ocean) + 1e-15)

    def eff(mask):
        e = np.where(mask & (~ice_mask), Q_net, 0.0)
        if ice_qfac > 0.0:
            e = e + np.where(mask & ice_mask, ice_qfac * Q_net, 0.0)
        return e
    Q_mean = float(np.sum(eff(ocean) * w) / wsum_ocean)
    if Ts_prev is None:
        implied = resid = 0.0
    else:
        dT = (Ts - Ts_prev) / max(1e-12, dt)
        implied = float(rho_w * cp_w * H * float(np.sum(dT * w * ocean) / wsum_ocean))
        resid = implied - Q_mean
    polar = (np.abs(np.rad2deg(lat_rad)) >= float(polar_lat)) & ocean
    if np.any(polar):
        wsum_p = float(np.sum(w * polar) + 1e-15)
        Qp = float(np.sum(eff(polar) * w) / wsum_p)
        dTp = (Ts - (Ts if Ts_prev is None else Ts_prev)) / max(1e-12, dt)
        implied_p = float(rho_w * cp_w * H * float(np.sum(dTp * w * polar) / wsum_p))
        resid_p = implied_p - Qp
    else:
        Qp = implied_p = resid_p = 0.0
    return {"Q_mean": Q_mean, "implied": implied, "resid": resid, "Qp_mean": Qp, "implied_p": implied_p, "resid_p": resid_p}


def ocean(lat_mesh, uo, vo, eta, cfl):
    """ocean.py:539-561"""
    w = weights(lat_mesh)
    return {"KE_mean": wmean(0.5 * (uo ** 2 + vo ** 2), w), "U_max": float(np.max(np.sqrt(uo ** 2 + vo ** 2))),
            "eta_min": float(np.min(eta)), "eta_max": float(np.max(eta)), "cfl_per_s": cfl}


def humidity(lat_mesh, E, P_cond, LH, LH_release):
    w = weights(lat_mesh)
    return {"E_mean": wmean(E, w), "Pcond_mean": wmean(P_cond, w), "LH_mean": wmean(LH, w), "LHrel_mean": wmean(LH_release, w)}


def water(lat_mesh, q, rho_a, h_mbl, h_ice, rho_i, W_land, S_snow, E, P, R, dt_since_prev=None, prev_total=None):
    """hydrology.py:304-340"""
    w = weights(lat_mesh)
    m = {"CWV_mean": wmean(float(rho_a) * float(h_mbl) * q, w), "ICE_mean": wmean(float(rho_i) * h_ice, w), "W_land_mean": wmean(W_land, w),
         "S_snow_mean": wmean(S_snow, w), "E_mean": wmean(E, w), "P_mean": wmean(P, w), "R_mean": wmean(R, w)}
    total = m["CWV_mean"] + m["ICE_mean"] + m["W_land_mean"] + m["S_snow_mean"]
    m["total_reservoir_mean"] = total
    if dt_since_prev is not None and prev_total is not None and dt_since_prev > 0:
        m["d/dt_total_mean"] = (total - prev_total) / float(dt_since_prev)
        m["closure_residual"] = m["d/dt_total_mean"] - (m["E_mean"] - m["P_mean"] - m["R_mean"])
    return m


def routing(flow, ocean_inflow_kgps, mass_closure_error_kg):
    """run_simulation.py:2387-2391"""
    with np.errstate(all="ignore"):
        return {"ocean_inflow_kgps": float(ocean_inflow_kgps), "mass_closure_error_kg": float(mass_closure_error_kg),
                "max_flow": float(np.nanmax(flow))}
