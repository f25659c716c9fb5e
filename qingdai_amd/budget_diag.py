"""
qingdai_amd/budget_diag.py -- the reference driver's periodic budget lines (QD_BUDGET_DIAG=1), host side of csrc/qd_budget_diag.hip.

The reference prints [EnergyDiag], [OceanDiag], [HumidityDiag], [WaterDiag] and [HydroRoutingDiag] on steps with run-local index
i % 200 == 0 (scripts/run_simulation.py:2148-2188, 2263-2287, 2349-2398) and its ocean prints [OceanE] whenever its own step count
is a multiple of QD_OCEAN_DIAG_EVERY (pygcm/ocean.py:446-516).  Here a span of the device loop runs straight across such steps: this
class names them in a schedule before the span (bit0 = the driver's cadence, bit1 = the ocean's), the device reduces at the
reference's positions inside the step and leaves one record per scheduled step, and after the span the records become the
reference's lines -- the last scalar operations and the f-strings below are the reference's own.

Nothing here touches the device at import; the formatting and the schedule are plain Python / NumPy (tests/test_budget_diag_cpu.py).
"""
from __future__ import annotations

import numpy as np

from ._lib import BUDGET_LOG_W as LOG_W, C

EVERY = 200                      # run_simulation.py:2150, 2264, 2275, 2350: `i % 200 == 0`
LINE_ENERGY, LINE_OCEAN, LINE_OCEAN_ENERGY, LINE_HUMIDITY, LINE_WATER = (
    C["QD_BD_LINE_" + n] for n in ("ENERGY", "OCEAN", "OCEAN_ENERGY", "HUMIDITY", "WATER"))
FIRE_MAIN, FIRE_OCEAN_E = 1, 2

# record slots (include/qingdai_hip.h, QD_BUDGET_LOG_W doubles)
REC = {k: i for i, k in enumerate(
    ("E_TOA", "E_SFC", "E_ATM", "E_TS_SUM", "E_TS_CNT",
     "OE_Q", "OE_DT", "OE_W", "OE_QP", "OE_DTP", "OE_WP", "OE_NP", "OE_PREV",
     "O_KE", "O_UMAX", "O_ETA_MIN", "O_ETA_MAX",
     "H_E", "H_PCOND", "H_LH", "H_LHREL",
     "W_E", "W_P", "W_R", "W_CWV", "W_ICE", "W_WLAND", "W_SSNOW",
     "R_FLOW", "R_INFLOW", "R_ERR"))}
REC.update({"RAN_ENERGY": 32, "RAN_OCEAN_ENERGY": 33, "RAN_OCEAN": 34, "RAN_HUMIDITY": 35, "RAN_WATER": 36, "FIRE": 37})


def read_env(env):
    """The reference's own variables with the reference's defaults -> dict.  `enabled` is this project's switch (default 0)."""
    def _i(name, dflt):
        return int(env.get(name, str(dflt)))
    every = _i("QD_OCEAN_DIAG_EVERY", 200)
    if every <= 0:                                              # ocean.py:449-451
        every = 200
    lines = ((LINE_ENERGY if _i("QD_ENERGY_DIAG", 1) == 1 else 0) | (LINE_OCEAN if _i("QD_OCEAN_DIAG", 1) == 1 else 0) |
             (LINE_OCEAN_ENERGY if _i("QD_OCEAN_ENERGY_DIAG", 1) == 1 else 0) | (LINE_HUMIDITY if _i("QD_HUMIDITY_DIAG", 1) == 1 else 0) |
             (LINE_WATER if _i("QD_WATER_DIAG", 1) == 1 else 0))
    return {"enabled": _i("QD_BUDGET_DIAG", 0) == 1, "lines": lines, "ocean_every": every,
            "polar_lat": float(env.get("QD_OCEAN_POLAR_LAT", "60.0")),
            "polar_label": int(float(env.get("QD_OCEAN_POLAR_LAT", "60")))}        # ocean.py:489, 513


def schedule(i0, n, ocean_step0=None, ocean_every=200):
    """The next n steps, the first with run-local index i0 -> int32 [n]: bit0 where i % 200 == 0, bit1 where the ocean's step
    count -- ocean_step0 before the span, raised at the top of each ocean step (ocean.py:281) -- is a multiple of ocean_every.
    ocean_step0 None: no ocean, no bit1."""
    i = i0 + np.arange(int(n), dtype=np.int64)
    fire = np.where(i % EVERY == 0, FIRE_MAIN, 0).astype(np.int32)
    if ocean_step0 is not None:
        fire |= np.where((int(ocean_step0) + 1 + np.arange(int(n), dtype=np.int64)) % int(ocean_every) == 0, FIRE_OCEAN_E, 0).astype(np.int32)
    return fire


def polar_rows(lat_deg_rows, polar_lat):
    """ocean.py:488-489 per row: abs(rad2deg(deg2rad(lat))) >= polar_lat -> uint8 [n_lat]."""
    lat = np.abs(np.rad2deg(np.deg2rad(np.asarray(lat_deg_rows, dtype=np.float64))))
    return (lat >= float(polar_lat)).astype(np.uint8)


def weight_sum(lat_mesh):
    """np.sum(max(cos(lat), 0)) over the mesh, as energy.py:520-522, ocean.py:539-540 and hydrology.py:263-268 form it."""
    return float(np.sum(np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)))


def cfl_per_s(g, H, a, dlat_rad, dlon_rad):
    """ocean.py:547-553 (coslat is floored at 0.5 there, ocean.py:82)."""
    c = np.sqrt(g * H)
    dx_min = min(a * dlat_rad, a * dlon_rad * max(1e-3, 0.5))
    return float(c / max(1e-12, dx_min))


# ---------------------------------------------------------------- record -> the reference's numbers
def energy_values(rec, wsum):
    """energy.py:524-530 and the <Ts> fall-back np.nanmean(T_s) of run_simulation.py:2185."""
    d = wsum + 1e-15
    cnt = rec[REC["E_TS_CNT"]]
    return {"TOA_net": float(rec[REC["E_TOA"]] / d), "SFC_net": float(rec[REC["E_SFC"]] / d), "ATM_net": float(rec[REC["E_ATM"]] / d),
            "Ts_mean": float(rec[REC["E_TS_SUM"]] / cnt) if cnt > 0 else float("nan")}


def ocean_energy_values(rec, rho_w, cp_w, H):
    """ocean.py:453-510 from the sums.  Before the first snapshot implied = resid = 0 and the polar dT is 0."""
    wsum_ocean = float(rec[REC["OE_W"]] + 1e-15)
    Q_mean = float(rec[REC["OE_Q"]] / wsum_ocean)
    if rec[REC["OE_PREV"]] != 0.0:
        dT_mean = float(rec[REC["OE_DT"]] / wsum_ocean)
        implied = float(rho_w * cp_w * H * dT_mean)
        resid = implied - Q_mean
    else:
        implied = 0.0
        resid = 0.0
    if rec[REC["OE_NP"]] > 0:
        wsum_p = float(rec[REC["OE_WP"]] + 1e-15)
        Qp_mean = float(rec[REC["OE_QP"]] / wsum_p)
        dTp_mean = float(rec[REC["OE_DTP"]] / wsum_p)
        implied_p = float(rho_w * cp_w * H * dTp_mean)
        resid_p = implied_p - Qp_mean
    else:
        Qp_mean = implied_p = resid_p = 0.0
    return {"Q_mean": Q_mean, "implied": implied, "resid": resid, "Qp_mean": Qp_mean, "implied_p": implied_p, "resid_p": resid_p}


def ocean_values(rec, wsum, cfl):
    """ocean.py:539-561"""
    return {"KE_mean": float(rec[REC["O_KE"]] / (wsum + 1e-15)), "U_max": float(rec[REC["O_UMAX"]]),
            "eta_min": float(rec[REC["O_ETA_MIN"]]), "eta_max": float(rec[REC["O_ETA_MAX"]]), "cfl_per_s": cfl}


def humidity_values(rec, wsum):
    """run_simulation.py:2276-2283"""
    d = wsum + 1e-15
    return {k: float(rec[REC[s]] / d) for k, s in (("E_mean", "H_E"), ("Pcond_mean", "H_PCOND"), ("LH_mean", "H_LH"), ("LHrel_mean", "H_LHREL"))}


def water_values(rec, wsum, dt_since_prev=None, prev_total=None):
    """hydrology.py:312-340"""
    d = wsum + 1e-15
    m = {k: float(rec[REC[s]] / d) for k, s in (("CWV_mean", "W_CWV"), ("ICE_mean", "W_ICE"), ("W_land_mean", "W_WLAND"),
                                                  ("S_snow_mean", "W_SSNOW"), ("E_mean", "W_E"), ("P_mean", "W_P"), ("R_mean", "W_R"))}
    total_now = m["CWV_mean"] + m["ICE_mean"] + m["W_land_mean"] + m["S_snow_mean"]
    m["total_reservoir_mean"] = total_now
    if (dt_since_prev is not None) and (prev_total is not None) and dt_since_prev > 0:
        ddt_total = (total_now - prev_total) / float(dt_since_prev)
        m["d/dt_total_mean"] = ddt_total
        m["closure_residual"] = ddt_total - (m["E_mean"] - m["P_mean"] - m["R_mean"])
    return m


def routing_values(rec, routed):
    """run_simulation.py:2387-2391.  routed False: no flow map took part (the slot holds 0); an all-NaN map leaves -inf -> NaN."""
    f = float(rec[REC["R_FLOW"]]) if routed else 0.0
    return {"ocean_inflow_kgps": float(rec[REC["R_INFLOW"]]), "mass_closure_error_kg": float(rec[REC["R_ERR"]]),
            "max_flow": float("nan") if f == float("-inf") else f}


# ---------------------------------------------------------------- the reference's f-strings
def energy_line(diagE):
    return (f"[EnergyDiag] TOA_net={diagE['TOA_net']:.2f} W/m^2 | "
            f"SFC_net={diagE['SFC_net']:.2f} | ATM_net={diagE['ATM_net']:.2f} | "
            f"<Ts>={diagE['Ts_mean']:.2f} K")


def ocean_energy_line(v, polar_label=60):
    return (f"[OceanE] ⟨Q_net⟩={v['Q_mean']:+.2f} W/m^2 | implied={v['implied']:+.2f} | resid={v['resid']:+.2f}  "
            f"|| Polar(|lat|>={polar_label}°): "
            f"⟨Q⟩={v['Qp_mean']:+.2f}, implied={v['implied_p']:+.2f}, resid={v['resid_p']:+.2f}")


def ocean_line(od):
    return (f"[OceanDiag] KE_mean={od['KE_mean']:.3e} m2/s2 | Umax={od['U_max']:.2f} m/s | "
            f"eta[{od['eta_min']:.3f},{od['eta_max']:.3f}] m | cfl/sqrt(gH)/dx={od['cfl_per_s']:.3e} s^-1")


def humidity_line(v):
    return (f"[HumidityDiag] ⟨E⟩={v['E_mean']:.3e} kg/m^2/s | ⟨P_cond⟩={v['Pcond_mean']:.3e} kg/m^2/s | "
            f"⟨LH⟩={v['LH_mean']:.2f} W/m^2 | ⟨LH_release⟩={v['LHrel_mean']:.2f} W/m^2")


def water_line(diag_h2o):
    msg = (f"[WaterDiag] ⟨E⟩={diag_h2o['E_mean']:.3e} kg/m^2/s | "
           f"⟨P⟩={diag_h2o['P_mean']:.3e} | ⟨R⟩={diag_h2o['R_mean']:.3e} | "
           f"⟨CWV⟩={diag_h2o['CWV_mean']:.3e} kg/m^2 | ⟨ICE⟩={diag_h2o['ICE_mean']:.3e} | "
           f"⟨W_land⟩={diag_h2o['W_land_mean']:.3e} | ⟨S_snow⟩={diag_h2o['S_snow_mean']:.3e}")
    if "closure_residual" in diag_h2o and "d/dt_total_mean" in diag_h2o:
        msg += (f" | d/dt Σ={diag_h2o['d/dt_total_mean']:.3e} vs (E−P−R) -> "
                f"residual={diag_h2o['closure_residual']:.3e}")
    return msg


def routing_line(rd):
    return (f"[HydroRoutingDiag] ocean_inflow={rd['ocean_inflow_kgps']:.3e} kg/s | "
            f"mass_error={rd['mass_closure_error_kg']:.3e} kg | "
            f"max_flow={rd['max_flow']:.3e} kg/s")


class BudgetFormatter:
    """Records -> lines, in the reference's order within a step; carries the [WaterDiag] closure state (_hydro_prev_total /
    _hydro_prev_time, run_simulation.py:2352-2398) from firing to firing, across chunks."""

    def __init__(self, wsum, cfl, rho_w, cp_w, H_ocean, polar_label=60):
        self.wsum, self.cfl = float(wsum), float(cfl)
        self.rho_w, self.cp_w, self.H_ocean = float(rho_w), float(cp_w), float(H_ocean)
        self.polar_label = int(polar_label)
        self._hydro_prev_total = None
        self._hydro_prev_time = None

    def lines(self, rec, i, dt, routed=False):
        """One record of the step with run-local index i -> its lines."""
        out = []
        if rec[REC["RAN_ENERGY"]]:
            out.append(energy_line(energy_values(rec, self.wsum)))
        if rec[REC["RAN_OCEAN_ENERGY"]]:
            out.append(ocean_energy_line(ocean_energy_values(rec, self.rho_w, self.cp_w, self.H_ocean), self.polar_label))
        if rec[REC["RAN_OCEAN"]]:
            out.append(ocean_line(ocean_values(rec, self.wsum, self.cfl)))
        if rec[REC["RAN_HUMIDITY"]]:
            out.append(humidity_line(humidity_values(rec, self.wsum)))
        if rec[REC["RAN_WATER"]]:
            t_now = (i * dt)
            dt_since_prev = None if self._hydro_prev_time is None else (t_now - self._hydro_prev_time)
            diag_h2o = water_values(rec, self.wsum, dt_since_prev, self._hydro_prev_total)
            out.append(water_line(diag_h2o))
            if routed:
                out.append(routing_line(routing_values(rec, True)))
            self._hydro_prev_total = diag_h2o["total_reservoir_mean"]
            self._hydro_prev_time = t_now
        return out


class BudgetDiag:
    """The lane's participant in Device.step_n (like RiverRouting, PhytoDaily, PopulationDaily): the run-local step index is its
    clock, span_schedule uploads the span's schedule, take() turns the drained records into lines."""

    def __init__(self, dev, grid, env=None, with_ocean=True, routed=False, out=print):
        import os
        cfg = read_env(os.environ if env is None else env)
        self.dev, self.cfg, self.out = dev, cfg, out
        self.with_ocean, self.routed = bool(with_ocean), bool(routed)
        self.i = 0                                   # run-local index of the next step (enumerate(time_steps))
        self._pending = []                           # (i, fire) of the scheduled steps whose records are still on the device
        p = dev.params
        lat_rows = np.asarray(grid.lat_mesh)[:, 0]
        dev.budget_diag_configure(cfg["lines"], polar_rows(lat_rows, cfg["polar_lat"]))
        self.fmt = BudgetFormatter(weight_sum(grid.lat_mesh), cfl_per_s(p.g_ocean, p.H_ocean, p.a, grid.dlat_rad, grid.dlon_rad),
                                   p.rho_w, p.cp_w, p.H_ocean, cfg["polar_label"])

    # -- the span protocol of Device.step_n
    def span_clock(self):
        return (self.i, list(self._pending))

    def span_restore(self, clock):
        self.i, self._pending = clock[0], list(clock[1])

    def span_schedule(self, t0, dt, n):
        ocean0 = self.dev.counters()[1] if self.with_ocean else None
        fire = schedule(self.i, n, ocean0, self.cfg["ocean_every"])
        self.dev.budget_diag_schedule(fire)
        return [(self.i + int(s), int(fire[s])) for s in np.flatnonzero(fire)], int(n)

    def _fired(self, k):
        fired, n = k
        self._pending.extend(fired)
        self.i += n

    def span_deliver(self, dt):
        self.take(self.dev.budget_diag_log(), dt)      # the span's budget lines, oldest first

    def take(self, records, dt):
        """The drained records, oldest first -> printed lines (returned too)."""
        if len(records) != len(self._pending):
            raise RuntimeError(f"budget diagnostics: {len(records)} records for {len(self._pending)} scheduled steps")
        lines = []
        for rec, (i, _fire) in zip(records, self._pending):
            lines += self.fmt.lines(rec, i, dt, routed=self.routed)
        self._pending = []
        for s in lines:
            self.out(s)
        return lines


def from_env(dev, grid, env, with_ocean=True, routed=False):
    """QD_BUDGET_DIAG (default 0) -> a BudgetDiag on this handle, or None: at 0 nothing is configured, allocated or launched."""
    if not read_env(env)["enabled"]:
        return None
    return BudgetDiag(dev, grid, env, with_ocean=with_ocean, routed=routed)
