"""
qingdai_amd/phyto.py -- transport of the phytoplankton tracers by the ocean currents
(pygcm/ecology/phyto.py:496-547) on the MI355X library.

`PhytoManager.advect_diffuse` reuses the ocean's two operators per species -- the semi-Lagrangian gather
and the spherical Laplacian, both on the ocean cos floor max(cos, 0.5).

Two forms:
  * `PhytoTracers` -- the tracers RESIDENT on the device (qd_phyto_*, csrc/qd_phyto.hip): all species in three launches per step,
    inside the resident loop of qd_step_n (flags bit6) on the currents the ocean step has just written, the way the reference
    driver calls it at scripts/run_simulation.py:2254-2258.  `driver.Simulation` creates one under QD_PHYTO_ENABLE /
    QD_PHYTO_ADVECTION (both default 1, run_simulation.py:1347,1351).
  * `advect_diffuse(dev, C_s, uo, vo, ...)` -- the operator-seam form for a host ecology that owns the [S, n_lat, n_lon] array:
    `qd_op_advect` + `qd_op_laplacian` (cos kind 1) per species, blend / clip / land mask / polar means in NumPy.
  * `PhytoDaily` -- PhytoManager.step_daily (phyto.py:339-435) on the same resident tracers (qd_phyto_daily_*,
    csrc/qd_phyto_daily.hip): growth, the nutrient pool N, Kd(490) and the ocean-colour albedo in one launch per planet-day, inside
    qd_step_n (flags bit8) where the driver calls it (run_simulation.py:2051-2061), or stand-alone.  The driver creates one under
    QD_PHYTO_ENABLE=1 and QD_PHYTO_DAILY=1.
Genes and plankton.json stay outside this path.
"""
from __future__ import annotations

import os

import numpy as np


def _env_list(name):
    v = os.getenv(name)
    if not v:
        return []
    try:
        return [float(x) for x in v.replace(";", ",").split(",") if x.strip()]
    except ValueError:
        return []


class PhytoTracers:
    """The prognostic part of the reference's PhytoManager that the per-step path touches: C_phyto_s [S, n_lat, n_lon] (mg Chl / m^3),
    initialised like phyto.py:152-158,253-270 (S = QD_PHYTO_NSPECIES (10), equal or QD_PHYTO_INIT_FRAC fractions of QD_PHYTO_CHL0
    (0.05) over the ocean, 0 on land), K_h = QD_PHYTO_KH | QD_KH_OCEAN (5e3, phyto.py:123), alpha = QD_PHYTO_ADV_ALPHA (0.7).
    The array lives on the device; `C_phyto_s` downloads / uploads it."""

    def __init__(self, grid, land_mask, dev=None):
        self.grid = grid
        self.land_mask = np.asarray(land_mask)
        self.ocean_mask = (self.land_mask == 0)
        try:
            self.S = max(1, int(os.getenv("QD_PHYTO_NSPECIES", "10")))
        except ValueError:
            self.S = 10
        self.K_h = float(os.getenv("QD_PHYTO_KH", os.getenv("QD_KH_OCEAN", "5.0e3")))
        self.adv_alpha = float(os.getenv("QD_PHYTO_ADV_ALPHA", "0.7"))
        self.chl0 = float(os.getenv("QD_PHYTO_CHL0", "0.05"))
        frac = _env_list("QD_PHYTO_INIT_FRAC")
        if len(frac) >= self.S:
            f = np.clip(np.array(frac[:self.S], dtype=float), 0.0, None)
            tot = float(np.sum(f))
            f = f / tot if tot > 0 else np.full((self.S,), 1.0 / self.S)
        else:
            f = np.full((self.S,), 1.0 / self.S)
        self.init_frac_s = f
        self.dev = None
        self._host = self.default_state()
        if dev is not None:
            self.attach(dev)

    def default_state(self):
        C = np.zeros((self.S, self.grid.n_lat, self.grid.n_lon))
        for s in range(self.S):
            C[s] = self.init_frac_s[s] * self.chl0
            C[s, ~self.ocean_mask] = 0.0
        return C

    def attach(self, dev):
        self.dev = dev
        dev.phyto_configure(self.S, self.K_h, self.adv_alpha)
        dev.phyto_upload(self._host)
        self._host = None

    @property
    def C_phyto_s(self):
        return self.dev.phyto_download() if self.dev is not None else self._host

    @C_phyto_s.setter
    def C_phyto_s(self, C):
        C = np.clip(np.asarray(C, dtype=np.float64), 0.0, np.inf)          # load_autosave: clip, land = 0 (phyto.py:625-628)
        C[:, ~self.ocean_mask] = 0.0
        if self.dev is not None:
            self.dev.phyto_upload(C)
        else:
            self._host = C

    def advect_diffuse(self, dt_seconds):
        """One transport step on the resident currents (outside qd_step_n; inside it: step_n(..., phyto=True))."""
        self.dev.phyto_advect_diffuse(dt_seconds)

    # -- data/plankton.nc, the tracer part of save_distribution_nc / load_distribution_nc (phyto.py:737-802)
    def save_distribution_nc(self, path, day_value=None):
        """phyto.py:737-802.  This build owns the tracer part of plankton.nc (lat, lon, C_phyto_s, S, day).  The reference's file also
        holds what its DAILY host code maintains (alpha_water_scalar, Kd_490, the prognostic nutrient pool N, alpha_water_bands,
        bands_lambda_centers, the band dimension, H_mld_m, NB): when a file of the same grid and species count is already there --
        a data directory shared with a reference run -- those variables and attributes are carried through the rewrite."""
        from . import ncio
        try:
            g = self.grid
            dims = {"lat": g.n_lat, "lon": g.n_lon, "species": self.S}
            v = {"lat": ("f4", ("lat",), np.asarray(g.lat, np.float32)), "lon": ("f4", ("lon",), np.asarray(g.lon, np.float32)),
                 "C_phyto_s": ("f4", ("species", "lat", "lon"), self.C_phyto_s.astype(np.float32))}
            attrs = {"title": "Qingdai Phytoplankton Distributions", "S": int(self.S)}
            if os.path.exists(path):
                try:
                    odims, ovars, oattrs = ncio.read_nc_full(path)
                    if all(odims.get(k) == n for k, n in dims.items()):
                        for d, n in odims.items():
                            dims.setdefault(d, n)
                        for name, rec in ovars.items():
                            v.setdefault(name, rec)
                        for k, val in oattrs.items():
                            if k != "day":
                                attrs.setdefault(k, val)
                except Exception as e:                          # an unreadable old file is replaced, like the reference does
                    print(f"[Phyto] plankton.nc: could not carry the existing variables through ({e}).")
            if day_value is not None:
                attrs["day"] = float(day_value)
            ncio.write_nc(path, dims, v, attrs)
            return True
        except Exception as e:                                  # the reference logs and carries on
            print(f"[Phyto] save_distribution_nc failed: {e}")
            return False

    def load_distribution_nc(self, path):
        from . import ncio
        try:
            v, _ = ncio.read_nc(path, ["C_phyto_s"])
            C = np.asarray(v["C_phyto_s"], dtype=np.float64)
            if C.shape != (self.S, self.grid.n_lat, self.grid.n_lon):
                print(f"[Phyto] plankton.nc shape {C.shape} does not match (S={self.S}, grid); keeping the current state.")
                return False
            self.C_phyto_s = C
            return True
        except Exception as e:
            print(f"[Phyto] load_distribution_nc failed: {e}")
            return False


def advect_diffuse(dev, C_s, uo, vo, dt_seconds, land_mask, K_h=None, adv_alpha=None):
    """dev: qingdai_amd.device.Device (or `grid._ops()`); C_s: [S, n_lat, n_lon]; returns the new array."""
    C_s = np.array(C_s, dtype=np.float64, copy=True)
    if dt_seconds <= 0.0:
        return C_s
    K_h = float(os.getenv("QD_PHYTO_KH", os.getenv("QD_KH_OCEAN", "5.0e3"))) if K_h is None else float(K_h)
    adv_alpha = float(os.getenv("QD_PHYTO_ADV_ALPHA", "0.7")) if adv_alpha is None else float(adv_alpha)
    ocean = (np.asarray(land_mask) == 0)
    for s in range(C_s.shape[0]):
        C = C_s[s]
        C_adv = dev.op_advect(C, uo, vo, float(dt_seconds), ocean=True)
        C_new = (1.0 - adv_alpha) * C + adv_alpha * C_adv
        if K_h > 0.0:
            C_new = np.nan_to_num(C_new)
            C_new += float(dt_seconds) * K_h * dev.op_laplacian(C_new, ocean=True)
        C_new = np.clip(C_new, 0.0, np.inf)
        C_new[~ocean] = 0.0
        C_s[s] = C_new
    for j in (0, -1):
        row = ocean[j, :]
        if np.any(row):
            for s in range(C_s.shape[0]):
                C_s[s, j, row] = float(np.mean(C_s[s, j, :][row]))
    return C_s


# ------------------------------------------------------------------ daily step (PhytoManager.step_daily, phyto.py:339-435)
def _ref_float(name, default):
    """phyto.py:38-45: the variable as a float, the default when it is unset or does not parse."""
    v = os.getenv(name)
    if v is None:
        return default
    try:
        return float(v)
    except ValueError:
        return default


def _ref_list(name):
    """phyto.py:58-67: comma-separated floats, or None when unset, empty or unparsable."""
    v = os.getenv(name)
    if not v:
        return None
    try:
        out = [float(p) for p in (x.strip() for x in v.split(",")) if p != ""]
        return out if out else None
    except ValueError:
        return None


def daily_tables(S, bands=None, H_mld_m=None):
    """Everything PhytoManager.__init__ (phyto.py:94-281) derives from the QD_PHYTO_* / QD_ECO_* environment for the daily step,
    for S species: a dict of NumPy tables and scalars, the reference's attribute names."""
    from .spectral import band_weights_from_mode, make_bands, star_band_weights
    bands = bands or make_bands()
    NB = bands.nbands
    t = {"S": int(S), "NB": int(NB), "bands": bands}
    t["mu_max"] = _ref_float("QD_PHYTO_MU_MAX", 1.5)
    t["alpha_P"] = _ref_float("QD_PHYTO_ALPHA_P", 0.04)
    t["Q10"] = _ref_float("QD_PHYTO_Q10", 2.0)
    t["T_ref"] = _ref_float("QD_PHYTO_T_REF", 293.15)
    t["m0"] = _ref_float("QD_PHYTO_M_LOSS", 0.05)
    t["lambda_sink_m_per_day"] = _ref_float("QD_PHYTO_LAMBDA_SINK", 0.0)
    t["kd_exp_m"] = _ref_float("QD_PHYTO_KD_EXP_M", 0.5)
    if H_mld_m is None:
        try:
            H_mld_m = float(os.getenv("QD_OCEAN_H_M", os.getenv("QD_MLD_M", "50")))
        except ValueError:
            H_mld_m = 50.0
    t["H_mld"] = float(max(0.1, H_mld_m))
    for key, env, dflt in (("Kd0_b", "QD_PHYTO_KD0", ("QD_PHYTO_KD0_DEFAULT", 0.04)),
                           ("kchl_b", "QD_PHYTO_KD_CHL", ("QD_PHYTO_KD_CHL_DEFAULT", 0.02)),
                           ("Apure_b", "QD_PHYTO_APURE", ("QD_PHYTO_APURE_DEFAULT", 0.06))):
        a = np.full((NB,), _ref_float(*dflt), dtype=float)
        for i, val in enumerate((_ref_list(env) or [])[:NB]):
            a[i] = float(val)
        t[key] = a
    lam = bands.lambda_centers
    mu_arr = _ref_list("QD_PHYTO_SPEC_MU_NM") or []
    sigma_arr = _ref_list("QD_PHYTO_SPEC_SIGMA_NM") or []
    c_arr = _ref_list("QD_PHYTO_SPEC_C_REFLECT") or []
    p_arr = _ref_list("QD_PHYTO_SPEC_P_REFLECT") or []
    mu_defaults = np.linspace(460.0, 680.0, S) if S > 1 else np.array([_ref_float("QD_PHYTO_SHAPE_MU_NM", 550.0)])
    sigma_default = _ref_float("QD_PHYTO_SHAPE_SIGMA_NM", 70.0)
    c_default = _ref_float("QD_PHYTO_REFLECT_C", 0.02)
    p_default = _ref_float("QD_PHYTO_REFLECT_P", 0.5)
    shape = np.zeros((S, NB))
    c_reflect = np.zeros((S,))
    p_reflect = np.zeros((S,))
    for s in range(S):
        mu_s = mu_arr[s] if s < len(mu_arr) else float(mu_defaults[min(s, len(mu_defaults) - 1)])
        sigma_s = sigma_arr[s] if s < len(sigma_arr) else sigma_default
        g = np.exp(-((lam - mu_s) ** 2) / (2.0 * sigma_s ** 2))
        shape[s, :] = g / (float(np.sum(g)) + 1e-12)
        c_reflect[s] = c_arr[s] if s < len(c_arr) else c_default
        p_reflect[s] = p_arr[s] if s < len(p_arr) else p_default
    t["shape_sb"], t["c_reflect_s"], t["p_reflect_s"] = shape, c_reflect, p_reflect
    t["alpha_clip_min"] = _ref_float("QD_PHYTO_ALPHA_MIN", 0.0)
    t["alpha_clip_max"] = _ref_float("QD_PHYTO_ALPHA_MAX", 1.0)
    t["w_b"] = band_weights_from_mode(bands)
    mu_max_arr = _ref_list("QD_PHYTO_SPEC_MU_MAX") or []
    m0_arr = _ref_list("QD_PHYTO_SPEC_M0") or []
    t["mu_max_s"] = np.array([(mu_max_arr[s] if s < len(mu_max_arr) else t["mu_max"]) for s in range(S)], dtype=float)
    t["m0_s"] = np.array([(m0_arr[s] if s < len(m0_arr) else t["m0"]) for s in range(S)], dtype=float)
    t["enable_N"] = int(os.getenv("QD_PHYTO_ENABLE_N", "1")) == 1
    KN_list = _ref_list("QD_PHYTO_KN") or []
    Y_list = _ref_list("QD_PHYTO_YIELD") or []
    t["KN_s"] = np.array([(KN_list[s] if s < len(KN_list) else 0.5) for s in range(S)], dtype=float)
    t["Y_s"] = np.array([(Y_list[s] if s < len(Y_list) else 1.0) for s in range(S)], dtype=float)
    t["R_remin"] = _ref_float("QD_PHYTO_REMIN", 0.01)
    t["N_init"] = _ref_float("QD_PHYTO_N_INIT", 1.0)
    t["idx_490"] = int(np.argmin(np.abs(lam - 490.0)))
    specA, specB, tray = star_band_weights(bands)
    t["specA"], t["specB"], t["T_ray"] = specA, specB, tray
    t["sink"] = float(t["lambda_sink_m_per_day"]) / max(1e-6, t["H_mld"]) if t["lambda_sink_m_per_day"] > 0.0 else 0.0
    return t


def daily_device_tables(t):
    """-> (band_tab [8][NB], species_tab [6][S], shape [S][NB]) in the layout of qd_phyto_daily_configure."""
    band_tab = np.stack([t["Kd0_b"], t["kchl_b"], t["Apure_b"], t["bands"].delta_lambda, t["w_b"], t["specA"], t["specB"], t["T_ray"]])
    species_tab = np.stack([t["c_reflect_s"], t["p_reflect_s"], t["mu_max_s"], t["m0_s"], t["KN_s"], t["Y_s"]])
    return (np.ascontiguousarray(band_tab, dtype=np.float64), np.ascontiguousarray(species_tab, dtype=np.float64),
            np.ascontiguousarray(t["shape_sb"], dtype=np.float64))


def daily_schedule(next_time, t0, dt, n, day_seconds):
    """The reference driver's firing clock (run_simulation.py:1738,2052-2061) over the span t = t0 + dt * arange(n), or over the n
    times themselves when t0 is an array (the driver's, which count from the run's origin):
    -> (int32 [n] 1 = the step fires, the clock after the span).  Same float64 comparisons as the reference."""
    if np.ndim(t0):
        times = np.asarray(t0, dtype=np.float64)
        if times.shape != (n,):
            raise ValueError(f"daily_schedule: {n} steps but times of shape {times.shape}")
    else:
        times = t0 + dt * np.arange(n)
    fire = np.zeros(n, dtype=np.int32)
    nt = float(next_time)
    for k in range(n):
        t = float(times[k])
        if t >= nt:
            fire[k] = 1
            nt = t + day_seconds
    return fire, nt


def diag_line(S, rec):
    """phyto.py:421-433 from one device log record (steps so far, <C_tot>, <Kd490>, <alpha_water>)."""
    return (f"[PhytoDiag] S={S} | ⟨Chl_tot⟩={rec[1]:.3f} mg/m^3 | ⟨Kd490⟩={rec[2]:.3f} m^-1 | "
            f"⟨α_water⟩={rec[3]:.3f}")


class PhytoDaily:
    """The daily part of the reference's PhytoManager on the resident tracers of a PhytoTracers (same species count): tables from
    the environment exactly as phyto.py:94-281 builds them, the nutrient pool N (N_init on the ocean, 0 on land), the band
    reflectances alpha_water_bands, alpha_water_scalar (the device's WATER_ALPHA) and Kd_490, all resident.  `phyto_next_time` is
    the driver's firing clock (day_in_seconds = 2 pi / PLANET_OMEGA)."""

    def __init__(self, tracers, H_mld_m=None, diag=None, dev=None, couple=None, day_seconds=None):
        self.tracers = tracers
        self.grid = tracers.grid
        self.S = tracers.S
        self.ocean_mask = tracers.ocean_mask
        self.t = daily_tables(self.S, H_mld_m=H_mld_m)
        self.bands = self.t["bands"]
        self.NB = self.bands.nbands
        self.H_mld = self.t["H_mld"]
        self.diag = (int(os.getenv("QD_PHYTO_DIAG", "1")) == 1) if diag is None else bool(diag)
        self.couple = (int(os.getenv("QD_PHYTO_ALBEDO_COUPLE", "1")) == 1) if couple is None else bool(couple)
        self.day_seconds = float(2 * np.pi / 8.726646259971648e-5) if day_seconds is None else float(day_seconds)
        self.phyto_next_time = 0.0
        self.dt_days = 1.0
        N = np.full((self.grid.n_lat, self.grid.n_lon), self.t["N_init"], dtype=float)
        N[~self.ocean_mask] = 0.0
        self._N_host = N
        self.dev = None
        self.n_steps = 0
        if self.diag:
            m = self.t["mu_max_s"]
            print(f"[Phyto] NB={self.NB} bands, H_mld={self.H_mld:.1f} m | S={self.S}, mu={m.min():.2f}..{m.max():.2f}/d | "
                  f"alpha_P={self.t['alpha_P']:.3f} | m0={self.t['m0']:.3f} d^-1 | Q10={self.t['Q10']:.2f}")
        if dev is not None:
            self.attach(dev)

    def params(self):
        from . import _lib
        t = self.t
        return _lib.qd_phyto_daily_params(self.S, self.NB, t["idx_490"], 1 if t["enable_N"] else 0, 1 if self.couple else 0, 0,
                                          t["H_mld"], t["alpha_P"], t["Q10"], t["T_ref"], t["kd_exp_m"], t["sink"], t["R_remin"],
                                          t["alpha_clip_min"], t["alpha_clip_max"], float(self.dt_days))

    def attach(self, dev):
        if self.tracers.dev is not dev:
            raise ValueError("PhytoDaily: the tracers live on another device handle (attach them first)")
        self.dev = dev
        dev.phyto_daily_configure(self.params(), *daily_device_tables(self.t))
        dev.upload_now("PHYTO_N", self._N_host)
        self._N_host = None

    # -- the reference's surface
    def step_daily(self, star_row, use_sst=True, dt_days=1.0):
        """One daily step now on the star row of the current step (ThermalForcing.star_table): T_w is SST (use_sst) or T_s.
        Returns (alpha_water_bands, alpha_water_scalar) like the reference; prints the [PhytoDiag] line when diag is on."""
        if float(dt_days) != self.dt_days:
            self.dt_days = float(dt_days)
            self.dev.phyto_daily_configure(self.params(), *daily_device_tables(self.t))
        self.dev.phyto_daily(star_row, use_sst)
        self._fired(1)
        self.print_diag(self.dev.phyto_daily_log())
        return self.get_alpha_maps()

    def _fired(self, n):
        self.n_steps += int(n)

    def schedule(self, t0, dt, n):
        """The span's firing steps; advances phyto_next_time as the reference's loop would."""
        fire, self.phyto_next_time = daily_schedule(self.phyto_next_time, t0, dt, n, self.day_seconds)
        return fire

    # ---- span participant (the protocol is stated in Device.step_n)
    def span_clock(self):
        return self.phyto_next_time

    def span_schedule(self, t0, dt, n):
        fire = self.schedule(t0, dt, n)
        self.dev.phyto_daily_schedule(fire)
        return int(fire.sum())                 # -> the span's daily steps, for _fired once the span has run

    def span_restore(self, clock):
        self.phyto_next_time = clock

    def span_deliver(self, dt):
        self.print_diag(self.dev.phyto_daily_log())    # the span's [PhytoDiag] lines, oldest first

    def print_diag(self, records):
        if self.diag:
            for rec in records:
                print(diag_line(self.S, rec))

    def get_alpha_maps(self):
        """(alpha_water_bands [NB, n_lat, n_lon] or None before the first daily step, alpha_water_scalar)."""
        bands = self.dev.phyto_daily_bands(self.NB) if self.n_steps > 0 else None
        return bands, np.array(self.dev.get("WATER_ALPHA"), copy=True)

    def get_kd490(self):
        return np.array(self.dev.get("KD490"), copy=True)

    @property
    def N(self):
        return np.array(self.dev.get("PHYTO_N"), copy=True) if self.dev is not None else self._N_host

    @N.setter
    def N(self, arr):
        arr = np.asarray(arr, dtype=np.float64)
        if self.dev is not None:
            self.dev.upload_now("PHYTO_N", arr)
        else:
            self._N_host = arr.copy()

    # -- data/plankton.nc with the reference's variable set (save_distribution_nc / load_distribution_nc, phyto.py:737-802)
    def save_distribution_nc(self, path, day_value=None):
        from . import ncio
        try:
            g = self.grid
            os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
            dims = {"lat": g.n_lat, "lon": g.n_lon, "species": self.S, "band": self.NB}
            f4 = np.float32
            v = {"lat": ("f4", ("lat",), np.asarray(g.lat, f4)), "lon": ("f4", ("lon",), np.asarray(g.lon, f4)),
                 "C_phyto_s": ("f4", ("species", "lat", "lon"), self.tracers.C_phyto_s.astype(f4))}
            bands, scalar = self.get_alpha_maps()
            if bands is not None:
                v["alpha_water_bands"] = ("f4", ("band", "lat", "lon"), bands.astype(f4))
            v["alpha_water_scalar"] = ("f4", ("lat", "lon"), scalar.astype(f4))
            v["Kd_490"] = ("f4", ("lat", "lon"), self.get_kd490().astype(f4))
            v["N"] = ("f4", ("lat", "lon"), self.N.astype(f4))
            v["bands_lambda_centers"] = ("f4", ("band",), np.asarray(self.bands.lambda_centers, f4))
            attrs = {"title": "Qingdai Phytoplankton Distributions", "H_mld_m": float(self.H_mld), "S": int(self.S),
                     "NB": int(self.NB)}
            if day_value is not None:
                attrs["day"] = float(day_value)
            ncio.write_nc(path, dims, v, attrs)
            if self.diag:
                print(f"[Phyto] Distribution NetCDF written: '{path}'")
            return True
        except Exception as e:                                  # the reference logs and carries on
            print(f"[Phyto] save_distribution_nc failed: {e}")
            return False

    def load_distribution_nc(self, path):
        """The reference's load (phyto.py:805-870): every present variable must fit the grid (and the band count), then C_phyto_s
        (clipped, land 0), alpha_water_scalar (clipped to the alpha bounds) and Kd_490 (clipped to >= 0) are restored.  N is not
        restored, and the band stack is rebuilt by the next daily step, which the driver runs on its first iteration."""
        from . import ncio
        try:
            v, _ = ncio.read_nc(path, ["C_phyto_s", "alpha_water_bands", "alpha_water_scalar", "Kd_490"])
        except Exception as e:
            print(f"[Phyto] load_distribution_nc failed: {e}")
            return False
        shp = (self.grid.n_lat, self.grid.n_lon)
        C, ab, aS, kd = (v.get(k) for k in ("C_phyto_s", "alpha_water_bands", "alpha_water_scalar", "Kd_490"))
        ok = (C is not None and C.shape == (self.S,) + shp and (ab is None or ab.shape == (self.NB,) + shp) and
              (aS is None or aS.shape == shp) and (kd is None or kd.shape == shp))
        if not ok:
            print("[Phyto] plankton.nc dims mismatch; keep=True")
            return False
        self.tracers.C_phyto_s = np.asarray(C, dtype=np.float64)
        if aS is not None:
            self.dev.upload_now("WATER_ALPHA", np.clip(np.asarray(aS, dtype=np.float64), self.t["alpha_clip_min"], self.t["alpha_clip_max"]))
        if kd is not None:
            self.dev.upload_now("KD490", np.clip(np.asarray(kd, dtype=np.float64), 0.0, np.inf))
        if self.diag:
            print(f"[Phyto] plankton.nc loaded: C_phyto_s[{(self.S,) + shp}], alpha_bands={'OK' if ab is not None else 'none'}, "
                  f"alpha_scalar={'OK' if aS is not None else 'none'}")
        return True
