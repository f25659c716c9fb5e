"""The parameter sweep's one table: every run-time parameter of `qd_params` (qingdai_amd.params `_DOUBLES + _INTS`) with the
scenario it is live in, the value it is moved to and the settings that make it matter.  Shared by

  * tests/test_param_sweep_cpu.py   completeness, liveness in the oracle, the oracle against the reference's digests, the env layer
  * tests/test_gpu_param_sweep.py   the device (C-ABI) against the oracle and the reference's digests, row by row
  * oracle/gen_golden.py            case_param_sweep: the reference run per row -> tests/golden/param_sweep_<scenario>_37x72.npz

All scenarios run at 37 x 72, the smallest committed-fixture shape on which the row-streaming kernels run (three strips and a ragged
second column tile); every run is a pure function of the override dict.

To add a parameter: add its row below (scenario, a perturbed value inside the range the reference accepts, companions that make
it live) -- or an entry of DEAD / EXEMPT with its reason -- and regenerate the fixtures if the row has one.  The completeness test
fails until every field of `_DOUBLES + _INTS` is in exactly one of the three.
"""
import numpy as np

import qd_oracle as qo

SHAPE = (37, 72)
DT = 300.0
STEP_TOL = 1e-9            # tests/test_gpu_parity.py: whole steps, f64, relative to the field's max-norm
COUPLED_OCEAN_TOL = 1e-7   # uo, vo, eta of a coupled run after <= 4 steps (test_driver_loop_vs_oracle)
STEP1_DIAG_TOL = 1e-11     # step-1 precipitation / albedo diagnostics (test_driver_physics_vs_reference)
N_SAMPLE = 64

STATE = ("u", "v", "h", "T_s", "q", "cloud_cover", "h_ice")
DIAG = ("E_flux_last", "P_cond_flux_last", "LH_last", "LH_release_last", "olr")
CS_OCEAN0 = 1000.0 * 4200.0 * 50.0


def relerr(a, b):
    a = np.asarray(a, dtype=float)
    b = np.asarray(b, dtype=float)
    return float(np.max(np.abs(a - b))) / max(float(np.max(np.abs(b))), 1e-300)


def surface():
    from qingdai_amd.topography import create_land_sea_mask, generate_base_properties
    g = qo.Grid(*SHAPE)
    mask = create_land_sea_mask(g)
    alb, fric = generate_base_properties(mask)
    return g, mask, alb, fric


def seeded_state(shape, seed, wet=False, cloudy=False, icy=False):
    """The seeded initial state of oracle/gen_golden.py's fixtures (same draws in the same order)."""
    r = np.random.default_rng(seed)
    nlat, nlon = shape
    lat = np.linspace(-np.pi / 2, np.pi / 2, nlat)[:, None]
    lon = np.linspace(0, 2 * np.pi, nlon)[None, :]
    st = {}
    st["u"] = 25.0 * np.cos(lat) * np.sin(2 * lon) + r.normal(0, 3.0, shape)
    st["v"] = 8.0 * np.sin(2 * lat) * np.cos(3 * lon) + r.normal(0, 2.0, shape)
    st["h"] = 8000.0 + 300 * np.sin(lat) ** 2 + 40.0 * np.cos(lat) * np.cos(2 * lon) + r.normal(0, 2.0, shape)
    st["T_s"] = 262.0 + 38.0 * np.cos(lat) ** 2 + r.normal(0, 1.0, shape)
    st["q"] = np.clip(0.006 + 0.004 * np.cos(lat) ** 2 + r.normal(0, 5e-4, shape), 0.0, 0.5)
    st["cloud_cover"] = np.zeros(shape)
    st["h_ice"] = np.zeros(shape)
    if wet:
        st["h"] = st["h"] - 7600.0
        st["q"] = st["q"] + 0.02 * (r.random(shape) > 0.5)
    if cloudy:
        st["cloud_cover"] = np.clip(0.3 + 0.3 * np.sin(3 * lon) * np.cos(lat) + r.normal(0, 0.05, shape), 0, 1)
    if icy:
        st["h_ice"] = np.where(np.abs(lat) > 1.1, 0.4 + 0.3 * r.random(shape), 0.0) * np.ones(shape)
        st["T_s"] = np.where(np.abs(lat) > 1.1, 268.0 + 4 * r.random(shape), st["T_s"])
    return st


def sample_cells(shape=SHAPE, n=N_SAMPLE, seed=1234):
    """Flat indices of `n` cells: both pole rows and the columns 0 and n_lon-1 always among them."""
    nlat, nlon = shape
    r = np.random.default_rng(seed)
    fixed = [(0, 0), (0, nlon - 1), (nlat - 1, 0), (nlat - 1, nlon - 1), (0, nlon // 2), (nlat - 1, nlon // 3),
             (nlat // 2, 0), (nlat // 2, nlon - 1), (1, 1), (nlat - 2, nlon - 2)]
    idx = [i * nlon + j for i, j in fixed]
    for k in r.permutation(nlat * nlon):
        if len(idx) >= n:
            break
        if int(k) not in idx:
            idx.append(int(k))
    return np.asarray(sorted(idx), dtype=np.int64)


def digest(field, cells):
    """(values at the sampled cells, np.sum, max|.|) of one field."""
    f = np.asarray(field, dtype=float)
    return f.ravel()[cells].copy(), float(np.sum(f)), float(np.max(np.abs(f)))


# ======================================================================================================== scenarios
# Each scenario: `base` (overrides of every run of it), the compared fields with their device-vs-oracle bound, and the bound
# tests/test_oracle_golden.py holds the oracle to against the reference for that family (None: no reference entry point).
COLUMN_FIELDS = STATE + DIAG + ("cloud_eff_last",)
OCEAN_FIELDS = ("uo", "vo", "eta", "Ts")
DRIVER_FIELDS = ("u", "v", "h", "T_s", "q", "cloud_cover", "h_ice", "precip", "albedo", "S_snow", "C_snow", "W_land", "runoff",
                 "uo", "vo", "eta", "SST", "s1_precip", "s1_albedo")

HYDRO_FIELDS = ("P_rain", "P_snow", "S_next", "melt", "C_snow", "alpha_snow", "W_next", "R_flux")

SCENARIOS = {
    # case_time_step's loop, albedo handed to time_step, wet + cloudy + icy seeded state, 7 steps (shapiro_every = 6 fires in the
    # baseline; *_every = 2 fires three times).  energy_w = 0.7 and not 1: at 1 the Newton path (c_sfc, greenhouse_factor)
    # has weight zero and is dead.
    "column": dict(base={"energy_w": 0.7}, nsteps=7, fields={k: STEP_TOL for k in COLUMN_FIELDS}, ref_tol=1e-11),
    # the same loop from the constructor's own initial state (h = H + 300 sin^2, q from q_init_rh): the only place H acts.
    # Two steps, not three: from that state the third step's gather on the south pole row is chaotic in the reference arithmetic
    # itself (oracle against oracle with h scaled by 1 + 1e-15: 2.8e-13 after two steps, 6.5e-5 in T_s after three).
    "column_init": dict(base={"energy_w": 0.7}, nsteps=2, fields={k: STEP_TOL for k in COLUMN_FIELDS}, ref_tol=1e-11),
    # case_ocean's loop, strong winds, ice mask, seeded currents and eta; ocean_cfl = 0.02 gives n_sub >= 3
    "ocean": dict(base={"ocean_cfl": 0.02}, nsteps=3, fields={k: STEP_TOL for k in OCEAN_FIELDS}, ref_tol=1e-14),
    # the cold, low-h driver loop of test_driver_loop_vs_oracle with the ocean coupled, an elevation map, an ice-sheet-deep polar
    # snowpack and a wet land bucket: Device.step_n (through Simulation.run_steps) against DriverOracle.step, 1 + 3 steps
    "driver": dict(base={}, nsteps=4, ref_tol=None,
                   fields={**{k: STEP_TOL for k in DRIVER_FIELDS}, "uo": COUPLED_OCEAN_TOL, "vo": COUPLED_OCEAN_TOL,
                           "eta": COUPLED_OCEAN_TOL, "s1_precip": STEP1_DIAG_TOL, "s1_albedo": STEP1_DIAG_TOL}),
    # one driver_physics call with QD_OROG=1 and an uploaded elevation map (case_orography's inputs)
    "orog": dict(base={"orog_enable": 1}, nsteps=1, fields={"precip": STEP1_DIAG_TOL}, ref_tol=0.0),
    # CPU only (the device has no entry point for it alone): the reference's hydrology functions -- phase split, snowpack, land
    # bucket (pygcm/hydrology.py:100-260) -- composed the way the driver calls them, on seeded inputs.  It ties the hydrology
    # rows of the driver scenario, and their QD_* names, to the reference; the oracle restates those functions operation for
    # operation, so the bound is bit equality.
    "hydro": dict(base={}, nsteps=1, fields={k: STEP_TOL for k in HYDRO_FIELDS}, ref_tol=0.0),
}


def live_threshold(tol):
    """Liveness: the perturbed oracle run must move a compared field by 1000 x the bound that field is held to, 1e-6 at least."""
    return max(1e-6, 1000.0 * tol)


_CACHE = {}


def _inputs(name):
    if name in _CACHE:
        return _CACHE[name]
    g, mask, alb, fric = surface()
    lat = np.deg2rad(g.lat_mesh)
    if name in ("column", "column_init"):
        st = None
        if name == "column":
            st = seeded_state(SHAPE, 5, wet=True, cloudy=True, icy=True)
            # dry polar air, so that the sea ice evaporates (ice_evap_scale); the pole rows ice free, warm (288 K) under cold air
            # (h = -1500: T_a = 273 K), so that their ocean cells lose heat above freezing and the polar-row freeze fix has
            # something to fix (under ice the t_freeze cap hides it)
            st["q"] = np.where(np.abs(lat) > 1.1, 0.3 * st["q"], st["q"])
            for j in (0, -1):
                st["h_ice"][j, :] = 0.0
                st["T_s"][j, :] = 288.0 + 0.01 * np.arange(SHAPE[1])
                st["h"][j, :] = -1500.0
        d = dict(state=st,
                 albedo=np.where(mask == 0, 0.08, alb), csmap=np.where(mask == 1, 3e6, CS_OCEAN0).astype(float))
    elif name == "ocean":
        st = seeded_state(SHAPE, 22, icy=True)
        r = np.random.default_rng(22 + 3)
        Q_net = 240.0 * np.cos(lat) - 120.0 + r.normal(0, 5.0, SHAPE)
        d = dict(u_atm=st["u"] * 4.0, v_atm=st["v"] * 4.0, Q_net=Q_net, ice=st["h_ice"] > 0.0,
                 init_Ts=np.where(mask == 0, st["T_s"], 288.0),
                 uo=np.where(mask == 0, 0.3 * np.cos(lat) + r.normal(0, 0.05, SHAPE), 0.0),
                 vo=np.where(mask == 0, r.normal(0, 0.05, SHAPE), 0.0),
                 eta=np.where(mask == 0, r.normal(0, 0.2, SHAPE), 0.0))
    elif name == "driver":
        from qingdai_amd.topography import generate_elevation_map
        r = np.random.default_rng(77)
        land = (mask == 1)
        alat = np.abs(g.lat_mesh)
        elev = np.maximum(generate_elevation_map(g, seed=77), 0.0) * land
        # 8 mm of snow on the land between 50 and 62 degrees; poleward of 62 an ice sheet of 3e4 mm w.e. (100 m at rho_snow = 300)
        S0 = np.where(land & (alat > 50), 8.0, 0.0) + np.where(land & (alat > 62), 3.0e4, 0.0)
        d = dict(h0=8000.0 - 10500.0 * np.sin(lat) ** 2 + r.normal(0, 2.0, SHAPE), Ts0=262.0 + 36.0 * np.cos(lat) ** 2, S0=S0,
                 W0=np.where(land, 20.0 + 30.0 * r.random(SHAPE), 0.0), elev=elev,
                 hice0=np.where((~land) & (alat > 63), 0.4 + 0.3 * r.random(SHAPE), 0.0),
                 u0=20.0 * np.cos(lat) * np.sin(2 * np.deg2rad(g.lon_mesh)) + r.normal(0, 2.0, SHAPE),
                 v0=6.0 * np.sin(2 * lat) * np.cos(3 * np.deg2rad(g.lon_mesh)) + r.normal(0, 1.0, SHAPE))
    elif name == "orog":
        from qingdai_amd.topography import generate_elevation_map
        st = seeded_state(SHAPE, 52, cloudy=True)
        r = np.random.default_rng(52 + 100)
        d = dict(u=st["u"], v=st["v"], T_s=st["T_s"], cloud_cover=st["cloud_cover"],
                 elev=np.maximum(generate_elevation_map(g, seed=52), 0.0) * (mask == 1),
                 Pc=np.abs(r.normal(3e-5, 2e-5, SHAPE)))
    elif name == "hydro":
        r = np.random.default_rng(91)
        land = (mask == 1)
        d = dict(P_flux=np.abs(r.normal(2e-5, 1e-5, SHAPE)), T_hat=272.0 + 10.0 * np.cos(lat) ** 2 - 6.0 * r.random(SHAPE),
                 S=np.where(land, 40.0 * r.random(SHAPE), 0.0), W=np.where(land, 20.0 + 30.0 * r.random(SHAPE), 0.0),
                 E_land=np.where(land, np.abs(r.normal(1e-5, 5e-6, SHAPE)), 0.0))
    else:
        raise KeyError(name)
    d.update(g=g, mask=mask, alb=alb, fric=fric)
    _CACHE[name] = d
    return d


def scenario_over(name, over):
    return {**SCENARIOS[name]["base"], **over}


# ---------------------------------------------------------------------------------------------------- oracle runs
def run_oracle(name, over, bump=None):
    """The oracle on the scenario's inputs with `over` on top of the scenario's base.  `bump`: (field, factor) scales one input
    field -- the 1e-15 perturbation of the conditioning measurement (tests/test_oracle_polar_noise_cpu.py's method)."""
    from types import SimpleNamespace
    from qd_oracle import physics as oph
    from qd_oracle.driver import DriverOracle
    I = _inputs(name)
    P = qo.defaults(**scenario_over(name, over))
    g, mask = I["g"], I["mask"]
    n = SCENARIOS[name]["nsteps"]

    def bumped(key, arr):
        return arr * bump[1] if bump is not None and bump[0] == key else arr.copy()
    if name in ("column", "column_init"):
        m = qo.AtmosOracle(g, I["fric"], mask, P, C_s_map=I["csmap"])
        if I["state"] is not None:
            for k in STATE:
                setattr(m, k, bumped(k, I["state"][k]))
        elif bump is not None:
            setattr(m, bump[0], getattr(m, bump[0]) * bump[1])
        f = qo.Forcing(g)
        for i in range(n):
            a_, b_ = f.insolation_components(i * DT)
            m.isr_A, m.isr_B, m.isr = a_, b_, a_ + b_
            m.time_step(f.equilibrium_temp(i * DT, I["albedo"]), DT, albedo=I["albedo"])
        return {k: np.array(getattr(m, k)) for k in COLUMN_FIELDS}
    if name == "ocean":
        oc = qo.OceanOracle(g, mask, P, init_Ts=I["init_Ts"])
        oc.uo, oc.vo, oc.eta = bumped("uo", I["uo"]), bumped("vo", I["vo"]), bumped("eta", I["eta"])
        nsub = []
        for _ in range(n):
            oc.step(DT, I["u_atm"], I["v_atm"], Q_net=I["Q_net"], ice_mask=I["ice"])
            nsub.append(oc.last_n_sub)
        out = {k: np.array(getattr(oc, k)) for k in OCEAN_FIELDS}
        out["n_sub"] = nsub
        return out
    if name == "driver":
        m = qo.AtmosOracle(g, I["fric"], mask, P, C_s_map=np.where(mask == 1, 3e6, P.Cs_ocean).astype(float))
        m.h, m.T_s, m.u, m.v = bumped("h", I["h0"]), I["Ts0"].copy(), bumped("u", I["u0"]), I["v0"].copy()
        m.h_ice = I["hice0"].copy()
        oc = qo.OceanOracle(g, mask, P, init_Ts=np.full(SHAPE, 288.0))
        d = DriverOracle(g, m, oc, qo.Forcing(g), mask, I["alb"], P, elevation=I["elev"])
        d.S_snow, d.W_land = I["S0"].copy(), I["W0"].copy()
        out = {}
        for i in range(n):
            d.step(i * DT, DT)
            if i == 0:
                out.update(s1_precip=d.precip.copy(), s1_albedo=d.albedo.copy())
        out.update({k: np.array(getattr(m, k)) for k in ("u", "v", "h", "T_s", "q", "cloud_cover", "h_ice")})
        out.update(precip=d.precip, albedo=d.albedo, S_snow=d.S_snow, C_snow=d.C_snow, W_land=d.W_land, runoff=d.R_flux,
                   uo=oc.uo, vo=oc.vo, eta=oc.eta, SST=oc.Ts)
        return out
    if name == "hydro":
        from qd_oracle import driver as odr
        land = (mask == 1)
        P_rain, P_snow, _ = odr.partition_precip_phase_smooth(I["P_flux"], I["T_hat"], P.snow_thresh_K, P.snow_t_band_K)
        S_next, melt, C_snow, alpha_snow = odr.snowpack_step(I["S"], P_snow * land, I["T_hat"], P, DT)
        W_next, R_flux = odr.update_land_bucket(I["W"], (P_rain * land) + melt, I["E_land"], P, DT)
        return dict(P_rain=P_rain, P_snow=P_snow, S_next=S_next, melt=melt, C_snow=C_snow, alpha_snow=alpha_snow, W_next=W_next,
                    R_flux=R_flux)
    if name == "orog":
        ns = SimpleNamespace(u=bumped("u", I["u"]), v=I["v"], T_s=I["T_s"], cloud_cover=I["cloud_cover"], P_cond_flux_last=I["Pc"])
        fac = oph.compute_orographic_factor(g, I["elev"], ns.u, ns.v, k_orog=float(P.orog_k)) if int(P.orog_enable) == 1 else None
        return {"precip": oph.diagnose_precipitation_hybrid(ns, g, P, orog_factor=fac)}
    raise KeyError(name)


# ---------------------------------------------------------------------------------------------------- device runs
def run_device(name, over):
    """The same scenario through the C-ABI: the calls the parity tests use.  One handle per run."""
    import qingdai_amd as qa
    from qingdai_amd.device import Device
    I = _inputs(name)
    p = qa.QdParams(**scenario_over(name, over))
    mask = I["mask"]
    n = SCENARIOS[name]["nsteps"]
    grid = qa.SphericalGrid(*SHAPE)
    if name in ("column", "column_init"):
        m = qa.SpectralModel(grid, I["fric"], g=p.g, H=p.H, tau_rad=p.tau_rad, greenhouse_factor=p.greenhouse_factor,
                             C_s_map=I["csmap"], land_mask=mask, Cs_ocean=p.Cs_ocean, Cs_land=p.Cs_land, Cs_ice=p.Cs_ice, params=p)
        if I["state"] is not None:
            for k in STATE:
                setattr(m, k, I["state"][k].copy())
        forcing = qa.ThermalForcing(grid, qa.OrbitalSystem())
        m._dev.set("ALBEDO", I["albedo"])
        for i in range(n):
            forcing.update_device(i * DT, with_teq=True)
            m.time_step(None, DT, albedo=True)
        out = {k: np.array(getattr(m, k)) for k in COLUMN_FIELDS}
        m._dev.close()
        return out
    if name == "ocean":
        oc = qa.WindDrivenSlabOcean(grid, mask, p.H_ocean, init_Ts=I["init_Ts"], params=p)
        oc.uo, oc.vo, oc.eta = I["uo"].copy(), I["vo"].copy(), I["eta"].copy()
        nsub = []
        for _ in range(n):
            oc.step(DT, I["u_atm"], I["v_atm"], Q_net=I["Q_net"], ice_mask=I["ice"])
            nsub.append(oc.last_n_sub)
        out = {k: np.array(getattr(oc, k)) for k in OCEAN_FIELDS}
        out["n_sub"] = nsub
        oc._dev.close()
        return out
    if name == "driver":
        from qingdai_amd.driver import Simulation
        sim = Simulation(*SHAPE, params=p, use_ocean=True, quiet=True, ecology=False, phyto=False)
        sim.gcm.h, sim.gcm.T_s, sim.gcm.u, sim.gcm.v = I["h0"].copy(), I["Ts0"].copy(), I["u0"].copy(), I["v0"].copy()
        sim.gcm.h_ice = I["hice0"].copy()
        sim.dev.set("S_SNOW", I["S0"])
        sim.dev.set("W_LAND", I["W0"])
        sim.dev.upload_now("ELEVATION", I["elev"])
        sim.run_steps(1)
        out = dict(s1_precip=np.array(sim.dev.get("PRECIP")), s1_albedo=np.array(sim.dev.get("ALBEDO")))
        sim.run_steps(n - 1)
        out.update({k: np.array(getattr(sim.gcm, k)) for k in ("u", "v", "h", "T_s", "q", "cloud_cover", "h_ice")})
        for k, f in (("precip", "PRECIP"), ("albedo", "ALBEDO"), ("S_snow", "S_SNOW"), ("C_snow", "C_SNOW"), ("W_land", "W_LAND"),
                     ("runoff", "RUNOFF")):
            out[k] = np.array(sim.dev.get(f))
        out.update(uo=np.array(sim.ocean.uo), vo=np.array(sim.ocean.vo), eta=np.array(sim.ocean.eta), SST=np.array(sim.ocean.Ts))
        sim.dev.close()
        return out
    if name == "orog":
        p.has_csmap = 0
        dev = Device(grid, p)
        for f, arr in (("LAND_MASK", mask), ("BASE_ALBEDO", I["alb"]), ("FRICTION", I["fric"]), ("ELEVATION", I["elev"]),
                       ("U", I["u"]), ("V", I["v"]), ("TS", I["T_s"]), ("CLOUD", I["cloud_cover"]), ("PCOND", I["Pc"])):
            dev.upload_now(f, arr)
        dev.driver_physics(DT)
        out = {"precip": np.array(dev.get("PRECIP"))}
        dev.close()
        return out
    raise KeyError(name)


# ============================================================================================================ table
# pin: where the row's tie to the reference lives when it has no fixture entry of its own
A5A6 = "test_oracle_golden.py::test_driver_known_answers_appendix_a5_a6"


def R(param, scenario, value, comp=None, unfused=False, fixture=None, how="env", tol=None, noise=None):
    """One row.  comp: companion overrides applied to the baseline AND the perturbed run.  unfused: the parameter reaches the fused
    dynamics / ocean kernels, so the row runs a second time with QD_FUSED=0.  fixture: the row has a reference digest (default:
    every column / ocean / orog row).  how: how the reference is given the value -- "env" (its QD_* variable), "ctor" (constructor
    argument), "attr" (attribute set after construction), "arg" (function argument); None for device-vs-oracle-only rows.
    tol: per-field bounds replacing the scenario's (only ever 100 x `noise`, the oracle's own measured 1e-15-perturbation noise)."""
    if fixture is None:
        fixture = scenario != "driver"
    pin = None
    if not fixture:
        pin = A5A6 + (" + the hydro digest (test_param_sweep_cpu.py::test_oracle_matches_the_reference_digest)" if param in HYDRO_PARAMS else "")
    return dict(param=param, scenario=scenario, value=value, comp=dict(comp or {}), unfused=unfused, fixture=fixture,
                how=(how if fixture else None), pin=pin, tol=tol, noise=noise, id=f"{param}={value}")


# the driver rows whose parameter the reference's hydrology functions read themselves (pygcm/hydrology.py:44-80, 172)
HYDRO_PARAMS = ("runoff_tau_days", "wland_cap_mm", "snow_thresh_K", "snow_melt_rate_mm_day", "snow_t_band_K", "snow_ddf_mm_per_k_day",
                "snow_melt_tref_K", "swe_ref_mm", "swe_max_mm", "snow_albedo_fresh", "snow_melt_mode")


LWV1 = {"lw_v2": 0}
SPEC = {"spec_every": 2}
SHALLOW = {"H_ocean": 10.0}                 # a 10 m mixed layer: the heating term is five times the default's
FALLBACK = {"pq_min": 1e-3}                  # the seeded P_cond has a mean of 3e-5: the fallback runs
QNET = {"lw_v2": 0, "gh_lock": 0}            # under gh_lock = 1 the surface longwave does not depend on the emissivity
ROWS = [
    # ---- SpectralModel constructor arguments
    R("g", "column", 9.5, how="ctor"), R("H", "column_init", 7500.0, how="ctor"), R("tau_rad", "column", 5 * 86400.0, how="ctor"),
    R("greenhouse_factor", "column", 0.5, how="ctor"),
    R("t_freeze", "column", 269.5), R("rho_i", "column", 900.0), R("L_f", "column", 3.0e5),
    R("Cs_ocean", "column", 1.5e8, how="ctor"), R("Cs_land", "column", 4e6, how="ctor"),
    # ---- humidity
    R("C_E", "column", 1.6e-3), R("rho_a", "column", 1.0), R("h_mbl", "column", 1000.0), R("L_v", "column", 2.3e6),
    R("p0", "column", 0.9e5), R("ocean_evap_scale", "column", 0.8), R("land_evap_scale", "column", 0.7),
    R("ice_evap_scale", "column", 0.2), R("tau_cond", "column", 900.0),
    # ---- energy column
    R("sw_a0", "column", 0.10), R("sw_kc", "column", 0.30), R("lw_eps0", "column", 0.60, LWV1), R("lw_kc", "column", 0.30, LWV1),
    R("t_floor", "column", 269.0), R("c_sfc", "column", 1.5e7), R("energy_w", "column", 0.4), R("rh0", "column", 0.5),
    R("k_q", "column", 0.4), R("k_p", "column", 0.5), R("pcond_ref", "column", 2e-6), R("hice_ref", "column", 0.4),
    R("ch", "column", 2.0e-3), R("cp_a", "column", 1100.0), R("atm_h", "column", 1200.0),
    R("gh_factor_lw", "column", 0.5), R("eps_ocean", "column", 0.95), R("eps_land", "column", 0.90),
    R("eps_ice", "column", 0.95), R("lw_tau0", "column", 5.0), R("lw_ktau", "column", 1.5),
    # ---- dynamics filters (fused dynamics kernels: second run with QD_FUSED=0)
    R("sigma4", "column", 0.03, unfused=True), R("k4_u", "column", 1.0e15, unfused=True), R("k4_v", "column", 1.0e15, unfused=True),
    R("k4_h", "column", 1.0e15, unfused=True), R("k4_q", "column", 1.0e15, unfused=True),
    R("k4_cloud", "column", 1.0e15, unfused=True),
    R("spec_cutoff", "column", 0.6, SPEC, unfused=True), R("spec_damp", "column", 0.3, SPEC, unfused=True),
    R("diff_factor", "column", 0.99, unfused=True),
    # ---- ocean
    R("H_ocean", "ocean", 40.0, how="ctor", unfused=True), R("rho_w", "ocean", 1025.0, unfused=True),
    R("cp_w", "ocean", 3500.0, SHALLOW, unfused=True), R("g_ocean", "ocean", 9.5, how="attr", unfused=True),
    R("CD", "ocean", 2.0e-3, unfused=True), R("r_bot", "ocean", 4.0e-5, unfused=True), R("rho_a_ocean", "ocean", 1.0, unfused=True),
    R("vcap", "ocean", 10.0, unfused=True), R("tau_scale", "ocean", 0.3, unfused=True),
    R("polar_sponge_lat", "ocean", 60.0, unfused=True), R("polar_sponge_gain", "ocean", 1.0e-4, unfused=True),
    R("K_h", "ocean", 8.0e3, unfused=True), R("sigma4_ocean", "ocean", 0.03, unfused=True),
    R("ocean_cfl", "ocean", 0.03, unfused=True), R("ocean_max_u", "ocean", 0.3, unfused=True),
    R("ocean_k4_u", "ocean", 1.0e15, unfused=True), R("ocean_k4_v", "ocean", 1.0e15, unfused=True),
    R("ocean_k4_eta", "ocean", 1.0e15, unfused=True), R("ocean_adv_alpha", "ocean", 0.5, unfused=True),
    R("ocean_ice_qfac", "ocean", 0.6, SHALLOW, unfused=True), R("eta_cap", "ocean", 0.3, unfused=True),
    R("ts_min", "ocean", 270.0, unfused=True), R("ts_max", "ocean", 295.0, unfused=True),
    # ---- driver-side physics: only the reference's driver script reads these (device vs oracle; pinned by A5/A6)
    R("alpha_water", "driver", 0.15, {"use_topo_albedo": 0}), R("alpha_ice", "driver", 0.5), R("alpha_cloud", "driver", 0.4),
    R("pref", "driver", 1e-5), R("cmax", "driver", 0.8), R("w_mem", "driver", 0.5),
    R("w_p", "driver", 0.3), R("w_src", "driver", 0.3), R("cloud_from_p_floor", "driver", 0.6),
    R("cloud_adv_alpha", "driver", 0.5), R("cloud_smooth_sigma", "driver", 0.4),
    R("runoff_tau_days", "driver", 5.0), R("wland_cap_mm", "driver", 30.0), R("snow_thresh_K", "driver", 271.15),
    R("snow_melt_rate_mm_day", "driver", 8.0, {"snow_melt_mode": 1}), R("snow_t_band_K", "driver", 2.5),
    R("snow_ddf_mm_per_k_day", "driver", 4.5), R("snow_melt_tref_K", "driver", 270.15), R("swe_ref_mm", "driver", 10.0),
    R("swe_max_mm", "driver", 25.0), R("snow_albedo_fresh", "driver", 0.8), R("lapse_k_kpm", "driver", 8.0),
    R("land_elev_max_m", "driver", 1500.0), R("polar_ice_thick_max_m", "driver", 50.0), R("polar_lat_thresh", "driver", 68.0, {"polar_ice_thick_max_m": 50.0}),
    R("rho_snow", "driver", 250.0), R("glacier_frac", "driver", 0.3), R("glacier_swe_mm", "driver", 5.0),
    R("qnet_lw_eps0", "driver", 0.61, QNET), R("qnet_lw_kc", "driver", 0.12, QNET),
    # ---- the hybrid precipitation on its own (one driver_physics call): arguments of the reference's function, and the three
    # variables it reads itself (physics.py:330-352); the dynamic fallback runs while the mean P_cond is below pq_min
    R("orog_k", "orog", 0.08, how="arg"), R("D_crit", "orog", -2e-7, how="arg"), R("p_betadiv", "orog", 0.6, how="arg"),
    R("k_precip", "orog", 1.5e5, FALLBACK, how="arg"), R("pq_min", "orog", 1e-3), R("p_blend", "orog", 0.4, FALLBACK),
    # ---- int switches
    R("seaice_enabled", "column", 0), R("cloud_couple", "column", 0), R("lw_v2", "column", 0), R("gh_lock", "column", 0),
    R("polar_freeze_fix_s", "column", 0), R("polar_freeze_fix_n", "column", 0),
    R("mom_scheme", "column", 1, unfused=True), R("diff_enable", "column", 0, unfused=True),
    R("filter_type", "column", "hyper4", SPEC, unfused=True), R("filter_type", "column", "shapiro", unfused=True),
    R("filter_type", "column", "spectral", SPEC, unfused=True),
    R("diff_every", "column", 2, unfused=True), R("k4_nsub", "column", 2, {"k4_u": 1.0e15}, unfused=True),
    R("diff_q", "column", 1, unfused=True), R("diff_cloud", "column", 1, unfused=True),
    R("shapiro_every", "column", 2, unfused=True), R("shapiro_n", "column", 1, {"shapiro_every": 2}, unfused=True),
    R("spec_every", "column", 2, unfused=True),
    R("ocean_k4_nsub", "ocean", 2, unfused=True), R("ocean_diff_every", "ocean", 2, unfused=True),
    R("ocean_shapiro_n", "ocean", 1, {"ocean_shapiro_every": 2}, unfused=True),
    R("ocean_shapiro_every", "ocean", 2, {"ocean_shapiro_n": 1}, unfused=True),
    R("ocean_outlier", "ocean", "clamp", {"ocean_max_u": 0.3}, unfused=True), R("ocean_use_qnet", "ocean", 0, SHALLOW, unfused=True),
    R("ocean_polar_fix", "ocean", 0, unfused=True),
    R("p_hybrid_fallback", "orog", 0, FALLBACK), R("cloud_advect", "driver", 0), R("use_topo_albedo", "driver", 0),
    R("snow_melt_mode", "driver", 1), R("swe_enable", "driver", 0), R("lapse_enable", "driver", 0),
    R("orog_enable", "orog", 0, how="arg"),
]

# the same rows (value, companions) on the CPU-only hydro scenario: digests of the reference's hydrology functions
PIN_ROWS = [dict(r, scenario="hydro", fixture=True, how="env", pin=None) for r in ROWS if r["param"] in HYDRO_PARAMS]

# Parameters the reference's path reads but whose value it then never uses on any entry point the product mirrors.
# name -> (scenario to show it on, perturbed value, reference file:line)
DEAD = {
    "Cs_ice": ("column", 6e6, "pygcm/energy.py:371 and 416: under ice the melt / freeze blocks (353-368) leave no residual flux for "
                              "C_s_ice to divide, and where they do not the result is capped at t_freeze (416)"),
    "eps_default": ("column", 0.90, "pygcm/dynamics.py:366-369: QD_EPS_DEFAULT is read only when the model has no land mask; "
                                     "every caller (run_simulation.py:1266, benchmark_jax.py) passes one"),
}

# Not parameters of the arithmetic.
EXEMPT = {
    "has_csmap": "set by the SpectralModel constructor from whether a C_s map was handed over; not a tunable",
    "a": "planet radius: a constant of the reference (pygcm/constants.py:32), no variable or argument sets it",
    "omega": "planet rotation rate: a constant of the reference (pygcm/constants.py:34), no variable or argument sets it",
}

# the four parameters whose environment variable is a word, not a number (qingdai_amd.params._env_int)
STRING_ENV = {
    "mom_scheme": {0: "geos", 1: "primitive"},
    "filter_type": {"combo": "combo", "hyper4": "hyper4", "shapiro": "shapiro", "spectral": "spectral"},
    "ocean_outlier": {"mean4": "mean4", "clamp": "clamp"},
    "snow_melt_mode": {0: "degree_day", 1: "constant"},
}


def env_name(param):
    from qingdai_amd.params import _DOUBLES, _INTS
    for n, env, _ in _DOUBLES + _INTS:
        if n == param:
            return env
    raise KeyError(param)


def env_value(param, value):
    """The string the reference (and QdParams.from_env) reads for `value`."""
    if param in STRING_ENV:
        return STRING_ENV[param][value]
    return repr(value) if isinstance(value, float) else str(value)


def row_tol(row):
    tol = dict(SCENARIOS[row["scenario"]]["fields"])
    if row["tol"]:
        tol.update(row["tol"])
    return tol


def fixture_name(scenario):
    return f"param_sweep_{scenario}_{SHAPE[0]}x{SHAPE[1]}"


def fixture_rows(scenario):
    return [r for r in ROWS + PIN_ROWS if r["scenario"] == scenario and r["fixture"]]
