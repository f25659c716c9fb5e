"""The ragged grid shapes at which the fused step kernels change form, what each shape is there for, and the form report
(Device.step_forms) each one must give.  Shared by tests/test_gpu_step_forms.py (device against oracle, form against form) and
tests/test_step_form_cases_cpu.py (fixtures, oracle sensitivities, coverage of the table).  Test infrastructure only.

The launchers' thresholds the table is built around (qingdai_amd/csrc):
  k_dyn_stream / k_ocn_stream   n_lon >= 64 and n_lat >= 12; column strips of 58; row strips min(target / ntc, n_lat // 12); vb trims the
                                north-pole strip
  k_dyn_hyper / k_ocn_hyper     everything else: tiles of TR x 58; their FAST path needs n_lon >= 64 and TR + 10 rows
  ocean tail                    one launch from 64 columns: k_ocn_tail_fast (groups of 60, pole strips of 3 rows, middle strips of >= 7)
                                or k_ocn_tail_stream (QD_TAIL_V=1, groups of 62); else k_cont_sstadv + k_sst_outlier_fused
  k_ocn_fused (QD_OCN_FUSED=1)  n_lat >= 38
"""
import numpy as np

STEP_TOL = 1e-9            # tests/test_gpu_parity.py
TAIL_TOL = 1e-11           # tests/test_gpu_bands.py
NSTEPS, DT = 3, 300.0
# the atmosphere step from the wet / cloudy / icy state: two steps.  Over three the oracle's own condensation diagnostics
# (P_cond_flux_last, LH_release_last) move by up to 2.3e-11 when the wind is perturbed by 1e-15, over two by <= 5e-12
# (tests/test_step_form_cases_cpu.py holds them to 1e-11, 100 x below STEP_TOL)
ATM_NSTEPS = 2

ALL = ("QD_FUSED=0", "QD_FUSED_FAST=0", "QD_OCN_TAIL=0", "QD_TAIL_GENERAL=1", "QD_TAIL_FIX=0", "QD_MEAN_IN_MOMENTUM=0", "QD_TAIL_V=1")
# QD_FUSED_FAST=3 (the tile kernels with their FAST path) is the one way to the tile FAST path on a grid the streaming form takes
ALL3 = ALL + ("QD_FUSED_FAST=3",)

# shape -> fixture (seed, ocean_cfl of oracle/gen_golden.py FORM_SHAPES) or None, the switches to cross, the form report of the
# DEFAULT handle after a coupled step with n_sub >= 2 (keys of Device.step_forms), the width of the last column strip of the
# momentum kernels (58 per strip) and of the last column group of the tail (60; QD_TAIL_V=1: 62), and what the row is for.
CASES = {
    (11, 63): dict(fixture=(111, 0.05), cfl=0.05, switches=("QD_FUSED=0",), last_strip=5, last_group=None,
                   forms=dict(dyn_stream=0, ocn_stream=0, tile_tr=6, tile_ntr=2, tile_ntc=2, tile_dyn_fast=0, tile_ocn_fast=0, tail_kernel=0,
                              last_use_tail=0, last_tail_kernel=0, last_mean_form=0, last_dyn_form=2, last_ocn_form=2, fused_ok=0),
                   why="tile kernels, EXACT path, two column tiles (58 + 5); two-launch ocean tail (n_lon < 64)"),
    (47, 61): dict(fixture=(112, 0.05), cfl=0.05, switches=("QD_FUSED=0",), last_strip=3, last_group=None,
                   forms=dict(dyn_stream=0, ocn_stream=0, tile_tr=6, tile_ntr=8, tile_ntc=2, tile_dyn_fast=0, tail_kernel=0,
                              last_use_tail=0, last_tail_kernel=0, last_mean_form=0, last_dyn_form=2, last_ocn_form=2, fused_ok=0),
                   why="tile kernels, eight row tiles with a ragged last one (7 x 6 + 5), column tiles 58 + 3"),
    (11, 64): dict(fixture=None, cfl=0.05, switches=("QD_OCN_TAIL=0", "QD_TAIL_GENERAL=1"), last_strip=6, last_group=4,
                   forms=dict(dyn_stream=0, ocn_stream=0, tile_tr=6, tile_ntr=2, tile_ntc=2, tile_dyn_fast=0, tail_kernel=1, tail_ntc=2,
                              tail_pole=2, tail_mid=1, tail_r=7, tail_rp=3, last_use_tail=1, last_tail_acc=1, last_mean_form=0,
                              last_dyn_form=2, last_ocn_form=2, fused_ok=0),
                   why="n_lat < 12: tile momentum with the one-launch tail; pole strips 3 + 3, one middle strip of 5 rows"),
    (12, 64): dict(fixture=(113, 0.05), cfl=0.05, switches=("QD_FUSED_FAST=0", "QD_FUSED=0"), last_strip=6, last_group=4,
                   forms=dict(dyn_stream=1, ocn_stream=1, dyn_ntc=2, dyn_nrs=1, dyn_r=12, dyn_vb=0, ocn_ntc=2, ocn_nrs=1, ocn_r=12, ocn_vb=0,
                              tail_kernel=1, tail_ntc=2, tail_pole=2, tail_mid=1, last_use_tail=1, last_mean_form=1, last_fix_now=0,
                              last_tail_kernel=1, last_dyn_form=1, last_ocn_form=1, fused_ok=0),
                   why="the smallest streaming grid: one row strip, column strips 58 + 6"),
    (13, 65): dict(fixture=(114, 0.05), cfl=0.05, switches=ALL, last_strip=7, last_group=5,
                   forms=dict(dyn_stream=1, ocn_stream=1, dyn_ntc=2, dyn_nrs=1, dyn_r=13, dyn_vb=0, ocn_ntc=2, ocn_nrs=1,
                              tail_kernel=1, tail_ntc=2, tail_pole=2, tail_mid=1, last_use_tail=1, last_mean_form=1, last_fix_now=0,
                              last_tail_kernel=1, last_dyn_form=1, last_ocn_form=1, fused_ok=0),
                   why="odd n_lon: column strips 58 + 7, tail groups 60 + 5"),
    (25, 117): dict(fixture=(115, 0.1), cfl=0.1, switches=ALL3, last_strip=1, last_group=57,
                    forms=dict(dyn_stream=1, ocn_stream=1, dyn_ntc=3, dyn_nrs=2, dyn_r=13, dyn_vb=2, ocn_ntc=3, ocn_nrs=2, ocn_r=13, ocn_vb=2,
                               tail_kernel=1, tail_ntc=2, tail_pole=2, tail_mid=3, tail_r=7, last_use_tail=1, last_mean_form=1,
                               last_tail_kernel=1, last_dyn_form=1, last_ocn_form=1, fused_ok=0),
                    why="two streaming row strips with the vb pole trim; 2 x 58 + 1 columns: a one-column last strip"),
    (29, 121): dict(fixture=(116, 0.1), cfl=0.1, switches=ALL3, last_strip=5, last_group=1,
                    forms=dict(dyn_stream=1, ocn_stream=1, dyn_ntc=3, dyn_nrs=2, dyn_r=15, dyn_vb=6, tail_kernel=1, tail_ntc=3, tail_pole=2,
                               tail_mid=4, tail_r=7, last_use_tail=1, last_mean_form=1, last_tail_kernel=1, last_dyn_form=1, last_ocn_form=1,
                               fused_ok=0),
                    why="2 x 60 + 1 columns: a one-column last group in k_ocn_tail_fast; four middle strips, the last of 2 rows"),
    (27, 125): dict(fixture=None, cfl=0.1, switches=("QD_TAIL_V=1", "QD_OCN_TAIL=0"), last_strip=9, last_group=5,
                    forms=dict(dyn_stream=1, ocn_stream=1, dyn_ntc=3, dyn_nrs=2, dyn_vb=4, tail_kernel=1, tail_ntc=3, last_use_tail=1,
                               last_mean_form=1, last_tail_kernel=1, fused_ok=0),
                    why="2 x 62 + 1 columns: a one-column last group in k_ocn_tail_stream (QD_TAIL_V=1)"),
    (37, 64): dict(fixture=None, cfl=0.1, switches=("QD_OCN_FUSED=1",), last_strip=6, last_group=4,
                   forms=dict(dyn_stream=1, ocn_stream=1, dyn_nrs=3, dyn_vb=1, tail_kernel=1, fused_ok=0, last_use_fused1=0),
                   why="k_ocn_fused refused one row below its threshold"),
    (38, 65): dict(fixture=None, cfl=0.1, switches=("QD_OCN_FUSED=1",), last_strip=7, last_group=5,
                   forms=dict(dyn_stream=1, ocn_stream=1, dyn_nrs=3, dyn_vb=2, tail_kernel=1, fused_ok=1, fused_ntc=2, fused_nmid=2, fused_r=12,
                              last_use_fused1=0),
                   why="k_ocn_fused accepted at its 38-row threshold"),
}
SHAPES = tuple(CASES)
FIXTURE_SHAPES = tuple(s for s in SHAPES if CASES[s]["fixture"])
COUPLED_SHAPES = ((13, 65), (25, 117), (29, 121))
MODE_SHAPES = ((13, 65), (25, 117))          # filter_type=hyper4 and mom_scheme=1 (k_dyn_stream<true>) are repeated here

# what a switch changes in the form report of the row's default handle (after the same coupled steps); a value may depend on the row
SWITCH_FORMS = {
    "QD_FUSED=0": dict(last_dyn_form=0, last_ocn_form=0, last_use_tail=0, last_tail_kernel=0, last_mean_form=0),
    "QD_FUSED_FAST=0": dict(dyn_stream=0, ocn_stream=0, last_dyn_form=2, last_ocn_form=2, tile_dyn_fast=0, tile_ocn_fast=0, last_mean_form=0),
    "QD_FUSED_FAST=3": dict(dyn_stream=0, ocn_stream=0, last_dyn_form=2, last_ocn_form=2, last_mean_form=0),
    "QD_OCN_TAIL=0": dict(tail_kernel=0, last_use_tail=0, last_tail_kernel=0, last_mean_form=0),
    "QD_TAIL_GENERAL=1": dict(tail_general=1),
    "QD_TAIL_FIX=0": dict(last_fix_now=0),
    "QD_MEAN_IN_MOMENTUM=0": dict(last_mean_form=0),
    "QD_TAIL_V=1": dict(tail_kernel=2, tail_pole=0, tail_rp=0, tail_r=7, last_tail_kernel=3, last_mean_form=0),
    "QD_OCN_FUSED=1": dict(),                                 # by the row: (37, 64) refuses, (38, 65) takes k_ocn_fused
}
# entries of the default report a switch may move that the row did not pin (strip counts of another kernel, the fix list's own policy)
SWITCH_FREE = {
    "QD_FUSED=0": ("last_fix_now",),
    "QD_OCN_TAIL=0": ("last_fix_now",),
    "QD_TAIL_V=1": ("tail_ntc", "tail_mid", "last_fix_now"),
    "QD_FUSED_FAST=3": ("tile_dyn_fast", "tile_ocn_fast", "last_fix_now", "last_tail_kernel"),
    "QD_FUSED_FAST=0": ("last_fix_now", "last_tail_kernel"),
    "QD_MEAN_IN_MOMENTUM=0": ("last_fix_now", "last_tail_kernel"),
    "QD_TAIL_FIX=0": ("last_tail_kernel",),
    "QD_OCN_FUSED=1": ("last_use_fused1", "last_tail_kernel", "last_mean_form", "last_fix_now", "last_ocn_form"),
}

# Coupled loop (DriverOracle against itself, initial zonal wind scaled by 1 + 1e-15, three steps): the largest deviation of uo, vo,
# eta relative to each field's max-norm, measured on the CPU by coupled_sensitivity() below and recomputed by
# tests/test_step_form_cases_cpu.py (it fails when one has drifted by more than 10 x).
COUPLED_SENS = {(13, 65): 5.7e-16, (25, 117): 4.4e-16, (29, 121): 1.8e-15}


def coupled_bound(shape):
    """Bound on uo, vo, eta of the device against DriverOracle: 1000 x the oracle's own sensitivity (a device rounding difference of
    a few hundred ulp entering at each of the three steps), not below STEP_TOL, not above the 1e-7 of the 61 x 96 test."""
    return min(1e-7, max(STEP_TOL, 1000.0 * COUPLED_SENS[tuple(shape)]))


def run_cfl(shape):
    """ocean_cfl of the coupled form-against-form runs (moderate winds: the gravity-wave speed sets the count): the one that gives
    ceil(2.5) = 3 sub-steps from cg alone, by ocean.py:293-303 -- n_sub = ceil(max(cg, |u|) dt / dx_min / cfl)"""
    import qd_oracle as qo
    P = qo.defaults()
    dlat, dlon = np.pi / (shape[0] - 1), 2 * np.pi / shape[1]
    dx_min = min(P.a * dlat, P.a * dlon * 0.5)
    return float(np.sqrt(P.g_ocean * 50.0) * DT / dx_min / 2.5)


def env_of(switches):
    return dict(s.split("=") for s in switches)


def last_widths(nlon):
    """Width of the last column strip of the momentum kernels (58), of k_ocn_tail_fast's last group (60), of k_ocn_tail_stream's (62)"""
    return tuple(nlon - (-(-nlon // w) - 1) * w for w in (58, 60, 62))


# ---------------------------------------------------------------- states
def perturbed_state(shape, seed, wet=False, cloudy=False, icy=False):
    """The seeded state of oracle/gen_golden.py (perturbed_state), restated: the *_forms fixtures start from it."""
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


def seed_of(shape):
    fx = CASES[tuple(shape)]["fixture"]
    return fx[0] if fx else 200 + shape[0] + shape[1]


def ts_case(shape, over=None):
    """(meta, d) of util.run_device_time_step / run_oracle_time_step: ATM_NSTEPS steps, energy_w = 1, albedo passed, wet / cloudy / icy"""
    o = {"energy_w": 1.0}
    o.update(over or {})
    st = perturbed_state(shape, seed_of(shape), wet=True, cloudy=True, icy=True)
    meta = dict(nlat=shape[0], nlon=shape[1], nsteps=ATM_NSTEPS, dt=DT, over=o, with_albedo=True)
    return meta, {"init_" + k: v for k, v in st.items()}


def ocean_case(shape):
    """Inputs of the three full ocean steps (oracle/gen_golden.py: case_ocean with strong=True), restated"""
    from util import surface
    nlat, nlon = shape
    g, mask, _, _ = surface(nlat, nlon)
    seed = seed_of(shape) + 100
    st = perturbed_state(shape, seed, icy=True)
    r = np.random.default_rng(seed + 3)
    Q_net = 120.0 * np.cos(np.deg2rad(g.lat_mesh)) - 60.0 + r.normal(0, 5.0, mask.shape)
    d = dict(u_atm=st["u"] * 4.0, v_atm=st["v"] * 4.0, Q_net=Q_net, ice_mask=st["h_ice"] > 0.0, init_Ts=np.where(mask == 0, st["T_s"], 288.0))
    d["init_uo"] = np.where(mask == 0, 0.3 * np.cos(np.deg2rad(g.lat_mesh)) + r.normal(0, 0.05, mask.shape), 0.0)
    d["init_vo"] = np.where(mask == 0, r.normal(0, 0.05, mask.shape), 0.0)
    d["init_eta"] = np.where(mask == 0, r.normal(0, 0.2, mask.shape), 0.0)
    return mask, d


def fast_ocean_state(shape):
    """The state of test_ocean_single_substep_every_row_vs_oracle_at_721x1440, at `shape`: currents up to the 3 m/s cap with fast pole
    rows, eta inside its clip, a warm-pool SST, a 250 m/s jet, Q_net with an ice mask."""
    from util import surface
    nlat, nlon = shape
    g, mask, _, _ = surface(nlat, nlon)
    ocean = mask == 0
    lat = np.deg2rad(g.lat_mesh); lon = np.deg2rad(g.lon_mesh)
    r = np.random.default_rng(5)
    uo = (2.6 * np.cos(lat) ** 0.25 * np.sin(2 * lon + lat) + 0.6 * r.standard_normal(shape)) * ocean
    vo = (2.2 * np.cos(3 * lon) * np.cos(lat) ** 0.25 + 0.6 * r.standard_normal(shape)) * ocean
    uo[[0, 1, -2, -1]] = 4.0 * ocean[[0, 1, -2, -1]]
    vo[[0, -1]] = -3.0 * ocean[[0, -1]]
    eta = (3.0 * np.sin(3 * lat) * np.cos(2 * lon) + 0.5 * r.standard_normal(shape)) * ocean
    sst = 288.0 + 12.0 * np.cos(lat) ** 2 + 1.5 * np.sin(4 * lon)
    u_atm = 250.0 * np.cos(lat) * (1.0 + 0.1 * np.sin(3 * lon)); v_atm = 60.0 * np.sin(2 * lat) * np.cos(2 * lon)
    qnet = 150.0 * np.cos(lat) - 60.0 + 20.0 * r.standard_normal(shape)
    ice = (np.abs(np.rad2deg(lat)) > 72.0) & ocean
    return mask, dict(uo=uo, vo=vo, eta=eta, sst=sst, u_atm=u_atm, v_atm=v_atm, qnet=qnet, ice=ice)


# ---------------------------------------------------------------- the coupled loop
def coupled_state(shape, land_mask):
    """test_driver_loop_vs_oracle's cold, low-h state (the snow branches fire), with a smooth wind so that the ocean is driven from the
    first step and a relative perturbation of the wind means something"""
    import qd_oracle as qo
    g = qo.Grid(*shape)
    lat, lon = np.deg2rad(g.lat_mesh), np.deg2rad(g.lon_mesh)
    return dict(h=8000.0 - 10500.0 * np.sin(lat) ** 2, T_s=262.0 + 36.0 * np.cos(lat) ** 2,
                S_snow=np.where((land_mask == 1) & (np.abs(np.rad2deg(lat)) > 55), 30.0, 0.0),
                u=25.0 * np.cos(lat) * np.sin(2 * lon), v=8.0 * np.sin(2 * lat) * np.cos(3 * lon))


def coupled_oracle(shape, land_mask, base_albedo, friction, scale=1.0):
    """DriverOracle on coupled_state, three steps; returns the oracle objects (atmosphere, ocean, driver)"""
    import qd_oracle as qo
    from qd_oracle.driver import DriverOracle
    nlat, nlon = shape
    st = coupled_state(shape, land_mask)
    g = qo.Grid(nlat, nlon)
    P = qo.defaults()
    m = qo.AtmosOracle(g, friction, land_mask, P, C_s_map=np.where(land_mask == 1, 3e6, P.Cs_ocean).astype(float))
    m.h, m.T_s, m.u, m.v = st["h"].copy(), st["T_s"].copy(), st["u"] * scale, st["v"].copy()
    oc = qo.OceanOracle(g, land_mask, P, init_Ts=np.full((nlat, nlon), 288.0))
    d = DriverOracle(g, m, oc, qo.Forcing(g), land_mask, base_albedo, P)
    d.S_snow = st["S_snow"].copy()
    for i in range(NSTEPS):
        d.step(i * DT, DT)
    return m, oc, d


def coupled_sensitivity(shape):
    """max over uo, vo, eta of |oracle(u0) - oracle(u0 (1 + 1e-15))| / max|field| after the three coupled steps, and the same of the
    atmosphere / surface fields"""
    from util import surface, relerr
    _, mask, alb, fric = surface(*shape)
    a = coupled_oracle(shape, mask, alb, fric)
    b = coupled_oracle(shape, mask, alb, fric, scale=1.0 + 1e-15)
    ocn = max(relerr(getattr(a[1], k), getattr(b[1], k)) for k in ("uo", "vo", "eta"))
    atm = max(relerr(getattr(a[0], k), getattr(b[0], k)) for k in ("u", "v", "h", "T_s", "q", "cloud_cover"))
    return ocn, atm
