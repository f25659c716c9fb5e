"""
qingdai_amd/topogen.py -- the procedural planet (P004, pygcm/topography.py:58-346, scripts/generate_topography.py) built on the device.

The reference's recipe is generalized-Gaussian continents blended with very-low-frequency noise, fBm octaves of Gaussian-filtered
white noise, a normalisation after every stage, and a cos(lat)-weighted quantile sea level.  `generate` makes the random draws on
the host in the reference's order (`draw`: NumPy's default_rng stream cannot be reproduced on the device), hands them with the
Gaussian weights and the trigonometric tables to qd_topogen_build (qingdai_amd/csrc/qd_topogen.hip) and returns the elevation,
the land mask and the sea level.  The filter (`smooth`) is bit-identical to topography._smooth; the elevation agrees with the host
recipe to about 1e-11 m (blocked instead of pairwise means, the device's exp / arccos), so the mask can differ from the host's
only in a cell whose elevation lies that close to sea level.  `write_topography` writes the reference's multi-field file, which
QD_TOPO_NC loads; scripts/generate_topography.py is the CLI.
"""
from __future__ import annotations

import numpy as np

from ._lib import C, OUT
from .params import PLANET_OMEGA, PLANET_RADIUS
from .topography import _kernel

PLANET_AXIAL_TILT = 27.0                      # constants.py:35
MAX_OCTAVES = C["QD_TOPOGEN_MAX_OCTAVES"]
MAX_CONTINENTS = C["QD_TOPOGEN_MAX_CONTINENTS"]

# generate_elevation_map's params (topography.py:101-109, 160-167, 183-186, 235-241); None: derived from the grid
DEFAULTS = {"N_CONTINENTS": 3, "CONTINENT_SIGMA_DEG": 30.0, "CONTINENT_SHAPE_P": 2.0, "CONTINENT_AMP_RANGE": (0.8, 1.2),
            "CONT_MIN_DIST_DEG": 0.0, "VLF_SIGMA_LAT": None, "VLF_SIGMA_LON": None, "W_VLF": 0.35, "FBM_OCTAVES": 5, "HURST_H": 0.8,
            "FBM_BASE_SIGMA_LAT": None, "FBM_BASE_SIGMA_LON": None, "W1": 1.0, "W3": 0.6, "SCALE_M": 4500.0}

# scripts/generate_topography.py:61-78: variable -> (params key or None, type, default)
ENV = (("QD_SEED", None, int, 42), ("QD_TARGET_LAND_FRAC", None, float, 0.40),
       ("QD_N_CONTINENTS", "N_CONTINENTS", int, 3), ("QD_CONT_SIGMA_DEG", "CONTINENT_SIGMA_DEG", float, 30.0),
       ("QD_CONT_SHAPE_P", "CONTINENT_SHAPE_P", float, 2.0), ("QD_CONT_MIN_DIST_DEG", "CONT_MIN_DIST_DEG", float, 40.0),
       ("QD_W_VLF", "W_VLF", float, 0.35), ("QD_FBM_OCTAVES", "FBM_OCTAVES", int, 5), ("QD_HURST_H", "HURST_H", float, 0.8),
       ("QD_W1", "W1", float, 1.0), ("QD_W3", "W3", float, 0.6), ("QD_SCALE_M", "SCALE_M", float, 4500.0))


class TopoGenError(RuntimeError):
    pass


def _env_value(env, name, kind, default):
    try:
        return kind(env.get(name, default))
    except Exception:
        return default


def params_from_env(env):
    """-> (seed, target_land_frac, params): the CLI's variables with its defaults; a value that does not parse is the default."""
    seed = _env_value(env, "QD_SEED", int, 42)
    target = _env_value(env, "QD_TARGET_LAND_FRAC", float, 0.40)
    params = {key: _env_value(env, name, kind, default) for name, key, kind, default in ENV if key is not None}
    return seed, target, params


def _resolved(grid, params):
    p = dict(params or {})
    unknown = set(p) - set(DEFAULTS)
    if unknown:
        raise TopoGenError(f"unknown topography parameters: {sorted(unknown)}")
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    derived = {"VLF_SIGMA_LAT": max(4, n_lat // 12), "VLF_SIGMA_LON": max(8, n_lon // 12),
               "FBM_BASE_SIGMA_LAT": max(1, n_lat // 20), "FBM_BASE_SIGMA_LON": max(1, n_lon // 20)}
    out = {}
    for k, d in DEFAULTS.items():
        v = p.get(k, derived[k] if d is None else d)
        out[k] = int(v) if k in ("N_CONTINENTS", "FBM_OCTAVES") else (tuple(v) if k == "CONTINENT_AMP_RANGE" else float(v))
    return out


def _spaced_centres(rng, n, min_dist_deg):
    """The rejection loop of topography.py:114-145: area-uniform candidates, kept when at least min_dist_deg of great circle from
    every centre kept so far; after 10000 candidates the rest is drawn without spacing."""
    lats, lons = [], []
    tries = 0
    while len(lats) < n and tries < 10000:
        la = np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0)))
        lo = rng.uniform(0.0, 360.0)
        a1, o1 = np.deg2rad(la), np.deg2rad(lo)
        far = True
        for lb, ob in zip(lats, lons):
            a2, o2 = np.deg2rad(lb), np.deg2rad(ob)
            cosd = np.clip(np.sin(a1) * np.sin(a2) + np.cos(a1) * np.cos(a2) * np.cos(o1 - o2), -1.0, 1.0)
            if np.rad2deg(np.arccos(cosd)) < min_dist_deg:
                far = False
                break
        if far:
            lats.append(la)
            lons.append(lo)
        tries += 1
    if len(lats) < n:
        rest = n - len(lats)
        lats.extend(list(np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0, size=rest)))))
        lons.extend(list(rng.uniform(0.0, 360.0, size=rest)))
    return np.asarray(lats[:n], dtype=float), np.asarray(lons[:n], dtype=float)


def draw(grid, seed=42, params=None):
    """The reference's random draws in its order -> dict: cont_lats, cont_lons (deg), cont_amps, vlf_noise [n_lat, n_lon] from
    default_rng(seed) (topography.py:99-162) and octave_noise [FBM_OCTAVES, n_lat, n_lon] from default_rng(seed + 1) (:181-193)."""
    p = _resolved(grid, params)
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    n, octaves = p["N_CONTINENTS"], p["FBM_OCTAVES"]
    if n < 0 or octaves < 0:
        raise TopoGenError("N_CONTINENTS and FBM_OCTAVES must not be negative")
    rng = np.random.default_rng(int(seed))
    if p["CONT_MIN_DIST_DEG"] <= 0.0:
        lats = np.rad2deg(np.arcsin(rng.uniform(-1.0, 1.0, size=n)))
        lons = rng.uniform(0.0, 360.0, size=n)
    else:
        lats, lons = _spaced_centres(rng, n, p["CONT_MIN_DIST_DEG"])
    a_min, a_max = p["CONTINENT_AMP_RANGE"]
    amps = rng.uniform(a_min, a_max, size=n)
    vlf = rng.standard_normal(size=(n_lat, n_lon))
    rng3 = np.random.default_rng(int(seed) + 1)
    octs = np.empty((octaves, n_lat, n_lon), dtype=np.float64)
    for k in range(octaves):
        octs[k] = rng3.standard_normal(size=(n_lat, n_lon))
    return {"cont_lats": lats, "cont_lons": lons, "cont_amps": amps, "vlf_noise": vlf, "octave_noise": octs}


def _half_kernel(sigma):
    """(w[0 .. r], r): the first half of topography._kernel's weights, the centre last"""
    w = _kernel(float(sigma))
    r = (len(w) - 1) // 2
    return np.ascontiguousarray(w[:r + 1], dtype=np.float64), r


class _Handle:
    """dev, the grid's own device, or a fresh one that is closed (and taken off the grid again) on exit"""

    def __init__(self, grid, dev, device=0):
        self.grid, self.dev, self.own, self.device = grid, dev, False, device

    def __enter__(self):
        if self.dev is None:
            self.dev = getattr(self.grid, "_device", None)
        if self.dev is None:
            from .device import Device
            self.dev, self.own = Device(self.grid, device=self.device), True
        return self.dev

    def __exit__(self, *exc):
        if self.own:
            self.dev.close()
            self.grid._device = None
        return False


def smooth(field, sig_lat, sig_lon, dev=None, grid=None, lds_bytes=0):
    """gaussian_filter(field, (sig_lat, sig_lon), mode=("nearest", "wrap")) on the device, bit-identical to topography._smooth.
    `dev`: a whole-globe Device of the field's shape (or `grid` to make one).  lds_bytes: the LDS a workgroup may stage a row or
    a column strip in (0: 64 KiB); a line that does not fit is filtered from global memory."""
    f = np.ascontiguousarray(np.asarray(field, dtype=np.float64))
    if f.ndim != 2:
        raise TopoGenError(f"field must be 2-D, got shape {f.shape}")
    if dev is None and grid is None:
        raise TopoGenError("smooth needs a device or a grid")
    with _Handle(grid, dev) as d:
        if f.shape != tuple(d.shape):
            raise TopoGenError(f"field shape {f.shape} != grid shape {tuple(d.shape)}")
        wa, ra = _half_kernel(sig_lat)
        wo, ro = _half_kernel(sig_lon)
        out = np.empty_like(f)
        d.call("qd_topogen_smooth", f.shape[0], f.shape[1], f, wa, ra, wo, ro, lds_bytes, out, error=TopoGenError)
    return out


def land_fraction(mask, grid):
    """the achieved fraction as create_land_sea_mask_from_elevation reports it (topography.py:262-274)"""
    w = np.maximum(np.cos(np.deg2rad(grid.lat_mesh)), 0.0)
    return float((w * (np.asarray(mask) == 1)).sum() / (w.sum() + 1e-15))


def build_inputs(grid, params, draws, target_land_frac):
    """What qd_topogen_build takes, as the reference's NumPy rounds it -> dict: par, oct_amp, noise, cont, cont_coslon, sin_lat,
    cos_lat, area_w, radii, weights (include/qingdai_hip.h) and the drawn cont_lats / cont_lons / cont_amps."""
    p = _resolved(grid, params)
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    n_cont, n_oct = p["N_CONTINENTS"], p["FBM_OCTAVES"]
    if not 0 <= n_cont <= MAX_CONTINENTS:
        raise TopoGenError(f"N_CONTINENTS {n_cont} outside [0, {MAX_CONTINENTS}]")
    if not 0 <= n_oct <= MAX_OCTAVES:
        raise TopoGenError(f"FBM_OCTAVES {n_oct} outside [0, {MAX_OCTAVES}]")
    d = draws
    vlf = np.asarray(d["vlf_noise"], dtype=np.float64)
    octs = np.asarray(d["octave_noise"], dtype=np.float64)
    lats, lons, amps = (np.asarray(d[k], dtype=np.float64) for k in ("cont_lats", "cont_lons", "cont_amps"))
    if vlf.shape != (n_lat, n_lon) or octs.shape != (n_oct, n_lat, n_lon):
        raise TopoGenError(f"noise shapes {vlf.shape}, {octs.shape} do not fit the grid {(n_lat, n_lon)} with {n_oct} octaves")
    if not (lats.shape == lons.shape == amps.shape == (n_cont,)):
        raise TopoGenError(f"centres / amplitudes do not hold {n_cont} continents")
    noise = np.empty((1 + n_oct, n_lat, n_lon), dtype=np.float64)
    noise[0] = vlf
    noise[1:] = octs
    # the operands of _great_circle_distance_rad (topography.py:42-48) as NumPy rounds them
    lat_rad, lon_rad = np.deg2rad(np.asarray(grid.lat, dtype=np.float64)), np.deg2rad(np.asarray(grid.lon, dtype=np.float64))
    sin_lat, cos_lat = np.ascontiguousarray(np.sin(lat_rad)), np.ascontiguousarray(np.cos(lat_rad))
    area_w = np.ascontiguousarray(np.maximum(cos_lat, 0.0))
    lat0, lon0 = np.deg2rad(lats), np.deg2rad(lons)
    cont = np.ascontiguousarray(np.stack([np.sin(lat0), np.cos(lat0), amps], axis=1)) if n_cont else np.zeros((0, 3))
    coslon = np.ascontiguousarray(np.cos(lon_rad[None, :] - lon0[:, None])) if n_cont else np.zeros((0, n_lon))
    # the filters: VLF, the octaves (sigma halves, floor 0.5), the last gentle one; the octave amplitudes as the reference steps them
    sig = [(p["VLF_SIGMA_LAT"], p["VLF_SIGMA_LON"])]
    amp, amps_oct = 1.0, []
    s_lat, s_lon = p["FBM_BASE_SIGMA_LAT"], p["FBM_BASE_SIGMA_LON"]
    for _ in range(n_oct):
        sig.append((s_lat, s_lon))
        amps_oct.append(amp)
        amp *= 2 ** (-p["HURST_H"])
        s_lat, s_lon = max(0.5, s_lat / 2.0), max(0.5, s_lon / 2.0)
    sig.append((0.5, 0.5))
    for s in sig:
        if not (np.isfinite(s[0]) and np.isfinite(s[1]) and s[0] > 0.0 and s[1] > 0.0):
            raise TopoGenError(f"filter widths must be positive and finite, got {s}")
    halves = [_half_kernel(s) for pair in sig for s in pair]
    par = np.array([np.deg2rad(p["CONTINENT_SIGMA_DEG"]), p["CONTINENT_SHAPE_P"], 1 - p["W_VLF"], p["W_VLF"], p["W1"], p["W3"],
                    p["SCALE_M"], float(target_land_frac)], dtype=np.float64)
    return {"par": par, "oct_amp": np.ascontiguousarray(np.array(amps_oct, dtype=np.float64)), "noise": noise, "cont": cont,
            "cont_coslon": coslon, "sin_lat": sin_lat, "cos_lat": cos_lat, "area_w": area_w,
            "radii": np.ascontiguousarray(np.array([r for _, r in halves], dtype=np.int32)),
            "weights": np.ascontiguousarray(np.concatenate([w for w, _ in halves])),
            "cont_lats": lats, "cont_lons": lons, "cont_amps": amps}


def generate(grid, seed=42, params=None, target_land_frac=0.29, dev=None, draws=None, timing=None, device=0):
    """generate_elevation_map + create_land_sea_mask_from_elevation (topography.py:206-276) on the device -> dict: elevation f64,
    land_mask u8, sea_level_m, land_frac, cont_lats, cont_lons, cont_amps.

    params: the reference's keys (DEFAULTS).  dev: a whole-globe Device of the grid (default: the grid's own, else a fresh one,
    closed afterwards, on GPU `device`).  draws: a `draw` result to use instead of drawing; timing: a dict that receives 'kernels_ms', the event
    time of the kernels.  Raises TopoGenError for what the device refuses."""
    a = build_inputs(grid, params, draw(grid, seed, params) if draws is None else draws, target_land_frac)
    n_lat, n_lon = int(grid.n_lat), int(grid.n_lon)
    elev = np.empty((n_lat, n_lon), dtype=np.float64)
    mask = np.empty((n_lat, n_lon), dtype=np.uint8)
    with _Handle(grid, dev, device) as h:
        sea = h.call("qd_topogen_build", n_lat, n_lon, a["par"], len(a["oct_amp"]), a["oct_amp"], a["noise"], len(a["cont"]), a["cont"],
                     a["cont_coslon"], a["sin_lat"], a["cos_lat"], a["area_w"], a["radii"], a["weights"], elev, mask, OUT, error=TopoGenError)
        if timing is not None:
            timing["kernels_ms"] = h.call("qd_topogen_last_ms", OUT)
    return {"elevation": elev, "land_mask": mask, "sea_level_m": sea, "land_frac": land_fraction(mask, grid),
            "cont_lats": a["cont_lats"], "cont_lons": a["cont_lons"], "cont_amps": a["cont_amps"]}


def base_properties(mask, elevation=None, grid=None):
    """generate_base_properties with elevation and latitude (topography.py:295-346): albedo 0.28 / 0.08 brightened towards the
    poles and with height over land, friction 1e-5 / 1e-6 raised by mountain drag.  Pointwise, on the host."""
    mask = np.asarray(mask).astype(np.uint8)
    land = mask == 1
    elevation = np.zeros(mask.shape, dtype=float) if elevation is None else np.asarray(elevation, dtype=float)
    lat_factor = (np.abs(grid.lat_mesh) / 90.0) ** 2 if grid is not None else np.zeros(mask.shape, dtype=float)
    height = np.clip(np.maximum(elevation, 0.0) / 4000.0, 0.0, 1.0)
    albedo = np.where(land, 0.28, 0.08)
    albedo += 0.08 * lat_factor
    albedo += 0.05 * height * land
    albedo = np.clip(albedo, 0.05, 0.85)
    friction = np.where(land, 1.0e-5, 1.0e-6)
    friction += 6.0e-6 * height * land
    return albedo, np.clip(friction, 5e-7, 3e-5)


def write_topography(path, grid, elevation, land_mask, base_albedo, friction, sea_level_m):
    """export_topography_to_netcdf (topography.py:353-423): f4 axes, elevation / base_albedo / friction f4, land_mask i1, the
    reference's global attributes (target_land_fraction is always 0.29 there) and the planet constants."""
    from .ncio import write_nc
    f4 = lambda a: np.asarray(a).astype(np.float32)
    v = {"lat": ("f4", ("lat",), f4(grid.lat)), "lon": ("f4", ("lon",), f4(grid.lon)),
         "elevation": ("f4", ("lat", "lon"), f4(elevation)),
         "land_mask": ("i1", ("lat", "lon"), np.asarray(land_mask).astype(np.int8)),
         "base_albedo": ("f4", ("lat", "lon"), f4(base_albedo)),
         "friction": ("f4", ("lat", "lon"), f4(friction))}
    attrs = {"title": "Qingdai Topography and Surface Properties", "institution": "PyGCM for Qingdai",
             "source": "Procedural generation (Project 004 Milestone 1)",
             "history": "Created by pygcm.topography.export_topography_to_netcdf",
             "references": "docs/projects/004-topography-generation.md"}
    # np.float64: doubles on disk with either backend, as the reference's netCDF4 writes Python floats
    attrs.update({k: np.float64(x) for k, x in (("sea_level_m", sea_level_m), ("target_land_fraction", 0.29),
                                                ("planet_radius_m", PLANET_RADIUS), ("planet_omega_rad_s", PLANET_OMEGA),
                                                ("planet_axial_tilt_deg", PLANET_AXIAL_TILT))})
    write_nc(path, {"lat": int(grid.n_lat), "lon": int(grid.n_lon)}, v, attrs)
