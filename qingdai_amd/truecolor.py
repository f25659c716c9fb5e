"""
qingdai_amd/truecolor.py -- the reference's true-colour frame (`plot_true_color`, scripts/run_simulation.py:539-778) from the
resident state.

The reference builds rgb_map[n_lat, n_lon, 3] with pointwise array arithmetic, hands it to imshow and prints a [TrueColor] line
with two sea-ice numbers.  Here the array is composed in one launch (csrc/qd_truecolor.hip) from the resident fields, the canopy
factor, the phytoplankton band stack and the routing flow map; three bytes per cell cross the host link and the PNG is written
with the standard library (imgio.py): n_lat x n_lon pixels, no axes, no title.

Host side: the reference's environment, read as plot_true_color reads it (with its fallbacks where it has them), the Gaussian
channel weights, the two-star band tables of spectral.py, and the effective leaf reflectance, which follows the species weights
and is therefore looked up again at every render.
"""
from __future__ import annotations

import os

import numpy as np

from . import _lib
from . import spectral as sp

MAX_BANDS = _lib.TRUECOLOR_MAX_BANDS


def _f(env, key, default):
    return float(env.get(key, default))


def _f_fallback(env, key, default):
    try:
        return float(env.get(key, default))
    except Exception:      # noqa: BLE001  (the reference's own try / except around these four)
        return float(default)


def band_centers(bands, nb):
    """lambda_centers of a band set, or the reference's coarse fallback when they do not fit (run_simulation.py:595-597)."""
    lam = getattr(bands, "lambda_centers", None)
    if lam is None or len(lam) != nb:
        lam = np.linspace(420.0, 680.0, nb)
    return np.asarray(lam, dtype=float)


def _norm_gauss(x, mu, sigma):
    w = np.exp(-((x - mu) ** 2) / (2.0 * sigma ** 2))
    return w / (float(np.sum(w)) + 1e-12)


def channel_weights(lam):
    """-> (wr, wg, wb): normalised Gaussians around 610 / 550 / 460 nm (run_simulation.py:599-607)."""
    lam = np.asarray(lam, dtype=float)
    return _norm_gauss(lam, 610.0, 50.0), _norm_gauss(lam, 550.0, 40.0), _norm_gauss(lam, 460.0, 40.0)


def read_env(env=None):
    """The switches and numbers plot_true_color reads, under its names -> dict.  The four values the reference guards with a
    try / except fall back to its defaults; a failure inside its snow block or its river block switches that block off, as its
    `except: pass` does; the remaining ones raise like the reference."""
    env = os.environ if env is None else env
    e = {"h_ice_ref": _f(env, "QD_HICE_REF", "0.5"), "ice_frac_thr": _f(env, "QD_TRUECOLOR_ICE_FRAC", "0.15")}
    try:
        e["snow_by_swe"] = int(env.get("QD_TRUECOLOR_SNOW_BY_SWE", "1")) == 1
        e["snow_cover_frac"], e["snow_vis_alpha"] = _f(env, "QD_SNOW_COVER_FRAC", "0.20"), _f(env, "QD_SNOW_VIS_ALPHA", "0.60")
    except Exception:      # noqa: BLE001
        e["snow_by_swe"], e["snow_cover_frac"], e["snow_vis_alpha"] = False, 0.20, 0.60
    try:
        e["veg"] = int(env.get("QD_ECO_TRUECOLOR_VEG", "1")) == 1
    except Exception:      # noqa: BLE001
        e["veg"] = False
    e["veg_gamma"] = _f_fallback(env, "QD_ECO_TRUECOLOR_GAMMA", "1.8")
    e["veg_sat"] = _f_fallback(env, "QD_ECO_TRUECOLOR_SAT", "1.35")
    try:
        e["oceancolor"] = int(env.get("QD_PLOT_OCEANCOLOR", "1")) == 1
    except Exception:      # noqa: BLE001
        e["oceancolor"] = False
    try:
        e["oc_gamma"] = float(env.get("QD_OC_GAMMA", env.get("QD_ECO_TRUECOLOR_GAMMA", "2.2")))
    except Exception:      # noqa: BLE001
        e["oc_gamma"] = 2.2
    e["oc_blend"] = _f_fallback(env, "QD_OC_BLEND", "0.85")
    e["snow_by_ts"] = int(env.get("QD_TRUECOLOR_SNOW_BY_TS", "0")) == 1
    e["snow_thresh"] = _f(env, "QD_SNOW_THRESH", "273.15")
    e["cloud_alpha"], e["cloud_white"] = _f(env, "QD_TRUECOLOR_CLOUD_ALPHA", "0.60"), _f(env, "QD_TRUECOLOR_CLOUD_WHITE", "0.95")
    e["overlay_ok"] = True
    try:
        e["rivers"] = int(env.get("QD_PLOT_RIVERS", "1")) == 1
        e["river_min"], e["river_alpha"] = _f(env, "QD_RIVER_MIN_KGPS", "1e6"), _f(env, "QD_RIVER_ALPHA", "0.45")
        e["lake_alpha"] = _f(env, "QD_LAKE_ALPHA", "0.40")
    except Exception:      # noqa: BLE001
        e.update(rivers=False, river_min=1e6, river_alpha=0.45, lake_alpha=0.40, overlay_ok=False)
    return e


def band_table(bands, nb, R_eff=None):
    """[6 or 7][nb]: (R_eff,) wr, wg, wb, specA, specB, T_ray of one band set."""
    wr, wg, wb = channel_weights(band_centers(bands, nb))
    specA, specB, tray = sp.star_band_weights(bands)
    rows = ([] if R_eff is None else [np.asarray(R_eff, dtype=float)]) + [wr, wg, wb, specA, specB, tray]
    return np.ascontiguousarray(np.stack([np.asarray(r, dtype=np.float64).reshape(nb) for r in rows]))


def build_config(env=None, eco=None, phyto=None, routing=None):
    """-> (qd_truecolor_params, eco_tab or None, phyto_tab or None, lake_mask or None) for the objects the reference hands to
    plot_true_color: `eco` an EcologyAdapter (or None), `phyto` a PhytoDaily (or None), `routing` a RiverRouting (or None)."""
    e = read_env(env)
    p = _lib.qd_truecolor_params()
    p.snow_by_swe, p.snow_by_ts = int(e["snow_by_swe"]), int(e["snow_by_ts"])
    for k in ("h_ice_ref", "ice_frac_thr", "snow_cover_frac", "snow_vis_alpha", "veg_gamma", "veg_sat", "oc_gamma", "oc_blend",
              "snow_thresh", "cloud_alpha", "cloud_white", "river_min", "river_alpha", "lake_alpha"):
        setattr(p, k, float(e[k]))
    p.soil_ref = 0.20
    eco_tab = phyto_tab = lake = None
    if e["veg"] and eco is not None:
        nb = int(eco.bands.nbands)
        if nb > MAX_BANDS:
            raise ValueError(f"true colour: the vegetation overlay supports at most {MAX_BANDS} ecology bands, got {nb} "
                             "(set QD_ECO_TRUECOLOR_VEG=0 to render without it)")
        pop = getattr(eco, "pop", None)
        R_eff = pop.effective_leaf_reflectance_bands(nb) if pop is not None else eco.R_leaf      # adapter.py:530-543 without one
        p.veg, p.veg_f_one, p.nb_eco, p.soil_ref = 1, 0 if pop is not None else 1, nb, float(eco.params.soil_ref)
        eco_tab = band_table(eco.bands, nb, R_eff)
    if e["oceancolor"] and phyto is not None:
        nb = int(phyto.bands.nbands)
        if nb > MAX_BANDS:
            raise ValueError(f"true colour: the ocean-colour overlay supports at most {MAX_BANDS} phytoplankton bands, got {nb} "
                             "(set QD_PLOT_OCEANCOLOR=0 to render without it)")
        p.oceancolor, p.nb_phyto = 1, nb
        phyto_tab = band_table(phyto.bands, nb)
    if routing is not None and e["overlay_ok"]:
        p.rivers = int(e["rivers"])
        lm = getattr(getattr(routing, "net", None), "lake_mask", None)
        if lm is None:
            lm = getattr(routing, "lake_mask", None)
        if lm is not None and np.any(lm):
            lake = np.ascontiguousarray(np.asarray(lm).astype(float).astype(np.uint8))
            p.lakes = 1
    return p, eco_tab, phyto_tab, lake


def plot_interval_steps(env, dt):
    """run_simulation.py:1649-1651."""
    return max(1, int(float(env.get("QD_PLOT_EVERY_DAYS", "10")) * 24 * 3600 / dt))


def firing_steps(i0, n, interval):
    """The steps k of [0, n) whose run-local index i0 + k fires the plots (i % plot_interval_steps == 0, run_simulation.py:2426)."""
    return [k for k in range(int(n)) if (int(i0) + k) % int(interval) == 0]


def frame_name(t_days):
    return f"true_color_day_{t_days:05.1f}.png"


def truecolor_line(sea_ice_area, mean_h_ice, ice_frac_thr, cloud_alpha):
    """run_simulation.py:776."""
    return f"[TrueColor] sea_ice_area≈{sea_ice_area:.3f}, mean_h_ice={mean_h_ice:.3f} m (thr={ice_frac_thr}, alpha={cloud_alpha})"


def _key(p, *arrays):
    return bytes(p) + b"".join(b"|" if a is None else np.ascontiguousarray(a).tobytes() + b"|" for a in arrays)


class TrueColor:
    """The renderer of one device handle.  `src`: a driver.Simulation (its device, ecology adapter, daily phytoplankton manager
    and routing are used) or a Device, with `eco`, `phyto` (a PhytoDaily), `routing` given by keyword.  `phyto_bands`: a host
    [NB, lat, lon] stack in place of the resident one (tests)."""

    def __init__(self, src, eco=None, phyto=None, routing=None, env=None, phyto_bands=None):
        if hasattr(src, "dev") and hasattr(src, "gcm"):
            self.dev = src.dev
            self._sim = src
        else:
            self.dev, self._sim = src, None
        self._eco, self._phyto, self._routing = eco, phyto, routing
        self.env = env
        self.phyto_bands = phyto_bands
        self._configured = None
        self.params = None

    def _parts(self):
        s = self._sim
        if s is None:
            return self._eco, self._phyto, self._routing
        return (self._eco if self._eco is not None else s.eco, self._phyto if self._phyto is not None else s.phyto_daily,
                self._routing if self._routing is not None else getattr(s, "routing", None))

    def configure(self):
        """Reads the environment and the tables again; uploads them when anything differs from what the device holds."""
        p, eco_tab, phyto_tab, lake = build_config(self.env, *self._parts())
        key = _key(p, eco_tab, phyto_tab, lake, self.phyto_bands)
        if key != self._configured:
            self.dev.truecolor_configure(p, eco_tab, phyto_tab, self.phyto_bands, lake)
            self._configured = key
        self.params = p
        return p

    def render(self, want_f64=False, flow=None):
        """-> (u8 image [n_lat, n_lon, 3] with the northernmost row first, sea_ice_area, mean_h_ice).  want_f64 also keeps the
        unquantised rgb_map of the reference on the device (rgb()).  Reads the state and changes none of it."""
        self.configure()
        area, mean_h = self.dev.truecolor_render(want_f64=want_f64, flow=flow)
        return self.dev.truecolor_image(), area, mean_h

    def rgb(self):
        return self.dev.truecolor_rgb()

    def line(self, area, mean_h):
        return truecolor_line(area, mean_h, float(self.params.ice_frac_thr), float(self.params.cloud_alpha))

    def write_frame(self, t_days, output_dir=None):
        """One firing: render, write <output_dir>/true_color_day_*.png -> (path, the [TrueColor] line)."""
        from .imgio import write_png
        img, area, mean_h = self.render()
        out = output_dir if output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, frame_name(t_days))
        write_png(path, img)
        return path, self.line(area, mean_h)
