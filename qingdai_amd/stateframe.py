"""
qingdai_amd/stateframe.py -- the reference's 15-panel status figure (`plot_state`, scripts/run_simulation.py:330-537) from the
resident state.

The reference hands fifteen derived maps to matplotlib's contourf and saves state_day_*.png.  Here a frame is a mosaic of 5 x 3
tiles of n_lat x n_lon pixels (one pixel per cell, northernmost row on top, a white gutter of 4 pixels, no titles, axes or
colourbars): csrc/qd_stateframe.hip computes the fields, reduces the extremes the level rules need (qd_stateframe_scan), and draws
every tile as the contourf sampled at the cell centres with the coast, river, lake and star-position overlays
(qd_stateframe_render).  This module is the host side between the two launches: contourf's level rules restated without
matplotlib (auto_levels), its band colours (band_colours; the colormap tables are package data, data/stateframe_cmaps.json,
written by scripts/gen_stateframe_cmaps.py -- text with repr floats, because the repository keeps binary files under tests/golden/
only and this one is read by the product at run time; twelve tables, one per colormap name plot_state uses, and Greens for
qingdai_amd/figures.py), the table the render reads (build_table / pack_table), and the JSON sidecar that
carries what the colourbars would say.

Two departures from the reference: the panels 7 and 8 fill the speed field the reference colours its streamlines with (the
streamlines are not drawn), and a panel without a usable range is left white apart from its overlays and marked "constant".
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from . import _lib

N_PANELS = _lib.STATEFRAME_PANELS
MAX_LEVELS = _lib.STATEFRAME_MAX_LEVELS
GUTTER = _lib.STATEFRAME_GUTTER
AUTO_PANELS = (3, 7, 8, 9, 10, 12, 13, 14, 15)                # 1-based: the order of the scan's min / max slots
CMAPS_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "data", "stateframe_cmaps.json")
RIVER_RGB, LAKE_RGB = (0.0, 0.749, 1.0), (0.118, 0.565, 1.0)  # deepskyblue, dodgerblue
STAR_A_RGB, STAR_B_RGB = (0.0, 1.0, 1.0), (1.0, 1.0, 0.0)     # cyan x, yellow +

# (title, unit, cmap, level rule, coast) per panel, in the reference's order (run_simulation.py:353-502)
_PANELS = (
    ("Surface Temperature (°C)", "°C", "coolwarm", "t", 1),
    ("Atmospheric Temperature (°C)", "°C", "coolwarm", "t", 1),
    ("Sea-level Pressure Anomaly (hPa, diag)", "hPa", "viridis", "auto", 1),
    ("SST (°C)", "°C", "coolwarm", "t", 1),
    ("Precipitation (instant, mm/day)", "mm/day", "Blues", "precip", 1),
    ("Cloud Cover Fraction", "Fraction", "Greys", "cloud", 1),
    ("Wind Field (m/s)", "m/s", "viridis", "auto", 1),
    ("Ocean Currents (m/s)", "m/s", "viridis", "auto", 1),
    ("Relative Vorticity (1/s)", "1/s", "PuOr", "vort", 1),
    ("Incoming Shortwave (W/m²)", "W/m²", "magma", "auto", 0),
    ("Dynamic Albedo", "Albedo", "cividis", "albedo", 1),
    ("Outgoing Longwave (W/m²)", "W/m²", "plasma", "auto", 2),
    ("Specific Humidity q (g/kg)", "g/kg", "GnBu", "auto", 1),
    ("Evaporation (mm/day)", "mm/day", "YlGn", "auto", 1),
    ("Condensation P_cond (mm/day)", "mm/day", "BuPu", "auto", 1),
)


def panels(ps_abs=False, ocean=True):
    """-> the fifteen (title, unit, cmap, rule, coast) with the two titles and the one colormap that depend on the run."""
    out = [list(p) for p in _PANELS]
    if ps_abs:
        out[2][0] = "Sea-level Pressure (hPa, diag)"
    if not ocean:
        out[7][:3] = ["Geopotential Height Anomaly (m)", "m", "RdBu_r"]
    return [tuple(p) for p in out]


def read_env(env=None):
    """What plot_state reads from the environment, under its defaults (QD_RIVER_ALPHA is 0.35 here, 0.45 in the true-colour frame).
    A failure inside its overlay block switches the overlays off, as its `except: pass` does."""
    env = os.environ if env is None else env
    e = {"ps_abs": str(env.get("QD_PLOT_PS_MODE", "anom")).lower() == "abs", "overlay_ok": True}
    try:
        e["rivers"] = int(env.get("QD_PLOT_RIVERS", "1")) == 1
        e["river_min"], e["river_alpha"] = float(env.get("QD_RIVER_MIN_KGPS", "1e6")), float(env.get("QD_RIVER_ALPHA", "0.35"))
        e["lake_alpha"] = float(env.get("QD_LAKE_ALPHA", "0.40"))
    except Exception:      # noqa: BLE001
        e.update(rivers=False, river_min=1e6, river_alpha=0.35, lake_alpha=0.40, overlay_ok=False)
    return e


# ------------------------------------------------------------------------------------- contourf's level rules
_STEPS = np.array([1, 1.5, 2, 2.5, 3, 4, 5, 6, 8, 10])
_EXT_STEPS = np.concatenate([0.1 * _STEPS[:-1], _STEPS, [10 * _STEPS[1]]])


def _nonsingular(vmin, vmax, expander=1e-13, tiny=1e-14):
    if not (math.isfinite(vmin) and math.isfinite(vmax)):
        return -expander, expander
    if vmax < vmin:
        vmin, vmax = vmax, vmin
    vmin, vmax = float(vmin), float(vmax)
    big = max(abs(vmin), abs(vmax))
    if big < (1e6 / tiny) * np.finfo(float).tiny:
        return -expander, expander
    if vmax - vmin <= big * tiny:
        if vmax == 0 and vmin == 0:
            return -expander, expander
        return vmin - expander * abs(vmin), vmax + expander * abs(vmax)
    return vmin, vmax


def _closeto(ms, edge, step, offset):
    if offset > 0:
        tol = min(0.4999, max(1e-10, 10 ** (np.log10(offset / step) - 12)))
    else:
        tol = 1e-10
    return abs(ms - edge) < tol


def auto_levels(zmin, zmax, n=20):
    """matplotlib's contourf(levels=n): MaxNLocator(n + 1, min_n_ticks=1).tick_values(zmin, zmax) trimmed by ContourSet._autolev
    (no extend), restated: scale_range, the default step table extended by one decade entry on either side, _Edge_integer's le / ge
    with their closeto tolerance, the trim."""
    nbins = n + 1
    vmin, vmax = _nonsingular(zmin, zmax)
    dv, meanv = abs(vmax - vmin), (vmax + vmin) / 2
    offset = 0 if abs(meanv) / dv < 100 else math.copysign(10 ** (math.log10(abs(meanv)) // 1), meanv)
    scale = 10 ** (math.log10(dv / nbins) // 1)
    lo, hi = vmin - offset, vmax - offset
    steps = _EXT_STEPS * scale
    large = steps >= (hi - lo) / nbins
    istep = int(np.nonzero(large)[0][0]) if large.any() else len(steps) - 1
    for step in steps[:istep + 1][::-1]:
        best = (lo // step) * step
        d, m = divmod(lo - best, step)
        low = d + 1 if _closeto(m / step, 1, step, abs(offset)) else d
        d, m = divmod(hi - best, step)
        high = d if _closeto(m / step, 0, step, abs(offset)) else d + 1
        ticks = np.arange(low, high + 1) * step + best
        if ((ticks <= hi) & (ticks >= lo)).sum() >= 1:
            break
    lev = ticks + offset
    under, over = np.nonzero(lev < zmin)[0], np.nonzero(lev > zmax)[0]
    i0 = under[-1] if len(under) else 0
    i1 = over[0] + 1 if len(over) else len(lev)
    if i1 - i0 < 3:
        i0, i1 = 0, len(lev)
    return np.asarray(lev[i0:i1], dtype=np.float64)


_cmaps = None


def cmap_table(name):
    """The 256 x 3 f64 lookup table of one of the reference's colormaps (package data)."""
    global _cmaps
    if _cmaps is None:
        with open(CMAPS_JSON, encoding="ascii") as f:
            _cmaps = {k: np.array(v, dtype=np.float64) for k, v in json.load(f).items()}
    return _cmaps[name]


def band_colours(cmap_name, levels, extend=False):
    """-> [len(levels) - 1 (+ 1 with extend), 3]: cmap(norm(mid)) per band, mid the midpoint of the band, norm linear between the first
    and the last level, LUT index int(x * 256) with x == 1 -> 255; the extended band takes the LUT's last entry."""
    lut = cmap_table(cmap_name)
    lev = np.asarray(levels, dtype=np.float64)
    mid = 0.5 * (lev[:-1] + lev[1:])
    with np.errstate(all="ignore"):
        x = (mid - lev[0]) / (lev[-1] - lev[0])
        xa = x * 256
    idx = np.where(xa == 256, 255, np.clip(np.nan_to_num(xa, nan=0.0), 0, 255)).astype(int)
    rgb = lut[idx]
    return np.concatenate([rgb, lut[-1:]]) if extend else rgb


def is_constant(zmin, zmax):
    """No finite value, or a range no wider than 1e-12 of its magnitude: the panel is left white."""
    if not (math.isfinite(zmin) and math.isfinite(zmax)) or zmax < zmin:
        return True
    return zmax - zmin <= 1e-12 * max(abs(zmin), abs(zmax))


def unpack_scan(out, marks):
    """The raw result of qd_stateframe_scan -> {"t_min" [3], "t_max" [3] (NaN for a T_a that holds a NaN, as np.min gives),
    "auto" {panel: (zmin, zmax)}, "vmax", "marks" [cell A, cell B], "mark_values"}."""
    out = np.asarray(out, dtype=np.float64)
    t_min, t_max = out[0:3].copy(), out[3:6].copy()
    if out[25] > 0.0:
        t_min[1] = t_max[1] = np.nan
    return {"t_min": t_min, "t_max": t_max, "auto": {p: (float(out[6 + k]), float(out[15 + k])) for k, p in enumerate(AUTO_PANELS)},
            "vmax": float(out[24]) if out[24] != -np.inf else float("nan"), "marks": [int(marks[0]), int(marks[1])],
            "mark_values": [float(out[26]), float(out[27])]}


def build_table(scan, env=None, ocean=True):
    """scan: unpack_scan's dict; env: read_env's dict (or an environment mapping, or None) -> the fifteen panels as a list of
    {"title", "unit", "cmap", "levels" (array or None), "colours" ([bands, 3] or None), "extend", "constant", "coast"} plus the two
    mark cells: ({"panels": [...], "marks": [a, b]}).  The level rules of run_simulation.py:349-351, 381, 396, 403, 432-435, 458."""
    e = env if isinstance(env, dict) and "ps_abs" in env else read_env(env)
    with np.errstate(all="ignore"):
        tmin, tmax = float(np.nanmin(scan["t_min"])), float(np.nanmax(scan["t_max"]))
    out = []
    for k, (title, unit, cmap, rule, coast) in enumerate(panels(e["ps_abs"], ocean)):
        extend, constant, lev = False, False, None
        if rule == "t":
            constant = is_constant(tmin, tmax)
            lev = None if constant else np.linspace(tmin, tmax, 20)
        elif rule == "precip":
            lev, extend = np.linspace(0, 30, 11), True
        elif rule == "cloud":
            lev = np.linspace(0, 1, 11)
        elif rule == "albedo":
            lev = np.linspace(0, 0.8, 17)
        else:
            vmax = scan["vmax"]
            if rule == "vort" and np.isfinite(vmax) and vmax > 0:
                lev = np.linspace(-vmax, vmax, 21)
            else:
                zmin, zmax = scan["auto"][k + 1]
                constant = is_constant(zmin, zmax)
                lev = None if constant else auto_levels(zmin, zmax, 20)
        if lev is not None and not (np.all(np.isfinite(lev)) and np.all(np.diff(lev) > 0)):
            constant, lev = True, None                          # contourf raises "Contour levels must be increasing" there
        out.append({"title": title, "unit": unit, "cmap": cmap, "levels": lev, "extend": extend, "constant": constant, "coast": coast,
                    "colours": None if lev is None else band_colours(cmap, lev, extend)})
    return {"panels": out, "marks": list(scan["marks"])}


def pack_table(tab):
    """build_table's result -> the _lib.qd_stateframe_table the render reads.  More than 32 levels are refused."""
    t = _lib.qd_stateframe_table()
    for k, p in enumerate(tab["panels"]):
        q = t.panel[k]
        q.extend_max, q.constant, q.coast = int(p["extend"]), int(p["constant"]), int(p["coast"])
        if p["levels"] is None:
            q.n_levels = 0
            continue
        n = len(p["levels"])
        if n > MAX_LEVELS:
            raise ValueError(f"state frame: panel {k + 1} has {n} levels, at most {MAX_LEVELS} are supported")
        q.n_levels = n
        for i, v in enumerate(p["levels"]):
            q.levels[i] = float(v)
        for i, c in enumerate(p["colours"]):
            for j in range(3):
                q.rgb[i][j] = float(c[j])
    t.mark_cell[0], t.mark_cell[1] = int(tab["marks"][0]), int(tab["marks"][1])
    return t


def mosaic_shape(n_lat, n_lon):
    return 5 * n_lat + 6 * GUTTER, 3 * n_lon + 4 * GUTTER


def tile_origin(k, n_lat, n_lon):
    """-> (top row, left column) of the tile of panel k (0-based) in the mosaic."""
    return GUTTER + (k // 3) * (n_lat + GUTTER), GUTTER + (k % 3) * (n_lon + GUTTER)


def frame_name(t_days):
    return f"state_day_{t_days:05.1f}.png"


def sidecar(tab, t_days, lat, lon):
    """What the colourbars and the legend would say -> a JSON-serialisable dict."""
    n_lon = len(lon)
    stars = {}
    for name, cell in zip(("A", "B"), tab["marks"]):
        stars[name] = None if cell < 0 else {"lat": float(lat[cell // n_lon]), "lon": float(lon[cell % n_lon])}
    return {"t_days": float(t_days), "layout": {"rows": 5, "cols": 3, "gutter": GUTTER, "tile": [len(lat), n_lon]},
            "panels": [{"panel": k + 1, "title": p["title"], "unit": p["unit"], "cmap": p["cmap"], "extend": "max" if p["extend"] else "neither",
                        "constant": bool(p["constant"]), "levels": None if p["levels"] is None else [float(v) for v in p["levels"]]}
                       for k, p in enumerate(tab["panels"])],
            "stars": stars}


class StateFrame:
    """The renderer of one device handle.  `src`: a driver.Simulation (its device, ocean and routing are used) or a Device, with
    `ocean` (is panel 4 the SST and panel 8 the currents?) and `routing` given by keyword."""

    def __init__(self, src, routing=None, env=None, ocean=None):
        if hasattr(src, "dev") and hasattr(src, "gcm"):
            self.dev, self._sim = src.dev, src
        else:
            self.dev, self._sim = src, None
        self._routing, self._ocean = routing, ocean
        self.env = env
        self._configured = None
        self.params = None
        self.table = None

    def _parts(self):
        s = self._sim
        routing = self._routing if self._routing is not None else (getattr(s, "routing", None) if s is not None else None)
        ocean = self._ocean if self._ocean is not None else (s.ocean is not None if s is not None else True)
        return routing, bool(ocean)

    def configure(self):
        """Reads the environment again; uploads when anything differs from what the device holds -> qd_stateframe_params."""
        routing, ocean = self._parts()
        e = read_env(self.env)
        p = _lib.qd_stateframe_params()
        dp = self.dev.params
        p.ps_abs, p.ocean = int(e["ps_abs"]), int(ocean)
        p.p0, p.rho_a, p.H = float(dp.p0), float(dp.rho_a), float(dp.H)
        p.river_min, p.river_alpha, p.lake_alpha = e["river_min"], e["river_alpha"], e["lake_alpha"]
        lake = None
        if routing is not None and e["overlay_ok"] and e["rivers"]:
            p.rivers = 1
            lm = getattr(getattr(routing, "net", None), "lake_mask", None)
            if lm is None:
                lm = getattr(routing, "lake_mask", None)
            if lm is not None and np.any(lm):
                lake = np.ascontiguousarray(np.asarray(lm).astype(float).astype(np.uint8))
                p.lakes = 1
        key = bytes(p) + (b"" if lake is None else lake.tobytes())
        if key != self._configured:
            self.dev.stateframe_configure(p, lake)
            self._configured = key
        self.params, self._env = p, e
        return p

    def render(self, want_stacks=False, flow=None):
        """scan -> table -> render -> the u8 mosaic [5 n_lat + 24, 3 n_lon + 16, 3].  want_stacks keeps the band indices and the
        fields on the device (bands() / fields()).  Reads the state and changes none of it."""
        self.configure()
        out, marks = self.dev.stateframe_scan()
        self.scan = unpack_scan(out, marks)
        self.table = build_table(self.scan, self._env, ocean=bool(self.params.ocean))
        self.dev.stateframe_render(pack_table(self.table), flow=flow, want_stacks=want_stacks)
        return self.dev.stateframe_image()

    def bands(self):
        return self.dev.stateframe_bands()

    def fields(self):
        return self.dev.stateframe_fields()

    def write_frame(self, t_days, output_dir=None):
        """One firing: render, write <output_dir>/state_day_*.png and the .json sidecar next to it -> the PNG's path."""
        from .imgio import write_png
        img = self.render()
        out = output_dir if output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")
        os.makedirs(out, exist_ok=True)
        path = os.path.join(out, frame_name(t_days))
        write_png(path, img)
        g = self.dev.grid
        with open(path[:-4] + ".json", "w", encoding="utf-8") as f:
            json.dump(sidecar(self.table, t_days, g.lat, g.lon), f, ensure_ascii=False, indent=1)
        return path
