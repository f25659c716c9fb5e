"""
qingdai_amd/figures.py -- the reference's ecology panel (`plot_ecology`, scripts/run_simulation.py:954-1060), plankton species maps
(`plot_plankton_species`, :828-889) and per-star ISR figure (`plot_isr_components`, :891-951) from the resident state.

A figure is one row of tiles with the state frame's geometry (one pixel per cell, northernmost row on top, a white gutter of 4
pixels, no titles, axes or colourbars): csrc/qd_tiles.hip evaluates the planes the reference hands to contourf, reduces what the
level rules need (qd_tiles_scan, qd_tiles_order_stats) and draws the tiles (qd_tiles_render).  This module is the host side between
the launches: the level rules (stateframe.auto_levels for `levels=20`, fixed tables, np.nanpercentile's linear rule on two order
statistics of the device), the band colours (stateframe.band_colours), the tile table, the [Diagnostics] line of the ISR figure and
the JSON sidecars that carry what titles and colourbars would say.  No matplotlib at run time.

As in the state frame, a tile without a usable range (contourf would raise, or `levels=20` meets a constant field) is left white
under its coast and marked "constant"; the reference's "... not available" placeholders are marked "unavailable".  The reference's
Whittaker annotation (:1025-1056) looks up a name that is not in scope inside plot_ecology and is never drawn: no sidecar carries it.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np

from . import _lib
from .stateframe import auto_levels, band_colours, is_constant, GUTTER, MAX_LEVELS

MAX_TILES = _lib.TILES_MAX
MARK_X, MARK_PLUS = 1, 2                                       # cyan x, yellow +


def read_env(env=None):
    """The switches of run_simulation.py:2431, 2469, 1646 (the reference's defaults), QD_PHYTO_VMAX (:858-860; None when unset or
    blank, the raw text otherwise) and QD_ECO_HEIGHT_SCALE_M (population.py:301-304)."""
    env = os.environ if env is None else env
    v = env.get("QD_PHYTO_VMAX")
    try:
        hs = float(env.get("QD_ECO_HEIGHT_SCALE_M", "10.0"))
    except Exception:      # noqa: BLE001
        hs = 10.0
    return {"plot_phyto": int(env.get("QD_PLOT_PHYTO", "1")) == 1, "plot_eco": int(env.get("QD_ECO_PLOT", "1")) == 1,
            "plot_isr": int(env.get("QD_PLOT_ISR", "0")) == 1, "vmax_env": v if (v is not None and v.strip() != "") else None,
            "height_scale": hs, "eco_diag": int(env.get("QD_ECO_DIAG", "1")) == 1, "phyto_diag": int(env.get("QD_PHYTO_DIAG", "1")) == 1}


def figures_enabled(env=None):
    """QD_FIGURES (default 0): this implementation's own switch, like QD_STATE_PLOT and QD_TRUECOLOR."""
    env = os.environ if env is None else env
    return int(env.get("QD_FIGURES", "0")) == 1


# ------------------------------------------------------------------------------------- np.nanpercentile's linear rule
def percentile_plan(n, q=99.0):
    """np.percentile(method="linear") on n sorted values -> (rank below, rank above, weight): the virtual index (n - 1) (q / 100),
    its floor and floor + 1, both the last rank when the index reaches it."""
    n = int(n)
    virtual = (n - 1) * np.true_divide(np.float64(q), np.float64(100))
    lo = int(np.floor(virtual))
    hi = lo + 1
    if virtual >= n - 1:
        lo = hi = -1
    elif virtual < 0:
        lo = hi = 0
    gamma = np.float64(virtual) - np.float64(lo)               # NumPy subtracts the index it ends up with (-1 included)
    return lo % n, hi % n, gamma


def percentile_lerp(a, b, t):
    """NumPy's _lerp: a + (b - a) t, replaced by b - (b - a) (1 - t) where t >= 0.5."""
    a, b, t = np.float64(a), np.float64(b), np.float64(t)
    with np.errstate(all="ignore"):
        d = b - a
        return float(b - d * (1 - t)) if t >= 0.5 else float(a + d * t)


def nanpercentile(order_stats, q=99.0):
    """order_stats(ranks) -> (count of non-NaN values, their ranks-th smallest): np.nanpercentile(x, q) as a number (NaN when
    the count is 0)."""
    n, _ = order_stats([])
    if n <= 0:
        return float("nan")
    lo, hi, t = percentile_plan(n, q)
    _, v = order_stats([lo, hi])
    return percentile_lerp(v[0], v[1], t)


def plankton_vmax(vmax_env, order_stats):
    """run_simulation.py:857-866: QD_PHYTO_VMAX when set and not blank, else the 99th percentile of the ocean cells; the largest value
    when either raises; 1e-3 when the result is not finite or not positive."""
    try:
        vmax = float(vmax_env) if vmax_env is not None else nanpercentile(order_stats, 99.0)
    except Exception:      # noqa: BLE001
        n, _ = order_stats([])
        vmax = float(order_stats([n - 1])[1][0]) if n > 0 else float("nan")      # np.nanmax
    if not np.isfinite(vmax) or vmax <= 0.0:
        vmax = 1.0e-3
    return vmax


# ------------------------------------------------------------------------------------- tiles
def _tile(title, unit, cmap, source, index=0, coast=1):
    return {"title": title, "unit": unit, "cmap": cmap, "source": source, "index": int(index), "coast": coast, "levels": None,
            "colours": None, "extend": False, "constant": False, "unavailable": False, "mark": None}


def _set_levels(t, lev):
    """Levels contourf would refuse (not finite, not increasing) leave the tile "constant"."""
    lev = None if lev is None else np.asarray(lev, dtype=np.float64)
    if lev is None or len(lev) < 2 or not (np.all(np.isfinite(lev)) and np.all(np.diff(lev) > 0)):
        t["constant"], t["levels"], t["colours"] = True, None, None
    else:
        t["levels"], t["colours"] = lev, band_colours(t["cmap"], lev, t["extend"])
    return t


def _auto(t, zmin, zmax, n=20):
    """contourf(levels=n) on a plane with the finite range [zmin, zmax]."""
    return _set_levels(t, None if is_constant(zmin, zmax) else auto_levels(zmin, zmax, n))


def ecology_tiles(t_days, population, alpha_ok, banded_ok, banded_source="ALPHA_BANDED"):
    """The tiles of plot_ecology in its order, without levels: five with a population, else three; "unavailable" where the reference
    draws its placeholder text."""
    out = [_tile(f"LAI (Day {t_days:.2f})", "LAI", "YlGn", "LAI"), _tile("Ecology alpha (scalar)", "alpha", "cividis", "ALPHA"),
           _tile("Ecology alpha (banded)", "alpha", "cividis", banded_source)]
    out[0]["unavailable"], out[1]["unavailable"], out[2]["unavailable"] = not population, not alpha_ok, not banded_ok
    if population:
        out += [_tile("Canopy height (m)", "m", "Greens", "CANOPY_HEIGHT"), _tile("Species 0 density (proxy)", "arb. units", "viridis", "SPECIES_DENSITY", 0)]
    return out


def ecology_levels(tiles, scan):
    """scan: {tile number: (zmin, zmax)} of the `levels=20` tiles (run_simulation.py:978, 989, 1000, 1009, 1019)."""
    for k, t in enumerate(tiles):
        if t["unavailable"]:
            continue
        if k in (1, 2):
            _set_levels(t, np.linspace(0, 0.8, 17))
        else:
            _auto(t, *scan[k])
    return tiles


def plankton_tile(t_days, species, vmax):
    """run_simulation.py:867-874."""
    t = _tile(f"Plankton species {species} (mg Chl m$^{{-3}}$) Day {t_days:.2f}", "mg Chl m$^{-3}$", "viridis", "PLANKTON", species)
    return _set_levels(t, np.linspace(0.0, vmax, 21))


def isr_tiles(t_days, max_a, max_b, cell_a, cell_b):
    """run_simulation.py:902-929.  max_a / max_b: np.max of the two planes (NaN when the plane holds one)."""
    vmax = max(max_a, max_b)                                   # Python's max, as the reference calls it
    lev = np.linspace(0.0, vmax, 21)
    out = [_tile(f"ISR - Star A (Day {t_days:.2f})", "W/m^2", "magma", "ISR_A", coast=0),
           _tile(f"ISR - Star B (Day {t_days:.2f})", "W/m^2", "magma", "ISR_B", coast=0)]
    for t, kind, cell in zip(out, (MARK_X, MARK_PLUS), (cell_a, cell_b)):
        _set_levels(t, lev)
        t["mark"] = (kind, int(cell))
    return out


def separation_line(t_days, lat, lon, cell_a, cell_b):
    """The [Diagnostics] line of run_simulation.py:923-947, character for character."""
    try:
        n_lon = len(lon)
        lonA, latA = lon[cell_a % n_lon], lat[cell_a // n_lon]
        lonB, latB = lon[cell_b % n_lon], lat[cell_b // n_lon]
        phi1 = math.radians(latA); lam1 = math.radians(lonA)       # noqa: E702
        phi2 = math.radians(latB); lam2 = math.radians(lonB)       # noqa: E702
        dlam = lam2 - lam1
        d_sigma = 2 * math.asin(math.sqrt(
            math.sin((phi2 - phi1)/2)**2 +
            math.cos(phi1)*math.cos(phi2)*math.sin(dlam/2)**2
        ))
        separation_deg = math.degrees(d_sigma)
        return (f"[Diagnostics] Day {t_days:.2f}: Subsolar separation ≈ {separation_deg:.2f}° "
                f"(A: lon={lonA:.1f}°, lat={latA:.1f}°; B: lon={lonB:.1f}°, lat={latB:.1f}°)")
    except Exception as e:      # noqa: BLE001
        return f"[Diagnostics] Could not compute subsolar separation: {e}"


def pack_tiles(tiles):
    """-> the list of _lib.qd_tile_desc the render reads.  More than 8 tiles or 32 levels are refused."""
    if len(tiles) > MAX_TILES:
        raise ValueError(f"figures: {len(tiles)} tiles, at most {MAX_TILES} are supported")
    out = []
    for k, p in enumerate(tiles):
        q = _lib.qd_tile_desc()
        q.source, q.index = _lib.TILE[p["source"]], int(p["index"])
        q.extend_max, q.constant, q.unavailable, q.coast = int(p["extend"]), int(p["constant"]), int(p["unavailable"]), int(p["coast"])
        q.mark_kind, q.mark_cell = (0, -1) if p["mark"] is None else (int(p["mark"][0]), int(p["mark"][1]))
        if p["levels"] is not None:
            n = len(p["levels"])
            if n > MAX_LEVELS:
                raise ValueError(f"figures: tile {k + 1} has {n} levels, at most {MAX_LEVELS} are supported")
            q.n_levels = n
            for i, v in enumerate(p["levels"]):
                q.levels[i] = float(v)
            for i, c in enumerate(p["colours"]):
                for j in range(3):
                    q.rgb[i][j] = float(c[j])
        out.append(q)
    return out


def mosaic_shape(n_tiles, n_lat, n_lon):
    return n_lat + 2 * GUTTER, n_tiles * n_lon + (n_tiles + 1) * GUTTER


def tile_origin(k, n_lat, n_lon):
    """-> (top row, left column) of tile k (0-based) in the mosaic."""
    return GUTTER, GUTTER + k * (n_lon + GUTTER)


def ecology_name(t_days):
    return f"ecology_day_{t_days:05.1f}.png"


def plankton_name(species, t_days):
    return os.path.join("plankton", f"species{species}_day_{t_days:05.1f}.png")


def isr_name(t_days):
    return f"isr_components_day_{t_days:05.1f}.png"


def sidecar(figure, tiles, t_days, lat, lon, **extra):
    """What titles, colourbars and legends would say -> a JSON-serialisable dict."""
    n_lon = len(lon)

    def mark(m):
        if m is None or m[1] < 0:
            return None
        return {"kind": "x" if m[0] == MARK_X else "+", "colour": "cyan" if m[0] == MARK_X else "yellow", "cell": int(m[1]),
                "lat": float(lat[m[1] // n_lon]), "lon": float(lon[m[1] % n_lon])}
    out = {"figure": figure, "t_days": float(t_days), "suptitle": None,
           "layout": {"rows": 1, "cols": len(tiles), "gutter": GUTTER, "tile": [len(lat), n_lon]},
           "tiles": [{"tile": k + 1, "title": p["title"], "unit": p["unit"], "cmap": p["cmap"], "extend": "max" if p["extend"] else "neither",
                      "constant": bool(p["constant"]), "unavailable": bool(p["unavailable"]), "coast": [None, "black", "white"][p["coast"]],
                      "levels": None if p["levels"] is None else [float(v) for v in p["levels"]], "mark": mark(p["mark"])}
                     for k, p in enumerate(tiles)]}
    out.update(extra)
    return out


class Figures:
    """The three figures of one device handle.  `src`: a driver.Simulation (its device, ecology and plankton are used) or a Device
    with the rest by keyword: `population` (is there one?), `layers` (a host [S, K, lat, lon] stack; None = the resident stack of
    eco_daily_configure), `alpha` / `banded` (None = ask the device whether the maps exist), `phyto_species` (S of the tracer stack)."""

    def __init__(self, src, env=None, population=None, layers=None, alpha=None, banded=None, phyto_species=None):
        if hasattr(src, "dev") and hasattr(src, "gcm"):
            self.dev, self._sim = src.dev, src
        else:
            self.dev, self._sim = src, None
        self.env = env
        self._population, self._layers, self._alpha, self._banded, self._phyto_S = population, layers, alpha, banded, phyto_species
        self.tiles = None
        self.line = None
        self.vmax = None

    # -- what the run has
    def _eco(self):
        return getattr(self._sim, "eco", None) if self._sim is not None else None

    def _stack(self):
        """-> (is there a population, the host stack to upload or None for the resident one)."""
        if self._sim is None:
            return bool(self._population), self._layers
        eco = self._eco()
        pop = getattr(eco, "pop", None) if eco is not None else None
        if pop is None:
            return False, None
        return True, (None if pop.daily is not None else np.asarray(pop.LAI_layers_SK, dtype=np.float64))

    def n_phyto(self):
        if self._sim is None:
            return int(self._phyto_S or 0)
        ph = getattr(self._sim, "phyto", None)
        return int(ph.S) if ph is not None else 0

    def configure(self):
        """Reads the environment again and hands the height scale and, without a resident stack, the host stack to the device.
        A latitude-band handle is refused here."""
        self._env = read_env(self.env)
        self._pop, layers = self._stack()
        self.dev.tiles_configure(self._env["height_scale"], layers)
        return self._env

    def _order_stats(self, source, index):
        return lambda ranks: self.dev.tiles_order_stats(source, index, ranks)

    def _render(self, tiles, want_stacks):
        self.tiles = tiles
        self.dev.tiles_render(pack_tiles(tiles), want_stacks=want_stacks)
        return self.dev.tiles_image()

    # -- the figures: scan -> levels -> render -> the u8 mosaic.  Each reads the state and changes none of it.
    def ecology(self, t_days, want_stacks=False):
        e = self.configure()
        have_lai, alpha_ok, banded_ok = self.dev.tiles_available()
        alpha_ok = alpha_ok if self._alpha is None else bool(self._alpha)
        banded_ok = banded_ok if self._banded is None else bool(self._banded)
        source = "ALPHA_BANDED"
        eco = self._eco()
        if not banded_ok and eco is not None and self._pop:
            # run_simulation.py:2458-2466: the panel's own fallback, into a local map -- the resident ECO_ALPHA_BANDED (and with it a
            # run under QD_ECO_BANDS_COUPLE) is left as it is
            try:
                A, w = eco.get_surface_albedo_bands()
            except Exception:      # noqa: BLE001
                A, w = None, None
            self.dev._host.pop("ECO_F", None)                  # a read: nothing to send back with the next flush
            if A is not None and w is not None:
                with np.errstate(all="ignore"):
                    self.dev.tiles_set_plane(np.clip(np.nansum(A * w[:, None, None], axis=0), 0.0, 1.0))
                banded_ok, source = True, "HOST_PLANE"
                if e["eco_diag"]:
                    print(f"[Ecology] Panel fallback: banded alpha computed from {A.shape[0]} bands.")
        tiles = ecology_tiles(t_days, self._pop, alpha_ok and eco_or_forced(self, eco), banded_ok, source)
        auto = [k for k, t in enumerate(tiles) if not t["unavailable"] and k not in (1, 2)]
        scan = {}
        if auto:
            res = self.dev.tiles_scan([(tiles[k]["source"], tiles[k]["index"]) for k in auto])
            scan = {k: (r["min"], r["max"]) for k, r in zip(auto, res)}
        return self._render(ecology_levels(tiles, scan), want_stacks)

    def plankton(self, t_days, species=0, want_stacks=False):
        e = self.configure()
        self.vmax = plankton_vmax(e["vmax_env"], self._order_stats("PLANKTON", species))
        return self._render([plankton_tile(t_days, species, self.vmax)], want_stacks)

    def isr(self, t_days, want_stacks=False):
        self.configure()
        a, b = self.dev.tiles_scan([("ISR_A", 0), ("ISR_B", 0)])
        tiles = isr_tiles(t_days, a["argmax_value"], b["argmax_value"], a["argmax"], b["argmax"])
        g = self.dev.grid
        self.line = separation_line(t_days, g.lat, g.lon, a["argmax"], b["argmax"])
        return self._render(tiles, want_stacks)

    def bands(self):
        return self.dev.tiles_bands()

    def planes(self):
        return self.dev.tiles_planes()

    # -- one firing each: the PNG and its .json sidecar -> the path(s)
    def _write(self, path, img, figure, t_days, **extra):
        from .imgio import write_png
        os.makedirs(os.path.dirname(path) or ".", exist_ok=True)
        write_png(path, img)
        g = self.dev.grid
        with open(path[:-4] + ".json", "w", encoding="utf-8") as f:
            json.dump(sidecar(figure, self.tiles, t_days, g.lat, g.lon, **extra), f, ensure_ascii=False, indent=1)
        return path

    @staticmethod
    def _out(output_dir):
        return output_dir if output_dir is not None else os.environ.get("QD_OUTPUT_DIR", "output")

    def write_ecology(self, t_days, output_dir=None):
        img = self.ecology(t_days)
        return self._write(os.path.join(self._out(output_dir), ecology_name(t_days)), img, "ecology", t_days)

    def write_plankton(self, t_days, output_dir=None):
        """species 0, and species 1 when there are at least two (run_simulation.py:884-886) -> the paths."""
        S = self.n_phyto()
        if S <= 0:
            return []
        out = []
        for s in ((0, 1) if S >= 2 else (0,)):
            img = self.plankton(t_days, s)
            out.append(self._write(os.path.join(self._out(output_dir), plankton_name(s, t_days)), img, "plankton", t_days, species=s,
                                   vmax=float(self.vmax)))
        return out

    def write_isr(self, t_days, output_dir=None, echo=None):
        """-> (path, the [Diagnostics] line).  echo: called with the line before the file is written, as the reference prints it."""
        img = self.isr(t_days)
        if echo is not None:
            echo(self.line)
        return self._write(os.path.join(self._out(output_dir), isr_name(t_days)), img, "isr_components", t_days, diagnostics=self.line), self.line


def eco_or_forced(fig, eco):
    """The scalar alpha tile needs an ecology (the reference's last_alpha_ecology_map stays None without one) unless the caller of a
    bare Device said that the map exists."""
    return eco is not None or fig._alpha is not None
