"""NumPy restatement of the figure tiles (qingdai_amd/figures.py, csrc/qd_tiles.hip): the planes plot_ecology,
plot_plankton_species and plot_isr_components hand to contourf (scripts/run_simulation.py:828-1060; the two stack maps as
pygcm/ecology/population.py:296-341 computes them), the scan, and the mosaic of one row of tiles.  Band rule, coast, marks and
quantisation are those of tests/stateframe_ref.py.  The goldens (tests/golden/figures_*.npz, scripts/gen_golden_figures.py) hold what
matplotlib and the reference's own functions recorded; tests/test_figures_cpu.py holds this file to them."""
import glob
import os

import numpy as np

from stateframe_ref import band_index, coast, marks, quantise, golden_meta, set_env, GUTTER      # noqa: F401

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDENS = sorted(glob.glob(os.path.join(HERE, "golden", "figures_*_19x36.npz")))
ECO_SOURCES = (("LAI", 0), ("ALPHA", 0), ("ALPHA_BANDED", 0), ("CANOPY_HEIGHT", 0), ("SPECIES_DENSITY", 0))


def case_of(path):
    return os.path.basename(path)[len("figures_"):-len("_19x36.npz")]


def canopy_height(layers, land, h_scale=10.0):
    """nan_to_num(canopy_height_map()), layered branch."""
    K = layers.shape[1]
    with np.errstate(all="ignore"):
        idx = np.arange(1, K + 1, dtype=float)[None, :, None, None] / float(K)
        by_k = np.sum(np.maximum(layers, 0.0), axis=0)
        H = h_scale * (np.sum(idx[0] * by_k, axis=0) / (np.sum(by_k, axis=0) + 1e-12))
    out = np.full(land.shape, np.nan)
    out[land == 1] = H[land == 1]
    return np.nan_to_num(out)


def species_density(layers, land, s):
    with np.errstate(all="ignore"):
        L_s = np.sum(np.maximum(layers, 0.0), axis=1)
    out = np.full(land.shape, np.nan)
    out[land == 1] = L_s[s][land == 1]
    return np.nan_to_num(out)


def plane(source, index, inp, h_scale=10.0):
    """inp: "land_mask", "lai", "alpha", "banded", "layers" [S, K, lat, lon], "C" [S, lat, lon], "isr_A", "isr_B"."""
    land = np.asarray(inp["land_mask"])
    if source == "LAI":
        return np.nan_to_num(inp["lai"])
    if source == "ALPHA":
        return np.nan_to_num(inp["alpha"])
    if source in ("ALPHA_BANDED", "HOST_PLANE"):
        return np.nan_to_num(inp["banded"])
    if source == "CANOPY_HEIGHT":
        return canopy_height(np.asarray(inp["layers"]), land, h_scale)
    if source == "SPECIES_DENSITY":
        return species_density(np.asarray(inp["layers"]), land, index)
    if source == "PLANKTON":
        f = np.array(inp["C"][index], dtype=float)
        f[land == 1] = np.nan
        return f
    return np.asarray(inp["isr_A" if source == "ISR_A" else "isr_B"], dtype=float)


def scan(z):
    """What qd_tiles_scan returns for one plane."""
    z = np.asarray(z, dtype=float)
    fin = z[np.isfinite(z)]
    cell = int(np.argmax(z))
    return {"min": float(fin.min()) if fin.size else float("inf"), "max": float(fin.max()) if fin.size else float("-inf"),
            "nan": bool(np.isnan(z).any()), "argmax": cell, "argmax_value": float(z.ravel()[cell])}


def render(planes, tiles, land):
    """planes: [n, lat, lon] (anything for an unavailable tile); tiles: the dicts of qingdai_amd.figures -> (int8 bands [n, lat, lon],
    the u8 mosaic)."""
    n = len(tiles)
    n_lat, n_lon = np.asarray(land).shape
    bands = np.full((n, n_lat, n_lon), -1, dtype=np.int8)
    img = np.full((n_lat + 2 * GUTTER, n * n_lon + (n + 1) * GUTTER, 3), 255, dtype=np.uint8)
    cst = coast(land)
    for k, t in enumerate(tiles):
        rgb = np.ones((n_lat, n_lon, 3))
        if t["levels"] is not None and not t["constant"] and not t["unavailable"]:
            bands[k] = band_index(planes[k], t["levels"], t["extend"])
            on = bands[k] >= 0
            rgb[on] = np.asarray(t["colours"])[bands[k][on]]
        if t["coast"]:
            rgb[cst] = 1.0 if t["coast"] == 2 else 0.0
        if t["mark"] is not None and t["mark"][1] >= 0:
            plus = t["mark"][0] == 2
            rgb[marks((n_lat, n_lon), t["mark"][1], plus)] = (1.0, 1.0, 0.0) if plus else (0.0, 1.0, 1.0)
        x0 = GUTTER + k * (n_lon + GUTTER)
        img[GUTTER:GUTTER + n_lat, x0:x0 + n_lon] = quantise(rgb)[::-1]
    return bands, img


def tile(img, k, n_lat, n_lon):
    """The pixels of tile k (0-based) of a mosaic, in grid order (southernmost row first)."""
    x0 = GUTTER + k * (n_lon + GUTTER)
    return img[GUTTER:GUTTER + n_lat, x0:x0 + n_lon][::-1]


def golden_tiles(z, meta, fig):
    """{tile number: (field, levels, colours, tile meta)} of one figure of a golden."""
    return {t["tile"]: (z[f"{fig}_{t['tile']}_field"], z[f"{fig}_{t['tile']}_levels"], z[f"{fig}_{t['tile']}_colours"], t)
            for t in meta["figures"][fig]["tiles"]}


def host_order_stats(z):
    """The order statistics of a plane with np.sort, in the calling convention of figures.nanpercentile."""
    v = np.sort(np.asarray(z, dtype=float).ravel())
    v = v[~np.isnan(v)]
    return lambda ranks: (int(v.size), np.array([v[r] if r < v.size else np.nan for r in ranks], dtype=float))
