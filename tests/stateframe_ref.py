"""NumPy restatement of the state frame (qingdai_amd/stateframe.py, csrc/qd_stateframe.hip): the fifteen fields of plot_state
(scripts/run_simulation.py:345-498) in its operation order, the extremes and argmax cells the level rules need, the band rule,
the overlays and the mosaic.  The level rules and the band colours themselves are the product's host code
(stateframe.build_table), which tests/test_stateframe_cpu.py checks against matplotlib's recorded output.

Band rule: a cell takes band i with levels[i] <= z < levels[i + 1]; the last band is closed above; a non-finite z or a z outside
every band is white (-1); with extend="max" a z above the top level takes the extended band, index len(levels) - 1.

VORT_TOL: the vorticity is a stencil; the device and this file agree with the reference to the tolerance of the operator test
(tests/test_gpu_parity.py OP_TOL = 1e-13 of the field's max-norm), not bit for bit.
"""
import json
import os

import numpy as np

VORT_TOL = 1e-13
INPUTS = {"TS": "T_s", "H": "h", "SST": "SST", "PRECIP": "precip", "CLOUD": "cloud", "U": "u", "V": "v", "UO": "uo", "VO": "vo",
          "ISR": "isr", "ISR_A": "isr_A", "ISR_B": "isr_B", "ALBEDO": "albedo", "OLR": "olr", "Q": "q", "EFLUX": "E", "PCOND": "P_cond"}
AUTO_PANELS = (3, 7, 8, 9, 10, 12, 13, 14, 15)
GUTTER = 4
RIVER_RGB, LAKE_RGB = (0.0, 0.749, 1.0), (0.118, 0.565, 1.0)


def golden_meta(z):
    return json.loads(str(z["meta"]))


def set_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def vorticity(u, v, lat, a):
    """grid.py:70-88 as qd_op_vorticity evaluates it: both axes by centred differences, the longitude periodic, the latitude
    derivative zero on the two pole rows, 1 / (a max(cos, 1e-6)) in front."""
    n_lat, n_lon = u.shape
    dlat = np.deg2rad(lat[1] - lat[0])
    dlon = np.deg2rad(np.linspace(0, 360, n_lon)[1])
    cos = np.cos(np.deg2rad(lat))[:, None]
    dv = (np.roll(v, -1, axis=1) - np.roll(v, 1, axis=1)) / (2 * dlon)
    uc = u * cos
    du = np.zeros_like(u)
    du[1:-1] = (uc[2:] - uc[:-2]) / (2 * dlat)
    return (1 / (a * np.maximum(cos, 1e-6))) * (dv - du)


def fields(inp, lat, ps_abs=False, ocean=True, p0=1.0e5, rho_a=1.2, H=8000.0, a=None):
    """-> [15, n_lat, n_lon]: what plot_state hands to contourf (and, for the panels 7 and 8, to streamplot's color)."""
    if a is None:
        from qingdai_amd import QdParams
        a = QdParams().a
    g = 9.81
    with np.errstate(all="ignore"):
        T_a = 288.0 + (g / 1004.0) * inp["h"]
        ps = (p0 + rho_a * g * inp["h"]) * 1e-2 if ps_abs else (rho_a * g * inp["h"]) * 1e-2
        if ocean:
            p8 = np.sqrt(np.nan_to_num(inp["uo"]) ** 2 + np.nan_to_num(inp["vo"]) ** 2)
        else:
            p8 = inp["h"] - float(H)
        out = [np.nan_to_num(inp["T_s"] - 273.15), T_a - 273.15, ps, np.nan_to_num((inp["SST"] if ocean else inp["T_s"]) - 273.15),
               np.nan_to_num(inp["precip"]) * 86400.0, np.asarray(inp["cloud"], dtype=float),
               np.sqrt(np.nan_to_num(inp["u"]) ** 2 + np.nan_to_num(inp["v"]) ** 2), p8, vorticity(inp["u"], inp["v"], lat, a),
               np.asarray(inp["isr"], dtype=float), np.asarray(inp["albedo"], dtype=float), np.asarray(inp["olr"], dtype=float),
               1e3 * np.nan_to_num(inp["q"]), np.nan_to_num(inp["E"]) * 86400.0, np.nan_to_num(inp["P_cond"]) * 86400.0]
    return np.stack(out)


def scan(F, isr_A, isr_B):
    """The dict qingdai_amd.stateframe.unpack_scan makes of the device's reductions, from a field stack with NumPy."""
    with np.errstate(all="ignore"):
        t = [F[0], F[1], F[3]]
        auto = {}
        for p in AUTO_PANELS:
            z = F[p - 1][np.isfinite(F[p - 1])]
            auto[p] = (float(z.min()), float(z.max())) if z.size else (float("inf"), float("-inf"))
        av = np.abs(F[8])
        vmax = float(np.nanmax(av)) if not np.isnan(av).all() else float("nan")
    a, b = int(np.argmax(isr_A)), int(np.argmax(isr_B))
    return {"t_min": np.array([x.min() for x in t]), "t_max": np.array([x.max() for x in t]), "auto": auto, "vmax": vmax, "marks": [a, b],
            "mark_values": [float(np.ravel(isr_A)[a]), float(np.ravel(isr_B)[b])]}


def band_index(z, levels, extend=False):
    """-> int8 map: the band of every cell, -1 = white."""
    z = np.asarray(z, dtype=float)
    out = np.full(z.shape, -1, dtype=np.int8)
    if levels is None:
        return out
    lev = np.asarray(levels, dtype=float)
    n = len(lev)
    with np.errstate(all="ignore"):
        for i in range(n - 1):
            out[(z >= lev[i]) & (z < lev[i + 1])] = i
        out[z == lev[-1]] = n - 2
        if extend:
            out[(z > lev[-1]) & np.isfinite(z)] = n - 1
    return out


def near_level(z, levels, rel=1e-9):
    """Cells within rel * (levels[-1] - levels[0]) of a level: where a field that agrees only to a tolerance may pick the other band."""
    if levels is None:
        return np.zeros(np.shape(z), dtype=bool)
    lev = np.asarray(levels, dtype=float)
    with np.errstate(all="ignore"):
        d = np.min(np.abs(np.asarray(z, dtype=float)[..., None] - lev), axis=-1)
    return d <= rel * (lev[-1] - lev[0])


def coast(land):
    """A land cell (== 1) with at least one ocean (== 0) 4-neighbour; longitude periodic, latitude clipped."""
    land = np.asarray(land)
    oc = land == 0
    up, down = np.vstack([oc[1:], oc[-1:]]), np.vstack([oc[:1], oc[:-1]])
    return (land == 1) & (up | down | np.roll(oc, 1, axis=1) | np.roll(oc, -1, axis=1))


def marks(shape, cell, plus):
    """The pixels of one star mark: the centre and its 4 diagonals (x) or orthogonals (+); columns wrap, rows outside are dropped."""
    m = np.zeros(shape, dtype=bool)
    if cell < 0:
        return m
    r, c = divmod(int(cell), shape[1])
    offs = [(0, 0), (0, 1), (0, -1), (1, 0), (-1, 0)] if plus else [(0, 0), (1, 1), (1, -1), (-1, 1), (-1, -1)]
    for dr, dc in offs:
        if 0 <= r + dr < shape[0]:
            m[r + dr, (c + dc) % shape[1]] = True
    return m


def quantise(rgb):
    with np.errstate(all="ignore"):
        return np.clip(np.floor(np.asarray(rgb) * 255.0 + 0.5), 0.0, 255.0).astype(np.uint8)


def render(F, tab, land, flow=None, lake=None, river_min=1e6, river_alpha=0.35, lake_alpha=0.40):
    """F: the field stack; tab: stateframe.build_table's result -> (int8 bands [15, lat, lon], u8 mosaic)."""
    n_lat, n_lon = F.shape[1:]
    land = np.asarray(land)
    bands = np.stack([band_index(F[k], p["levels"], p["extend"]) for k, p in enumerate(tab["panels"])])
    img = np.full((5 * n_lat + 6 * GUTTER, 3 * n_lon + 4 * GUTTER, 3), 255, dtype=np.uint8)
    cst = coast(land)
    for k, p in enumerate(tab["panels"]):
        rgb = np.ones((n_lat, n_lon, 3))
        if p["levels"] is not None:
            sel = bands[k] >= 0
            rgb[sel] = np.asarray(p["colours"])[bands[k][sel]]
        if p["coast"]:
            rgb[cst] = 0.0 if p["coast"] == 1 else 1.0
        if k in (0, 7):
            if flow is not None:
                m = (np.asarray(flow) >= river_min) & (land == 1)
                rgb[m] = rgb[m] * (1.0 - river_alpha) + np.array(RIVER_RGB) * river_alpha
            if lake is not None:
                m = np.asarray(lake) != 0
                rgb[m] = rgb[m] * (1.0 - lake_alpha) + np.array(LAKE_RGB) * lake_alpha
        if k == 9:
            rgb[marks((n_lat, n_lon), tab["marks"][0], plus=False)] = (0.0, 1.0, 1.0)
            rgb[marks((n_lat, n_lon), tab["marks"][1], plus=True)] = (1.0, 1.0, 0.0)
        y0, x0 = GUTTER + (k // 3) * (n_lat + GUTTER), GUTTER + (k % 3) * (n_lon + GUTTER)
        img[y0:y0 + n_lat, x0:x0 + n_lon] = quantise(rgb)[::-1]
    return bands, img


def tile(img, k, n_lat, n_lon):
    """The pixels of panel k (0-based) of a mosaic, in grid order (southernmost row first)."""
    y0, x0 = GUTTER + (k // 3) * (n_lat + GUTTER), GUTTER + (k % 3) * (n_lon + GUTTER)
    return img[y0:y0 + n_lat, x0:x0 + n_lon][::-1]
