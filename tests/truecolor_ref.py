"""NumPy restatement of the true-colour frame (qingdai_amd/csrc/qd_truecolor.hip), written from the stage list of DESIGN.md, and
the helpers the two truecolor test modules share: a golden's environment, the stand-ins its configuration is built from, and the
u8 rounding.  `render` takes the same parameter struct and tables the device takes."""
import json
import os
import types

import numpy as np

OCEAN, LAND, ICE = (0.10, 0.20, 0.50), (0.40, 0.30, 0.20), (0.90, 0.90, 0.95)
RIVER, LAKE = (0.05, 0.35, 0.90), (0.15, 0.55, 0.95)
# Tolerance of the f64 rgb and of the two sea-ice numbers against the goldens (absolute; the values lie in [0, 1] and [0, a few m]).
# exp and pow are the only operations whose rounding may differ from NumPy's; the sea-ice sums are taken in a blocked order.  The
# bound in force is ten times the largest deviation measured on the MI355X over the goldens, and no looser than START.
START = 1e-12
MEASURED = 2.3e-16                 # largest |device - golden| measured on the MI355X (2.220e-16, rounded up): the sea-ice numbers; rgb 1.110e-16
BOUND = START if MEASURED is None else min(START, 10 * MEASURED)
FIELDS = {"HICE": "h_ice", "C_SNOW": "C_snow", "CLOUD": "cloud", "TS": "T_s", "ISR": "isr", "ISR_A": "isr_A", "ISR_B": "isr_B", "ECO_F": "eco_f"}


def _pow(x, e):
    return x ** e


def _wrel(tab, isr_A, isr_B, isr):
    """tab rows: specA, specB, T_ray -> w_rel [nb, lat, lon]."""
    sa, sb, tr = tab
    S = (sa[:, None, None] * isr_A + sb[:, None, None] * isr_B) * tr[:, None, None]
    ssum = S[0].copy()
    for b in range(1, S.shape[0]):
        ssum = ssum + S[b]
    tot = isr_A + isr_B
    pos = (ssum > 1e-12) & (tot > 1e-12)
    with np.errstate(all="ignore"):
        I = np.where(pos, (S / ssum) * tot, 0.0)
    I = np.where(np.isfinite(I), I, 0.0)
    itot = np.maximum(isr, 0.0)
    with np.errstate(all="ignore"):
        return np.where(itot > 1e-12, I / (itot + 1e-12), 0.0)


def _channels(A, w3, wrel):
    out = []
    for w in w3:
        acc = None
        for b in range(A.shape[0]):
            t = A[b] * (w[b] * wrel[b])
            t = np.where(np.isnan(t), 0.0, t)
            acc = t if acc is None else acc + t
        out.append(np.clip(acc, 0.0, 1.0))
    return out


def render(inp, p, eco_tab=None, phyto_tab=None, phyto_bands=None, lake_mask=None, flow=None, lat=None):
    """inp: dict with land_mask, h_ice, C_snow, cloud, T_s, isr, isr_A, isr_B, eco_f -> dict(rgb, sea_ice_mask, sea_ice, img)."""
    land_mask = np.asarray(inp["land_mask"])
    ocean, land = land_mask == 0, land_mask == 1
    shape = land_mask.shape
    with np.errstate(all="ignore"):
        rgb = [np.where(ocean, OCEAN[c], np.where(land, LAND[c], 0.0)) for c in range(3)]
        h = np.asarray(inp["h_ice"], dtype=float)
        ice_frac = 1.0 - np.exp(-np.maximum(h, 0.0) / max(1e-6, p.h_ice_ref))
        sea_ice = ocean & (ice_frac >= p.ice_frac_thr)
        rgb = [np.where(sea_ice, ICE[c], rgb[c]) for c in range(3)]
        if p.snow_by_swe:
            C = np.nan_to_num(inp["C_snow"], nan=0.0)
            m = land & (C >= p.snow_cover_frac)
            al = p.snow_vis_alpha * np.clip(C, 0.0, 1.0)
            rgb = [np.where(m, rgb[c] * (1.0 - al) + ICE[c] * al, rgb[c]) for c in range(3)]
        if p.veg:
            nb = p.nb_eco
            fraw = np.where(land, 1.0 if p.veg_f_one else np.asarray(inp["eco_f"], dtype=float), np.nan)
            fn = np.where(land, 1.0, 0.0) if p.veg_f_one else np.nan_to_num(fraw, nan=0.0)
            A = np.stack([np.where(land, np.clip(eco_tab[0][b] * fraw + (1.0 - fraw) * p.soil_ref, 0.0, 1.0), np.nan) for b in range(nb)])
            v = _channels(A, eco_tab[1:4], _wrel(eco_tab[4:7], inp["isr_A"], inp["isr_B"], inp["isr"]))
            if p.veg_gamma > 0:
                v = [_pow(x, 1.0 / p.veg_gamma) for x in v]
            if p.veg_sat != 1.0:
                m = ((v[0] + v[1]) + v[2]) / 3.0
                v = [np.clip(m + p.veg_sat * (x - m), 0.0, 1.0) for x in v]
            f = np.clip(fn, 0.0, 1.0)
            rgb = [np.where(land, rgb[c] * (1.0 - f) + v[c] * f, rgb[c]) for c in range(3)]
        if p.oceancolor and phyto_bands is not None:
            v = _channels(np.asarray(phyto_bands, dtype=float), phyto_tab[0:3], _wrel(phyto_tab[3:6], inp["isr_A"], inp["isr_B"], inp["isr"]))
            if p.oc_gamma > 0:
                v = [_pow(x, 1.0 / p.oc_gamma) for x in v]
            open_ocean = ocean & ~sea_ice
            rgb = [np.where(open_ocean, rgb[c] * (1.0 - p.oc_blend) + v[c] * p.oc_blend, rgb[c]) for c in range(3)]
        if p.snow_by_ts:
            m = land & (np.asarray(inp["T_s"]) <= p.snow_thresh)
            rgb = [np.where(m, 0.97 * ICE[c], rgb[c]) for c in range(3)]
        ca = p.cloud_alpha * np.asarray(inp["cloud"], dtype=float)
        rgb = [rgb[c] * (1.0 - ca) + ca * p.cloud_white for c in range(3)]
        land_f = land.astype(float)
        if p.rivers:
            am = p.river_alpha * ((np.asarray(flow) >= p.river_min).astype(float) * land_f)
            rgb = [rgb[c] * (1.0 - am) + RIVER[c] * am for c in range(3)]
        if p.lakes:
            am = p.lake_alpha * (np.asarray(lake_mask).astype(float) * land_f)
            rgb = [rgb[c] * (1.0 - am) + LAKE[c] * am for c in range(3)]
        out = np.clip(np.stack(rgb, axis=-1), 0.0, 1.0)
    lat = np.linspace(-90.0, 90.0, shape[0]) if lat is None else np.asarray(lat)
    w = np.repeat(np.maximum(np.cos(np.deg2rad(lat)), 0.0)[:, None], shape[1], axis=1)
    nums = np.array([float((w * sea_ice).sum() / (w.sum() + 1e-15)), float(h[sea_ice].mean()) if sea_ice.any() else 0.0])
    return {"rgb": out, "sea_ice_mask": sea_ice, "sea_ice": nums, "img": quantise(out)}


def quantise(rgb):
    """The u8 image of an rgb map: min(255, floor(x 255 + 0.5)), NaN -> 0, northernmost row first."""
    with np.errstate(all="ignore"):
        q = np.minimum(255.0, np.floor(np.asarray(rgb) * 255.0 + 0.5))
    return np.where(np.isnan(q), 0.0, q).astype(np.uint8)[::-1]


# ---- goldens
def golden_meta(z):
    return json.loads(str(z["meta"]))


def set_env(monkeypatch, env=None):
    for k in [k for k in os.environ if k.startswith("QD_")]:
        monkeypatch.delenv(k)
    for k, v in (env or {}).items():
        monkeypatch.setenv(str(k), str(v))


def stand_ins(z):
    """(eco, phyto, routing) stand-ins of a golden, as qingdai_amd.truecolor.build_config reads them; the environment of the golden
    must be set (set_env): the band sets and the star tables come from it."""
    from qingdai_amd import spectral as sp
    meta = golden_meta(z)
    eco = phyto = routing = None
    if meta["has_eco"]:
        R = np.asarray(z["eco_R_eff"], dtype=float)
        pop = types.SimpleNamespace(effective_leaf_reflectance_bands=lambda nb: R) if meta["use_lai"] else None
        eco = types.SimpleNamespace(bands=sp.make_bands(), pop=pop, R_leaf=R,
                                    params=types.SimpleNamespace(soil_ref=float(os.environ.get("QD_ECO_SOIL_REFLECT", "0.20"))))
    if meta["nb_phyto"]:
        phyto = types.SimpleNamespace(bands=sp.make_bands(nbands=meta["nb_phyto"]))
    if meta["has_routing"]:
        routing = types.SimpleNamespace(lake_mask=np.asarray(z["lake_mask"]))
    return eco, phyto, routing


def golden_config(z):
    """-> (params, eco_tab, phyto_tab, lake, phyto_bands or None, flow or None) of a golden under its environment."""
    from qingdai_amd.truecolor import build_config
    meta = golden_meta(z)
    p, eco_tab, phyto_tab, lake = build_config(None, *stand_ins(z))
    return (p, eco_tab, phyto_tab, lake, np.asarray(z["phyto_bands"]) if meta["nb_phyto"] else None,
            np.asarray(z["flow"]) if meta["has_routing"] else None)
