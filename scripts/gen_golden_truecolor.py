"""Regenerate tests/golden/truecolor_<case>_19x36.npz from the reference's plot_true_color (scripts/run_simulation.py:539-778).

Needs a checkout of the reference project (default ../reference next to this repository, or --reference DIR) and matplotlib, which
the reference driver imports.  Each case builds 19 x 36 inputs by hand, sets the case's QD_* environment and calls the reference's
plot_true_color with stand-ins for the objects it reads: a namespace with the model fields for `gcm`, the reference's real
EcologyAdapter for `eco` (its canopy cache set to the case's factor map), a namespace with bands and get_alpha_maps for `phyto`,
a namespace with diagnostics() and lake_mask for `routing`.  matplotlib.pyplot's subplots, savefig and close are replaced for the
call, so that the array handed to imshow is captured and no figure is made; the printed [TrueColor] line is captured too.

The golden holds the inputs, the environment of the case, what the adapter contributed (R_eff, the band centres), and the outputs:
rgb (the array given to imshow), the sea-ice mask, the two sea-ice numbers and the printed line.

The sea-ice mask comes from a computed exp, and one ulp can flip it: the script asserts that no cell of any case has
|ice_frac - thr| < 1e-9.  Thresholds compared against raw inputs (C_snow, flow, T_s) carry exact ties on purpose.
"""
import argparse
import contextlib
import io
import json
import os
import re
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "tests", "golden")
NLAT, NLON = 19, 36


def base_inputs(rng):
    land = (rng.uniform(size=(NLAT, NLON)) < 0.45).astype(np.int64)
    land[:, 28:34] = 0                                  # an ocean basin
    land[3:8, 4:12] = 1                                 # a continent
    land[NLAT - 2:, 10:20] = 1                          # land on the northern pole rows
    h_ice = np.where(rng.uniform(size=(NLAT, NLON)) < 0.5, 0.0, rng.uniform(0.0, 0.06, (NLAT, NLON)))
    h_ice[NLAT - 4:, :] = rng.uniform(0.2, 2.5, (4, NLON))     # the northern cap only: the two hemispheres differ
    h_ice[0, 0:6] = rng.uniform(0.1, 0.3, 6)
    C = np.where(rng.uniform(size=(NLAT, NLON)) < 0.5, 0.0, rng.uniform(0.0, 1.3, (NLAT, NLON)))
    cloud = rng.uniform(0.0, 1.0, (NLAT, NLON))
    cloud[rng.uniform(size=(NLAT, NLON)) < 0.2] = 0.0
    T_s = rng.uniform(255.0, 300.0, (NLAT, NLON))
    isr_A = rng.uniform(0.0, 700.0, (NLAT, NLON))
    isr_B = rng.uniform(0.0, 400.0, (NLAT, NLON))
    isr_B[:, 0:9] = 0.0                                 # one star below the horizon
    return dict(land_mask=land, h_ice=h_ice, C_snow=C, cloud=cloud, T_s=T_s, isr_A=isr_A, isr_B=isr_B, isr=isr_A + isr_B,
                eco_f=rng.uniform(0.0, 1.0, (NLAT, NLON)), flow=np.zeros((NLAT, NLON)), lake_mask=np.zeros((NLAT, NLON), dtype=np.uint8),
                phyto_bands=np.zeros((0, NLAT, NLON)))


def night_side(d):
    for k in ("isr_A", "isr_B", "isr"):
        d[k][:, NLON // 2:] = 0.0


def flow_map(rng, d, river_min):
    land = d["land_mask"] == 1
    flow = np.where(land, 10.0 ** rng.uniform(3.0, 8.0, (NLAT, NLON)), 0.0)
    flow[3:8, 4:8] = river_min                          # exactly at the threshold: a river (>=)
    flow[3:8, 8:12] = np.nextafter(river_min, 0.0)      # one ulp below: none
    flow[10, 30] = 5.0 * river_min                      # a large flow on an ocean cell: masked by land
    d["flow"] = flow
    lake = ((rng.uniform(size=(NLAT, NLON)) < 0.1) & land).astype(np.uint8)
    lake[9, 31] = 1                                     # a lake flag on an ocean cell: masked by land
    d["lake_mask"] = lake


def phyto_stack(rng, d, nb):
    A = rng.uniform(0.01, 0.25, (nb, NLAT, NLON))
    A[:, d["land_mask"] == 1] = np.nan                  # the reference's maps hold NaN on land
    d["phyto_bands"] = A


def case_base(rng):
    d = base_inputs(rng)
    land = d["land_mask"] == 1
    d["C_snow"][4, 4:8] = 0.20                          # exactly at the cover threshold: snow (>=)
    d["C_snow"][5, 4:8] = np.nextafter(0.20, 0.0)
    d["C_snow"][6, 4:8] = np.nan                        # nan_to_num -> 0: no snow
    assert land[4:7, 4:8].all()
    return d, {}, dict(eco=False, phyto_nb=0, routing=False)


def case_veg(rng):
    d = base_inputs(rng)
    night_side(d)
    return d, {"QD_ECO_NS": "3", "QD_ECO_SPECIES_WEIGHTS": "0.5,0.3,0.2", "QD_ECO_SPECIES_1_PEAKS": "440:30:0.7,660:25:0.9"}, \
        dict(eco=True, phyto_nb=0, routing=False)


def case_veg_nolai(rng):
    d, env, has = case_veg(rng)
    env = dict(env, QD_ECO_USE_LAI="0")
    return d, env, has


def case_oceancolour(rng):
    d = base_inputs(rng)
    phyto_stack(rng, d, 8)
    return d, {}, dict(eco=False, phyto_nb=8, routing=False)


def case_rivers(rng):
    d = base_inputs(rng)
    flow_map(rng, d, 1e6)
    return d, {}, dict(eco=False, phyto_nb=0, routing=True)


def case_all_nondefault(rng):
    d = base_inputs(rng)
    night_side(d)
    phyto_stack(rng, d, 5)
    flow_map(rng, d, 2.5e5)
    d["T_s"][3:5, 4:12] = 268.0                         # exactly at the threshold: snow (<=)
    d["T_s"][5:8, 4:12] = np.nextafter(268.0, 300.0)
    env = {"QD_HICE_REF": "0.8", "QD_TRUECOLOR_ICE_FRAC": "0.3", "QD_SNOW_COVER_FRAC": "0.35", "QD_SNOW_VIS_ALPHA": "0.8",
           "QD_ECO_TRUECOLOR_GAMMA": "2.4", "QD_ECO_TRUECOLOR_SAT": "0.7", "QD_OC_GAMMA": "1.6", "QD_OC_BLEND": "0.5",
           "QD_TRUECOLOR_SNOW_BY_TS": "1", "QD_SNOW_THRESH": "268.0", "QD_TRUECOLOR_CLOUD_ALPHA": "0.35",
           "QD_TRUECOLOR_CLOUD_WHITE": "0.9", "QD_RIVER_MIN_KGPS": "2.5e5", "QD_RIVER_ALPHA": "0.7", "QD_LAKE_ALPHA": "0.25",
           "QD_ECO_TOA_TO_SURF_MODE": "rayleigh", "QD_ECO_NS": "4", "QD_ECO_SPECTRAL_BANDS": "12", "QD_ECO_SOIL_REFLECT": "0.3"}
    return d, env, dict(eco=True, phyto_nb=5, routing=True)


def case_nonfinite(rng):
    d = base_inputs(rng)
    phyto_stack(rng, d, 8)
    flow_map(rng, d, 1e6)
    ocean = np.argwhere(d["land_mask"] == 0)
    land = np.argwhere(d["land_mask"] == 1)
    for (j, i) in ocean[[3, 40, 90]]:
        d["h_ice"][j, i] = np.nan                       # NaN >= thr is False: open ocean, and out of the mean
    d["h_ice"][NLAT - 1, 30] = np.nan
    for (j, i) in land[[2, 30, 77]]:
        d["eco_f"][j, i] = np.nan                       # nan_to_num -> 0: bare soil colour
    j, i = land[50]
    d["cloud"][j, i] = np.nan                           # the reference leaves that pixel NaN
    return d, {"QD_ECO_NS": "2"}, dict(eco=True, phyto_nb=8, routing=True)


CASES = {"base": case_base, "veg": case_veg, "veg_nolai": case_veg_nolai, "oceancolour": case_oceancolour, "rivers": case_rivers,
         "all_nondefault": case_all_nondefault, "nonfinite": case_nonfinite}


def run_case(name, ref):
    rs, adapter, spectral = ref
    rng = np.random.default_rng(sum(map(ord, "truecolor_" + name)))
    d, env, has = CASES[name](rng)
    env = dict(env, QD_ECO_DIAG="0")
    for k in [k for k in os.environ if k.startswith("QD_")]:
        del os.environ[k]
    os.environ.update(env)
    lat = np.linspace(-90.0, 90.0, NLAT)
    lon = np.linspace(0.0, 360.0, NLON)
    lon_mesh, lat_mesh = np.meshgrid(lon, lat)
    grid = types.SimpleNamespace(n_lat=NLAT, n_lon=NLON, lat=lat, lon=lon, lat_mesh=lat_mesh, lon_mesh=lon_mesh)
    gcm = types.SimpleNamespace(h_ice=d["h_ice"], C_snow_map_last=d["C_snow"], T_s=d["T_s"], cloud_cover=d["cloud"], isr=d["isr"],
                                isr_A=d["isr_A"], isr_B=d["isr_B"])
    land = d["land_mask"]
    eco = phyto = routing = None
    extra = {"eco_R_eff": np.zeros(0), "eco_lambda": np.zeros(0), "phyto_lambda": np.zeros(0)}
    if has["eco"]:
        eco = adapter.EcologyAdapter(grid, land)
        nb = eco.bands.nbands
        if eco.pop is not None:
            eco.pop._canopy_f_cached = d["eco_f"].copy()
            extra["eco_R_eff"] = np.asarray(eco.pop.effective_leaf_reflectance_bands(nb), dtype=float)
        else:
            extra["eco_R_eff"] = np.asarray(eco.R_leaf, dtype=float)
        extra["eco_lambda"] = np.asarray(eco.bands.lambda_centers, dtype=float)
    if has["phyto_nb"]:
        bands = spectral.make_bands(nbands=has["phyto_nb"])
        stack = d["phyto_bands"]
        phyto = types.SimpleNamespace(bands=bands, get_alpha_maps=lambda: (stack, None))
        extra["phyto_lambda"] = np.asarray(bands.lambda_centers, dtype=float)
    if has["routing"]:
        routing = types.SimpleNamespace(diagnostics=lambda: {"flow_accum_kgps": d["flow"]}, lake_mask=d["lake_mask"])
    shown = {}
    ax = types.SimpleNamespace(imshow=lambda a, **kw: shown.update(rgb=np.array(a, dtype=float, copy=True), kw=kw),
                               set_title=lambda *a, **k: None, set_xlabel=lambda *a, **k: None, set_ylabel=lambda *a, **k: None)
    saved = (rs.plt.subplots, rs.plt.savefig, rs.plt.close)
    rs.plt.subplots = lambda *a, **k: (object(), ax)
    rs.plt.savefig = lambda *a, **k: shown.update(filename=a[0])
    rs.plt.close = lambda *a, **k: None
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf), np.errstate(all="ignore"):
            rs.plot_true_color(grid, gcm, land, 12.25, "out", routing=routing, eco=eco, phyto=phyto)
    finally:
        rs.plt.subplots, rs.plt.savefig, rs.plt.close = saved
    line = [ln for ln in buf.getvalue().splitlines() if ln.startswith("[TrueColor]")]
    assert len(line) == 1 and shown["kw"].get("origin") == "lower" and os.path.basename(shown["filename"]) == "true_color_day_012.2.png"
    rgb = shown["rgb"]
    assert rgb.shape == (NLAT, NLON, 3)
    # the condition on the inputs: no cell within 1e-9 of the sea-ice threshold
    href, thr = float(env.get("QD_HICE_REF", "0.5")), float(env.get("QD_TRUECOLOR_ICE_FRAC", "0.15"))
    with np.errstate(all="ignore"):
        ice_frac = 1.0 - np.exp(-np.maximum(d["h_ice"], 0.0) / max(1e-6, href))
    margin = np.nanmin(np.abs(ice_frac - thr))
    assert margin >= 1e-9, f"{name}: a cell sits {margin:.3e} from the sea-ice threshold"
    mask = (land == 0) & (ice_frac >= thr)
    m = re.match(r"\[TrueColor\] sea_ice_area≈([0-9.]+), mean_h_ice=([0-9.naif-]+) m", line[0])
    w = np.maximum(np.cos(np.deg2rad(lat_mesh)), 0.0)
    sea_ice = np.array([float((w * mask).sum() / (w.sum() + 1e-15)), float(d["h_ice"][mask].mean()) if mask.any() else 0.0])
    assert m and f"{sea_ice[0]:.3f}" == m.group(1) and f"{sea_ice[1]:.3f}" == m.group(2), (line, sea_ice)
    for x in sea_ice:                                   # the line prints three decimals: stay away from their rounding boundaries
        y = abs(x) * 1e3
        assert not np.isfinite(x) or abs((y - np.floor(y)) - 0.5) / 1e3 > 1e-9, f"{name}: {x!r} sits on a rounding boundary"
    meta = {"case": name, "nlat": NLAT, "nlon": NLON, "env": env, "has_eco": bool(has["eco"]), "use_lai": bool(eco is not None and eco.pop is not None),
            "nb_phyto": int(has["phyto_nb"]), "has_routing": bool(has["routing"]), "t_days": 12.25}
    np.savez_compressed(os.path.join(OUT, f"truecolor_{name}_{NLAT}x{NLON}.npz"), lat=lat, land_mask=land.astype(np.int8),
                        h_ice=d["h_ice"], C_snow=d["C_snow"], cloud=d["cloud"], T_s=d["T_s"], isr=d["isr"], isr_A=d["isr_A"], isr_B=d["isr_B"],
                        eco_f=d["eco_f"], flow=d["flow"], lake_mask=d["lake_mask"], phyto_bands=d["phyto_bands"],
                        rgb=rgb, sea_ice_mask=mask, sea_ice=sea_ice, line=np.array(line[0]), meta=json.dumps(meta), **extra)
    print(f"{name}: sea ice {int(mask.sum())} cells, NaN pixels {int(np.isnan(rgb).any(axis=-1).sum())}, margin {margin:.2e} | {line[0]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(HERE, "..", "..", "reference"))
    ap.add_argument("cases", nargs="*", default=list(CASES))
    a = ap.parse_args()
    root = os.path.abspath(a.reference)
    sys.path.insert(0, root)
    sys.path.insert(0, os.path.join(root, "scripts"))
    os.environ.setdefault("MPLBACKEND", "Agg")
    import run_simulation as rs                         # the reference driver (its main() runs only under __main__)
    from pygcm.ecology import adapter, spectral
    for name in a.cases:
        run_case(name, (rs, adapter, spectral))


if __name__ == "__main__":
    main()
